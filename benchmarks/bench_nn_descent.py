#!/usr/bin/env python3
"""Three ways to the kNN graph cagra_build needs, on one data set: n x 128 fp32
make_blobs rows (the data of bench_ivf_pq.py), K = 64 neighbours per row.

Routes
  * nn_descent(x, K, engine="kernel")
  * brute force: cagra._knn_graph(x, K, "brute_force"), knn(x, x, K + 1) in row chunks
  * IVF-PQ + refine: cagra._knn_graph(x, K, "ivf_pq")

It reports the build time of every route and its recall@K against exact kNN
(brute_force.knn on --sample rows drawn with a seed; a row's own id is left out
of both sides), and for nn_descent the time of a torch-path build when
--torch-path is given.

Method: every route is first run at 8192 rows, which loads the code objects and
lets the libraries pick algorithms; a timed call is synchronised on both sides;
--rounds calls per route, the routes alternating inside a round; median and
min..max printed. A build is one long call (seconds), so a window holds one call.
One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=100_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--centers", type=int, default=1024)
    p.add_argument("--n-samples", type=int, default=32)
    p.add_argument("--max-iterations", type=int, default=20)
    p.add_argument("--sample", type=int, default=10_000, help="rows recall is measured on")
    p.add_argument("--routes", nargs="*", default=["nn_descent", "brute_force", "ivf_pq"])
    p.add_argument("--torch-path", action="store_true")
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd.distance import DistanceType
    from raft_amd.neighbors import cagra as C
    from raft_amd.neighbors import knn, nn_descent
    from raft_amd.random import RngState, make_blobs

    n, d, K = args.rows, args.dim, args.k
    x, _, _ = make_blobs(n, d, n_clusters=args.centers, state=RngState(seed=7), device=dev)
    x = x[torch.randperm(n, device=dev, generator=torch.Generator(dev).manual_seed(1))].contiguous()

    def nnd(t, engine="kernel"):
        return nn_descent(t, K, n_samples=args.n_samples, max_iterations=args.max_iterations,
                          engine=engine)[1]

    def drop_own(ids):                     # [m, K + 1] -> [m, K], as cagra_build does
        own = ids == torch.arange(ids.shape[0], device=dev).unsqueeze(1)
        own[:, K] |= ~own.any(dim=1)
        return ids[~own].reshape(-1, K)

    routes = {"nn_descent": nnd,
              "brute_force": lambda t: drop_own(C._knn_graph(t, K, "brute_force",
                                                             DistanceType.L2Expanded, 0)),
              "ivf_pq": lambda t: drop_own(C._knn_graph(t, K, "ivf_pq",
                                                        DistanceType.L2Expanded, 0))}
    if args.torch_path:
        routes["nn_descent_torch"] = lambda t: nnd(t, "torch")
        args.routes = args.routes + ["nn_descent_torch"]
    routes = {name: routes[name] for name in args.routes}

    def sync_time(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rows = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:args.sample].to(dev)
    exact = knn(x, x[rows], K + 1)[1]
    exact = torch.where(exact == rows.unsqueeze(1), -2, exact)

    out = {"metric": "kNN graph build, seconds and recall@K", "data": "blobs",
           "centers": args.centers, "rows": n, "dim": d, "k": K, "n_samples": args.n_samples,
           "max_iterations": args.max_iterations, "recall_rows": int(rows.numel()),
           "rounds": args.rounds}
    times = {name: [] for name in routes}
    for name, f in routes.items():
        f(x[:8192].contiguous())                                  # warm
    for r in range(args.rounds):
        for name, f in routes.items():                            # alternate
            t, ids = sync_time(lambda: f(x))
            times[name].append(t)
            print(f"# round {r} {name} {t:.2f} s", file=sys.stderr, flush=True)
            if r == 0:
                hit = sum(int((ids[rows[s:s + 512], :, None] == exact[s:s + 512, None, :])
                              .any(dim=2).sum()) for s in range(0, rows.numel(), 512))
                out[name] = {"recall": round(hit / (rows.numel() * K), 4)}
            del ids
    for name, ts in times.items():
        out[name].update(s_median=round(statistics.median(ts), 3), s_min=round(min(ts), 3),
                         s_max=round(max(ts), 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
