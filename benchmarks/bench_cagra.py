#!/usr/bin/env python3
"""CAGRA beside IVF-PQ + refine on one data set: 1M x 128 fp32 make_blobs rows
(1024 centers) and 10,000 held-out queries, the data of bench_ivf_pq.py.

It reports
  * the build time of the CAGRA index per stage: the kNN graph (build_algo
    "auto": IVF-PQ + refine above 131072 rows), the detour-count prune kernel,
    and the reverse-edge merge in torch,
  * queries per second and recall@10 of cagra_search(engine="kernel") at
    itopk_size 32 / 64 / 128 / 256 and search_width 1 and 4, with the
    hash_slots the call picked, the dynamic LDS of a block and the blocks per
    CU that LDS allows (160 KiB per CU),
  * queries per second and recall@10 of ivf_pq_search(..., dataset=x,
    refine_ratio=r) for r = 4 and 40, run in the same session.

Method (as bench_ivf_pq.py): every call is warmed at the timed shape; a timed
window is synchronised on both sides and holds --reps calls; --rounds windows,
the calls alternating inside a round; median and min..max printed. One JSON
line.

With the default 1024 well-separated centers the kNN graph has no edges between
clusters, so a walk finds a query's neighbours only if a seed fell into its
cluster: recall is then about itopk_size / 1024 whatever the search width.
--centers 1 measures one connected cloud.
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

LDS_PER_CU = 160 * 1024


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--queries", type=int, default=10_000)
    p.add_argument("--centers", type=int, default=1024,
                   help="make_blobs centers; 1 gives one connected cloud")
    p.add_argument("--graph-degree", type=int, default=64)
    p.add_argument("--intermediate-graph-degree", type=int, default=128)
    p.add_argument("--itopk", type=int, nargs="*", default=[32, 64, 128, 256])
    p.add_argument("--search-width", type=int, nargs="*", default=[1, 4])
    p.add_argument("--n-lists", type=int, default=1024)
    p.add_argument("--n-probes", type=int, default=32)
    p.add_argument("--refine-ratio", type=int, nargs="*", default=[4, 40])
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd._ext import require_ext
    from raft_amd.distance import DistanceType
    from raft_amd.neighbors import (BruteForceIndex, CagraIndex, IvfPqParams, cagra_search,
                                    ivf_pq_build, ivf_pq_search)
    from raft_amd.neighbors import cagra as C
    from raft_amd.random import RngState, make_blobs

    n, d, nq, k = args.rows, args.dim, args.queries, args.k

    def sync_time(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    allx, _, _ = make_blobs(n + nq, d, n_clusters=args.centers, state=RngState(seed=7),
                            device=dev)
    allx = allx[torch.randperm(n + nq, device=dev,
                               generator=torch.Generator(dev).manual_seed(1))]
    x, q = allx[:n].contiguous(), allx[n:].contiguous()
    del allx

    # the stages of cagra_build, timed one by one
    kd, g = min(args.intermediate_graph_degree, n - 1), args.graph_degree
    algo = "brute_force" if n <= C._AUTO_BRUTE_FORCE_ROWS else "ivf_pq"
    knn_s, nbrs = sync_time(lambda: C._knn_graph(x, kd, algo, DistanceType.L2Expanded, 0))
    own = nbrs == torch.arange(n, device=dev).unsqueeze(1)
    own[:, kd] |= ~own.any(dim=1)
    knn_graph = nbrs[~own].reshape(n, kd).int().contiguous()
    del nbrs, own
    pruned = torch.empty((n, g), dtype=torch.int32, device=dev)
    require_ext().cagra_prune(knn_graph[:4096].contiguous(), pruned[:4096])        # warm
    prune_s, _ = sync_time(lambda: require_ext().cagra_prune(knn_graph, pruned))
    merge_s, graph = sync_time(lambda: C._merge_reverse(pruned.long()).int())
    seeds = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:512].int().to(dev)
    index = CagraIndex(x, graph, seeds, "sqeuclidean")
    print(f"# cagra built: knn graph ({algo}) {knn_s:.2f} s, prune {prune_s:.3f} s, "
          f"merge {merge_s:.3f} s", file=sys.stderr, flush=True)

    pq_s, pq = sync_time(lambda: ivf_pq_build(x, IvfPqParams(n_lists=args.n_lists)))
    bf_ids = BruteForceIndex(x).search(q, k)[1]

    out = {"metric": "CAGRA vs IVF-PQ + refine, queries per second", "data": "blobs",
           "centers": args.centers, "rows": n, "dim": d, "queries": nq, "k": k,
           "reps": args.reps, "rounds": args.rounds,
           "cagra_build": {"algo": algo, "knn_graph_s": round(knn_s, 3),
                           "prune_s": round(prune_s, 4), "merge_s": round(merge_s, 4),
                           "graph_degree": g, "intermediate_graph_degree": kd,
                           "edges_present": round(float((graph >= 0).float().mean()), 4)},
           "ivf_pq_build_s": round(pq_s, 3)}
    calls = {}
    for L in args.itopk:
        for w in args.search_width:
            name = f"cagra_itopk{L}_w{w}"
            calls[name] = lambda L=L, w=w: cagra_search(index, q, k, itopk_size=L,
                                                        search_width=w, engine="kernel")
            H = C.auto_hash_slots(L, w * g, min(L, 512), L // w + 10)
            lds = require_ext().cagra_search_lds_bytes(d, 4, L, w * g, min(L, 512), H, w)
            out[name] = {"hash_slots": H, "lds_bytes": lds,
                         "blocks_per_cu_by_lds": min(8, LDS_PER_CU // lds)}
    for r in args.refine_ratio:
        name = f"ivf_pq_refine_x{r}"
        calls[name] = lambda r=r: ivf_pq_search(pq, q, k, args.n_probes, dataset=x,
                                                refine_ratio=r)
        out[name] = {"n_probes": args.n_probes, "n_cand": k * r}
    times = {name: [] for name in calls}
    for name, f in calls.items():
        ids = f()[1]                                          # warm this shape
        hit = 0
        for s in range(0, nq, 1024):
            hit += int((ids[s:s + 1024, :, None] == bf_ids[s:s + 1024, None, :])
                       .any(dim=2).sum())
        out[name]["recall"] = round(hit / (nq * k), 4)
    for _ in range(args.rounds):
        for name, f in calls.items():                         # alternate
            t, _ = sync_time(lambda: [f() for _ in range(args.reps)])
            times[name].append(t / args.reps)
    for name, ts in times.items():
        out[name].update(
            qps_median=round(nq / statistics.median(ts)), qps_min=round(nq / max(ts)),
            qps_max=round(nq / min(ts)), ms_median=round(1e3 * statistics.median(ts), 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
