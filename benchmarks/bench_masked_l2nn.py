#!/usr/bin/env python3
"""Masked fused L2-NN and cross-component NN: 262144 x 128 fp32 blobs, with
G = 64 and G = rows/16 groups.

Per G it times
  (a) masked_l2nn(x, x, adj, group_idxs) with the block-diagonal-complement
      mask (a row may match every group but its own), packed adj, for
      fp32_mode "bf16x1v" and "bf16x2v"
  (b) cross_component_nn(x, labels) (fp32_mode="auto") on the same groups
  (c) what a user had before these ops for the result of (a)/(b): row-chunked
      pairwise_distance + masked_fill + min (the mask of a chunk comes from a
      label comparison, the cheapest way to get it). Unverified.
and once
  (d) unmasked fused_l2nn at the same shape: the ceiling.
It reports the time per call, the share of tiles skipped and the share of rows
that took the exact rescan.

Method: every variant is warmed at the timed shape; each timed window is
synchronised on both sides and holds enough calls to last >= --window seconds;
the variants alternate inside one process for --repeats rounds; the median and
the min..max spread over the rounds are printed as one JSON line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=262_144)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--clusters", type=int, default=64)
    p.add_argument("--groups", type=str, default="64,rows/16")
    p.add_argument("--window", type=float, default=1.0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--baseline-chunk", type=int, default=8192)
    p.add_argument("--skip", type=str, default="",
                   help="comma-separated variant prefixes to leave out")
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd.distance import pairwise_distance
    from raft_amd.neighbors import cross_component_nn, fused_l2nn, masked_l2nn
    from raft_amd.neighbors.epsilon_neighborhood import _pack_rows
    from raft_amd.random import RngState, make_blobs

    m = args.rows
    x, blob, _ = make_blobs(m, args.dim, n_clusters=args.clusters,
                            state=RngState(seed=7), device=dev)
    x = x.contiguous()
    blob = blob.to(torch.int64)
    gen = torch.Generator(device=dev).manual_seed(11)
    skip = tuple(s for s in args.skip.split(",") if s)
    bc = min(args.baseline_chunk, m)
    variants, stats, info = {}, {}, {}

    for spec in args.groups.split(","):
        n_groups = m // int(spec.split("/")[1]) if "/" in spec else int(spec)
        # components inside the blobs: blob id refined by a random sub-id
        sub = max(1, n_groups // args.clusters)
        labels = blob * sub + torch.randint(0, sub, (m,), device=dev, generator=gen)
        perm = torch.argsort(labels, stable=True)
        xs = x[perm].contiguous()
        comp, dense, counts = torch.unique_consecutive(
            labels[perm], return_inverse=True, return_counts=True)
        g = comp.numel()
        ends = counts.cumsum(0)
        adj = torch.empty((m, (g + 31) // 32), dtype=torch.int32, device=dev)
        ids = torch.arange(g, device=dev)
        for r0 in range(0, m, 4096):
            adj[r0:r0 + 4096] = _pack_rows(dense[r0:r0 + 4096, None] != ids[None, :])
        info[spec] = {"groups": g}

        def run_masked(mode, xs=xs, adj=adj, ends=ends, key=spec):
            def f():
                _, _, st = masked_l2nn(xs, xs, adj, ends, fp32_mode=mode,
                                       return_stats=True)
                stats[f"{key}:{mode}"] = st
            return f

        def run_cc(labels=labels, key=spec):
            def f():
                out = cross_component_nn(x, labels)
                stats[f"{key}:cc"] = int(out[0].numel())
            return f

        def run_baseline(xs=xs, dense=dense, g=g, key=spec):
            def f():
                dmin = torch.empty(m, dtype=torch.float32, device=dev)
                amin = torch.empty(m, dtype=torch.int64, device=dev)
                for r0 in range(0, m, bc):
                    r1 = min(r0 + bc, m)
                    d2 = pairwise_distance(xs[r0:r1], xs)
                    d2.masked_fill_(dense[r0:r1, None] == dense[None, :], float("inf"))
                    dmin[r0:r1], amin[r0:r1] = d2.min(dim=1)
                cmin = torch.full((g,), float("inf"), device=dev)
                cmin = cmin.scatter_reduce(0, dense, dmin, "amin")
                stats[f"{key}:baseline"] = float(cmin.sum())
            return f

        variants[f"a_masked_bf16x1v[G={spec}]"] = run_masked("bf16x1v")
        variants[f"a_masked_bf16x2v[G={spec}]"] = run_masked("bf16x2v")
        variants[f"b_cross_component_nn[G={spec}]"] = run_cc()
        variants[f"c_baseline_pairwise_fill_min[G={spec}]"] = run_baseline()

    def run_ceiling():
        fused_l2nn(x, x)
    variants["d_unmasked_fused_l2nn"] = run_ceiling
    variants = {k: v for k, v in variants.items() if not k.startswith(skip or ("\0",))}

    def timed(f, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    reps = {}
    for name, f in variants.items():
        timed(f, 1)                                  # warm this shape
        reps[name] = max(1, math.ceil(args.window / max(timed(f, 1), 1e-6)))
        print(f"# warmed {name}: {reps[name]} calls per window", file=sys.stderr,
              flush=True)

    times = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, f in variants.items():             # alternate in one process
            times[name].append(timed(f, reps[name]))

    shares = {}
    for key, st in stats.items():
        if isinstance(st, dict):
            shares[key] = {"tiles": st["tiles"],
                           "skipped_share": st["tiles_skipped"] / max(st["tiles"], 1),
                           "rescanned_share": st["rescanned"] / m}
    out = {
        "metric": "masked L2-NN seconds per call (fp32 blobs, self join)",
        "rows": m, "dim": args.dim, "clusters": args.clusters, "groups": info,
        "engine_stats": shares,
        "components_found": {k: v for k, v in stats.items() if k.endswith(":cc")},
        "calls_per_window": reps, "repeats": args.repeats,
        "seconds": {
            name: {"median": round(statistics.median(v), 5),
                   "min": round(min(v), 5), "max": round(max(v), 5)}
            for name, v in times.items()},
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
