#!/usr/bin/env python3
"""Epsilon-neighborhood throughput: 200k x 200k x 128 fp32 blobs, mean degree ~64.

Reports pairs/s for
  (a) eps_neighbors_l2sq packed, fp32_mode="bf16x1v"
  (b) eps_neighbors_l2sq packed, fp32_mode="bf16x2v"
  (c) eps_neighbors_l2sq_csr (fp32_mode="auto")
  (d) the baseline a user had before this op existed: ext.pairwise_l2_mfma
      tiles into a reused fp32 buffer, then `<= eps_sq` and a row sum, under
      the same split (d1: 1 slice, d2: 2 slices). Unverified.
and the fraction of pairs that took the exact fp32 recheck in (a) and (b).

Method: every variant is warmed at the timed shape; each timed window is
synchronised on both sides and holds enough sweeps to last >= --window
seconds; the variants alternate inside one process for --repeats rounds; the
median and the min..max spread over the rounds are printed as one JSON line.
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
    p.add_argument("--rows", type=int, default=200_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--clusters", type=int, default=64)
    p.add_argument("--degree", type=float, default=64.0)
    p.add_argument("--window", type=float, default=1.0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--baseline-chunk", type=int, default=8192)
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd._ext import require_ext
    from raft_amd.neighbors import eps_neighbors_l2sq, eps_neighbors_l2sq_csr
    from raft_amd.linalg.split_bf16 import split_bf16_slices
    from raft_amd.random import RngState, make_blobs
    ext = require_ext()

    n = args.rows
    state = RngState(seed=7)
    x, _, centers = make_blobs(n, args.dim, n_clusters=args.clusters,
                               state=state, device=dev)
    y, _, _ = make_blobs(n, args.dim, centers=centers, state=state, device=dev)
    x, y = x.contiguous(), y.contiguous()

    # eps_sq from a sample: the quantile that gives the requested mean degree
    s = min(n, 4096)
    d2s = torch.cdist(x[:s].double(), y[:s].double()) ** 2
    q = min(max(args.degree / n, 1.0 / d2s.numel()), 1.0)
    kth = max(1, int(round(q * d2s.numel())))
    eps = float(torch.tensor(float(d2s.flatten().kthvalue(kth).values),
                             dtype=torch.float32))
    del d2s

    pairs = float(n) * float(n)
    stats = {}

    def run_packed(mode):
        def f():
            _, vd, st = eps_neighbors_l2sq(x, y, eps, packed=True, fp32_mode=mode,
                                           return_stats=True)
            stats[mode] = (st["rechecked"], int(vd[-1]))
        return f

    def run_csr():
        indptr, indices, vd = eps_neighbors_l2sq_csr(x, y, eps)
        stats["csr"] = int(vd[-1])

    xn = (x * x).sum(dim=1).contiguous()
    yn = (y * y).sum(dim=1).contiguous()
    bc = min(args.baseline_chunk, n)
    buf = torch.empty((bc, n), dtype=torch.float32, device=dev)
    slices = {k: (split_bf16_slices(x, k), split_bf16_slices(y, k)) for k in (1, 2)}

    def run_baseline(nsl):
        xs, ys = slices[nsl]

        def f():
            deg = torch.empty(n, dtype=torch.int64, device=dev)
            for r0 in range(0, n, bc):
                r1 = min(r0 + bc, n)
                ext.pairwise_l2_mfma([t[r0:r1] for t in xs], ys, xn[r0:r1], yn,
                                     out=buf)
                deg[r0:r1] = (buf[: r1 - r0] <= eps).sum(dim=1)
            stats[f"baseline{nsl}"] = int(deg.sum())
        return f

    variants = {
        "a_packed_bf16x1v": run_packed("bf16x1v"),
        "b_packed_bf16x2v": run_packed("bf16x2v"),
        "c_csr_auto": run_csr,
        "d1_baseline_1slice": run_baseline(1),
        "d2_baseline_2slice": run_baseline(2),
    }

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

    rates = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, f in variants.items():             # alternate in one process
            rates[name].append(pairs / timed(f, reps[name]))

    out = {
        "metric": "eps-neighborhood pairs/s (fp32 blobs)",
        "rows": n, "dim": args.dim, "clusters": args.clusters,
        "eps_sq": eps, "pairs_per_sweep": pairs,
        "mean_degree": stats["bf16x2v"][1] / n,
        "recheck_fraction": {m: stats[m][0] / pairs for m in ("bf16x1v", "bf16x2v")},
        "neighbors": {"bf16x1v": stats["bf16x1v"][1], "bf16x2v": stats["bf16x2v"][1],
                      "csr": stats["csr"], "baseline_1slice": stats["baseline1"],
                      "baseline_2slice": stats["baseline2"]},
        "sweeps_per_window": reps, "repeats": args.repeats,
        "Gpairs_per_sec": {
            name: {"median": round(statistics.median(v) / 1e9, 2),
                   "min": round(min(v) / 1e9, 2), "max": round(max(v) / 1e9, 2)}
            for name, v in rates.items()},
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
