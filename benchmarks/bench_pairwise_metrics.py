#!/usr/bin/env python3
"""Pairwise-distance metrics beyond L2: KL divergence, Jensen-Shannon,
Bray-Curtis, Haversine (register-tiled / elementwise kernels) and Hellinger,
Russel-Rao, Jaccard, Dice (GEMM + fused epilogue), 8192 x 8192 x 128 fp32,
1 GPU. The L1 and Canberra kernels (32x32 tile, csrc/pairwise.hip) are timed
at the same shape as yardsticks.

Metric: Gdist/s (distance values produced per second) through the public
pairwise_distance call, output allocation included. Per metric: warm-up calls,
then --repeats timed windows (device events around the window); the MEDIAN
window is reported with min/max as the spread. A window holds as many calls
as fill --window-s seconds (sized from a timed warm-up call; --iters N fixes
the count instead) — a millisecond window would measure the clock. The
metrics are interleaved per repeat, so drift on a shared host hits all alike.
Haversine is d = 2 by definition.

Usage: python benchmarks/bench_pairwise_metrics.py [--rows 8192] [--dim 128]
         [--warmup 3] [--window-s 0.2] [--iters 0] [--repeats 7]
         [--fp32-mode auto]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW = ["kl_divergence", "jensenshannon", "braycurtis", "haversine",
       "hellinger", "russelrao", "jaccard", "dice"]
YARDSTICKS = ["l1", "canberra"]


def make_inputs(metric, rows, dim, dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    if metric == "haversine":
        lat = (torch.rand(rows, generator=g) - 0.5) * 3.14159
        lon = (torch.rand(rows, generator=g) - 0.5) * 6.28318
        return torch.stack([lat, lon], dim=1).to(dev)
    if metric in ("russelrao", "jaccard", "dice"):
        return (torch.rand(rows, dim, generator=g) < 0.3).float().to(dev)
    x = torch.rand(rows, dim, generator=g) + 1e-3
    return (x / x.sum(dim=1, keepdim=True)).to(dev)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=8192)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--window-s", type=float, default=0.2)
    p.add_argument("--iters", type=int, default=0, help="0 = size from --window-s")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--fp32-mode", default="auto")
    p.add_argument("--metrics", default=",".join(NEW + YARDSTICKS))
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda")
    from raft_amd._ext import require_ext
    from raft_amd.distance import pairwise_distance

    require_ext()
    metrics = args.metrics.split(",")
    data = {m: make_inputs(m, args.rows, args.dim, dev) for m in metrics}

    def call(m):
        return pairwise_distance(data[m], data[m], m, fp32_mode=args.fp32_mode)

    def window(m, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call(m)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3 / iters

    iters = {}
    for m in metrics:
        for _ in range(args.warmup):
            call(m)
        torch.cuda.synchronize()
        iters[m] = args.iters or max(5, int(args.window_s / window(m, 3)) + 1)

    windows = {m: [] for m in metrics}
    for _ in range(args.repeats):
        for m in metrics:
            windows[m].append(window(m, iters[m]))

    n_dist = args.rows * args.rows
    results = {}
    for m in metrics:
        w = windows[m]
        results[m] = {
            "gdist_per_s": round(n_dist / statistics.median(w) / 1e9, 3),
            "gdist_per_s_min": round(n_dist / max(w) / 1e9, 3),
            "gdist_per_s_max": round(n_dist / min(w) / 1e9, 3),
            "median_ms": round(statistics.median(w) * 1e3, 3),
            "iters_per_window": iters[m],
            "dim": 2 if m == "haversine" else args.dim,
        }
    print(json.dumps({
        "metric": "pairwise metric throughput (Gdist/s), fp32, median of windows",
        "rows": args.rows, "dim": args.dim, "fp32_mode": args.fp32_mode,
        "warmup": args.warmup, "window_s": args.window_s, "repeats": args.repeats,
        "results": results,
    }), flush=True)


if __name__ == "__main__":
    main()
