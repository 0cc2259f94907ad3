#!/usr/bin/env python3
"""Brute-force kNN over int8 / uint8 rows (csrc/pairwise_i8.hip) against what a
user could do before it: knn on the same values widened to bf16.

Clustered byte data (1024 centres, rounded into 0 .. 255; int8 holds the same
values shifted by -128, which keeps every L2 distance), squared L2. Per shape
and k the two paths alternate in one process: both warmed at shape, then
`--windows` windows per path of as many calls as fill `--window-s` seconds,
each window ended by a device synchronise. One JSON line per (rows, k, dtype)
with the median, minimum and maximum window of each path in queries per
second, and whether the two paths returned the same distances (at d = 128
every squared distance is below 2^24, so the bf16 path is exact as well).
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


def make_bytes(rows, dim, centres, gen, dev):
    """uint8 [rows, dim]: centre + N(0, 16^2), rounded and clamped, in chunks."""
    out = torch.empty((rows, dim), dtype=torch.uint8, device=dev)
    for s in range(0, rows, 1_000_000):
        e = min(s + 1_000_000, rows)
        lab = torch.randint(0, centres.shape[0], (e - s,), generator=gen, device=dev)
        noise = torch.randn((e - s, dim), generator=gen, device=dev) * 16.0
        out[s:e] = (centres[lab] + noise).round_().clamp_(0, 255).to(torch.uint8)
    return out


def windows(fn, n_windows, window_s, queries):
    """queries/s of n_windows windows of fn(), sized from one timed call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(1, int(window_s / max(time.perf_counter() - t0, 1e-6)))
    rates = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        rates.append(queries * calls / (time.perf_counter() - t0))
    return rates, calls


def summary(rates):
    return {"median": round(statistics.median(rates), 1), "min": round(min(rates), 1),
            "max": round(max(rates), 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="1000000,10000000")
    p.add_argument("--k", default="10,64")
    p.add_argument("--dtypes", default="int8,uint8")
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--queries", type=int, default=10_000)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--window-s", type=float, default=1.0)
    args = p.parse_args()

    assert torch.cuda.is_available(), "bench_knn_int8 needs a GPU"
    dev = torch.device("cuda")
    from raft_amd.neighbors.brute_force import BruteForceIndex

    gen = torch.Generator(device=dev).manual_seed(11)
    centres = torch.rand((1024, args.dim), generator=gen, device=dev) * 128.0 + 64.0
    for rows in (int(r) for r in args.rows.split(",")):
        xu = make_bytes(rows, args.dim, centres, gen, dev)
        qu = make_bytes(args.queries, args.dim, centres, gen, dev)
        for name in args.dtypes.split(","):
            if name == "int8":
                x, q = (xu.int() - 128).to(torch.int8), (qu.int() - 128).to(torch.int8)
            else:
                x, q = xu, qu
            index_i8 = BruteForceIndex(x)
            index_bf = BruteForceIndex(x.bfloat16())
            q_bf = q.bfloat16()
            for k in (int(v) for v in args.k.split(",")):
                d_i8, _ = index_i8.search(q, k)
                d_bf, _ = index_bf.search(q_bf, k)
                same = bool(torch.equal(d_i8, d_bf))
                r_i8, r_bf = [], []
                for _ in range(args.windows):  # the two paths alternate
                    a, calls_i8 = windows(lambda: index_i8.search(q, k), 1,
                                          args.window_s, args.queries)
                    b, calls_bf = windows(lambda: index_bf.search(q_bf, k), 1,
                                          args.window_s, args.queries)
                    r_i8 += a
                    r_bf += b
                print(json.dumps({
                    "bench": "knn_int8", "rows": rows, "dim": args.dim, "k": k,
                    "queries": args.queries, "dtype": name,
                    "i8_qps": summary(r_i8), "bf16_widened_qps": summary(r_bf),
                    "i8_over_bf16": round(statistics.median(r_i8)
                                          / statistics.median(r_bf), 3),
                    "calls_per_window": [calls_i8, calls_bf],
                    "distances_equal": same}), flush=True)
            del index_i8, index_bf
        del xu


if __name__ == "__main__":
    main()
