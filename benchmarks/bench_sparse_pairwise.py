#!/usr/bin/env python3
"""Sparse (CSR x CSR) pairwise distances, 8192 x 8192 rows over d = 65536
columns with about 64 stored values per row, fp32, 1 GPU: cosine and L1
through sparse_pairwise_distance under each LDS staging strategy ("hash",
"dense", and whatever "auto" resolves to), against what the library could do
before the sparse kernels existed:

  densify   csr_to_dense on both sides, then the dense pairwise_distance
            (the two [rows, d] fp32 matrices take 2 x 2 GiB at this shape);
  spmm      inner product only: torch.sparse.mm(A, B^T) densified.

Metric: milliseconds per call through the public entry points, row statistics
and output allocation included; the densify baseline includes the
densification, which a caller holding CSR data has to pay. Per variant:
warm-up calls, then --repeats timed windows (device events around the window);
the MEDIAN window is reported with min/max as the spread. A window holds as
many calls as fill --window-s seconds (sized from a timed warm-up call). The
variants are interleaved per repeat, so drift on a shared host hits all alike.
Before timing, every variant's output is compared with the densify baseline.

Usage: python benchmarks/bench_sparse_pairwise.py [--rows 8192] [--cols 65536]
         [--row-nnz 64] [--warmup 2] [--window-s 0.3] [--repeats 5]
         [--metrics cosine,l1,inner_product] [--strategies auto,hash,dense]
         [--hash-capacities 128,256] [--no-densify]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_csr(rows, cols, row_nnz, seed, dev):
    """Random CSR: per row, row_nnz uniform column draws with the repeats
    dropped (sorted unique ids, so rows are slightly ragged), values in
    [0.1, 1.1)."""
    from raft_amd.sparse import CSR
    g = torch.Generator(device="cpu").manual_seed(seed)
    draws = max(1, row_nnz)
    c = torch.randint(0, cols, (rows, draws), generator=g).sort(dim=1).values
    keep = torch.ones_like(c, dtype=torch.bool)
    keep[:, 1:] = c[:, 1:] != c[:, :-1]
    indptr = torch.zeros(rows + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    idx = c[keep]
    vals = torch.rand(idx.numel(), generator=g) + 0.1
    return CSR(indptr.to(torch.int32).to(dev), idx.to(torch.int32).to(dev),
               vals.to(dev), rows, cols)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=8192)
    p.add_argument("--cols", type=int, default=65536)
    p.add_argument("--row-nnz", type=int, default=64)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--window-s", type=float, default=0.3)
    p.add_argument("--iters", type=int, default=0, help="0 = size from --window-s")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--metrics", default="cosine,l1,inner_product")
    p.add_argument("--strategies", default="auto,hash,dense")
    p.add_argument("--hash-capacities", default="",
                   help="comma list: also time the hash strategy at these capacities")
    p.add_argument("--no-densify", action="store_true",
                   help="skip the densify baseline (and the output check)")
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda")
    from raft_amd._ext import require_ext
    from raft_amd.distance import pairwise_distance
    from raft_amd.sparse import csr_to_dense, sparse_pairwise_distance

    require_ext()
    a = make_csr(args.rows, args.cols, args.row_nnz, 1, dev)
    b = make_csr(args.rows, args.cols, args.row_nnz, 2, dev)
    bt = b.to_torch_sparse().to_sparse_coo().t().coalesce().to_sparse_csr()
    at = a.to_torch_sparse()

    def sparse_call(metric, strategy, cap=None):
        return lambda: sparse_pairwise_distance(a, b, metric, strategy=strategy,
                                                hash_capacity=cap)

    def densify_call(metric):
        return lambda: pairwise_distance(csr_to_dense(a), csr_to_dense(b), metric)

    def spmm_call():
        return lambda: torch.sparse.mm(at, bt).to_dense()

    variants = {}
    spmm_error = None
    for metric in args.metrics.split(","):
        for s in args.strategies.split(","):
            variants[f"{metric}/{s}"] = sparse_call(metric, s)
        for cap in filter(None, args.hash_capacities.split(",")):
            variants[f"{metric}/hash@{cap}"] = sparse_call(metric, "hash", int(cap))
        if not args.no_densify:
            variants[f"{metric}/densify"] = densify_call(metric)
        if metric == "inner_product":
            try:  # CSR x CSR products are not available on every torch build
                spmm_call()()
                variants[f"{metric}/spmm"] = spmm_call()
            except RuntimeError as e:
                spmm_error = str(e).splitlines()[0]

    # outputs at the timed size: every variant against the densify baseline
    max_abs_diff = {}
    if not args.no_densify:
        for metric in args.metrics.split(","):
            ref = variants[f"{metric}/densify"]()
            for name, fn in variants.items():
                if name.startswith(metric + "/") and not name.endswith("/densify"):
                    max_abs_diff[name] = float((fn() - ref).abs().max())
            del ref
        torch.cuda.empty_cache()

    def window(fn, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3 / iters

    iters = {}
    for name, fn in variants.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        iters[name] = args.iters or max(2, int(args.window_s / window(fn, 2)) + 1)

    windows = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            windows[name].append(window(fn, iters[name]))

    results = {}
    for name, w in windows.items():
        results[name] = {
            "median_ms": round(statistics.median(w) * 1e3, 3),
            "min_ms": round(min(w) * 1e3, 3),
            "max_ms": round(max(w) * 1e3, 3),
            "iters_per_window": iters[name],
        }
    for name, r in results.items():
        metric = name.split("/")[0]
        for base in ("densify", "spmm"):
            ref = results.get(f"{metric}/{base}")
            if ref is not None and not name.endswith("/" + base):
                r[f"speedup_vs_{base}"] = round(ref["median_ms"] / r["median_ms"], 3)
    print(json.dumps({
        "metric": "sparse pairwise distance, ms per call, fp32, median of windows",
        "rows": args.rows, "cols": args.cols,
        "mean_row_nnz": round(a.nnz / max(args.rows, 1), 2),
        "warmup": args.warmup, "window_s": args.window_s, "repeats": args.repeats,
        "max_abs_diff_vs_densify": max_abs_diff,
        "spmm_error": spmm_error,
        "results": results,
    }), flush=True)


if __name__ == "__main__":
    main()
