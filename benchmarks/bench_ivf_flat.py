#!/usr/bin/env python3
"""IVF-Flat against brute-force kNN: 1M x 128 fp32, n_lists = 1024, 10,000
queries, on make_blobs data (1024 centers) and on uniform-random data.

Per data set it reports
  * the index build time (k-means training + assignment + packing),
  * BruteForceIndex.search queries per second at k = 10 and k = 64,
  * for k in {10, 64} x n_probes in {1, 8, 32, 128}: IVF-Flat queries per
    second (the whole ivf_flat_search call), recall@k against the brute-force
    ids, and one staged call with a device synchronise around the list-scan
    kernel launch (with the device-side pair sort that feeds it) and around
    the select, so the two shares can be read separately,
  * the smallest n_probes whose recall reaches --recall-target and the ratio
    of IVF-Flat to brute-force queries per second there,
  * with --qg a,b,c: the staged scan time of every query-group size at
    n_probes = 32, k = 10, alternating in one process.

Method: every configuration is warmed at the timed shape; a timed window is
synchronised on both sides and holds --reps calls; --rounds windows per
configuration, median and min..max printed. Queries are held-out rows of the
same distribution. One JSON line per data set.
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
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--queries", type=int, default=10_000)
    p.add_argument("--n-lists", type=int, default=1024)
    p.add_argument("--data", type=str, default="blobs,uniform")
    p.add_argument("--k", type=str, default="10,64")
    p.add_argument("--n-probes", type=str, default="1,8,32,128")
    p.add_argument("--qg", type=str, default="",
                   help="comma-separated query-group sizes to compare (4, 8, 16, 32)")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--recall-target", type=float, default=0.95)
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd.neighbors import (BruteForceIndex, IvfFlatParams, ivf_flat,
                                    ivf_flat_build, ivf_flat_search)
    from raft_amd.random import RngState, make_blobs

    n, d, nq = args.rows, args.dim, args.queries
    ks = [int(v) for v in args.k.split(",")]
    probe_counts = [int(v) for v in args.n_probes.split(",")]
    qgs = [int(v) for v in args.qg.split(",") if v]

    def sync_time(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def windows(f):
        f()                                           # warm this shape
        ts = []
        for _ in range(args.rounds):
            t, _ = sync_time(lambda: [f() for _ in range(args.reps)])
            ts.append(t / args.reps)
        return ts

    def rate(ts):
        return {"qps_median": round(nq / statistics.median(ts)),
                "qps_min": round(nq / max(ts)), "qps_max": round(nq / min(ts))}

    # staged call: synchronise around the scan and around the select
    stage = {"scan": 0.0, "select": 0.0}
    scan_fn, select_fn = ivf_flat._scan_kernel, ivf_flat._select

    def staged(name, fn):
        def wrapped(*a, **kw):
            t, out = sync_time(lambda: fn(*a, **kw))
            stage[name] += t
            return out
        return wrapped

    def staged_call(index, q, k, n_probes, **kw):
        stage["scan"] = stage["select"] = 0.0
        ivf_flat._scan_kernel = staged("scan", scan_fn)
        ivf_flat._select = staged("select", select_fn)
        try:
            total, _ = sync_time(lambda: ivf_flat_search(index, q, k, n_probes, **kw))
        finally:
            ivf_flat._scan_kernel, ivf_flat._select = scan_fn, select_fn
        return {"total_s": round(total, 5), "scan_s": round(stage["scan"], 5),
                "select_s": round(stage["select"], 5)}

    for data in args.data.split(","):
        if data == "blobs":
            allx, _, _ = make_blobs(n + nq, d, n_clusters=1024, state=RngState(seed=7),
                                    device=dev)
            allx = allx[torch.randperm(n + nq, device=dev,
                                       generator=torch.Generator(dev).manual_seed(1))]
        elif data == "uniform":
            allx = torch.rand((n + nq, d), device=dev,
                              generator=torch.Generator(dev).manual_seed(2))
        else:
            raise SystemExit(f"unknown data set {data!r}")
        x, q = allx[:n].contiguous(), allx[n:].contiguous()
        del allx

        params = IvfFlatParams(n_lists=args.n_lists)
        ivf_flat_build(x[:max(args.n_lists * 8, n // 16)], params)      # warm
        build_s, index = sync_time(lambda: ivf_flat_build(x, params))
        sizes = index.list_sizes
        out = {"metric": "IVF-Flat vs brute-force kNN, queries per second",
               "data": data, "rows": n, "dim": d, "queries": nq,
               "n_lists": args.n_lists, "build_s": round(build_s, 3),
               "list_size_min_mean_max": [int(sizes.min()), round(float(n) / args.n_lists),
                                          int(sizes.max())],
               "reps": args.reps, "rounds": args.rounds, "k": {}}
        print(f"# {data}: built in {build_s:.2f} s", file=sys.stderr, flush=True)

        bf = BruteForceIndex(x)
        for k in ks:
            bf_ts = windows(lambda: bf.search(q, k))
            bf_ids = bf.search(q, k)[1]
            rows = {}
            for n_probes in probe_counts:
                ts = windows(lambda: ivf_flat_search(index, q, k, n_probes))
                ids = ivf_flat_search(index, q, k, n_probes)[1]
                hit = 0
                for s in range(0, nq, 1024):
                    hit += int((ids[s:s + 1024, :, None] == bf_ids[s:s + 1024, None, :])
                               .any(dim=2).sum())
                rows[n_probes] = dict(rate(ts), recall=round(hit / (nq * k), 4),
                                      staged=staged_call(index, q, k, n_probes))
                print(f"# {data} k={k} n_probes={n_probes}: {rows[n_probes]}",
                      file=sys.stderr, flush=True)
            reached = [m for m in probe_counts if rows[m]["recall"] >= args.recall_target]
            entry = {"brute_force": rate(bf_ts), "ivf_flat": rows,
                     "n_probes_at_target": reached[0] if reached else None}
            if reached:
                entry["ivf_over_brute_force_at_target"] = round(
                    rows[reached[0]]["qps_median"] / entry["brute_force"]["qps_median"], 3)
            out["k"][k] = entry

        if qgs:
            scans = {g: [] for g in qgs}
            for g in qgs:
                staged_call(index, q, 10, 32, qg=g)                       # warm
            for _ in range(args.rounds):
                for g in qgs:                                             # alternate
                    scans[g].append(staged_call(index, q, 10, 32, qg=g)["scan_s"])
            out["qg_scan_s_at_32_probes"] = {
                g: {"median": round(statistics.median(v), 5), "min": min(v), "max": max(v)}
                for g, v in scans.items()}
        print(json.dumps(out), flush=True)
        del index, bf, x, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
