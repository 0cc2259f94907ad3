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

With --dtype (a comma-separated subset of fp32, bf16, int8, uint8) it instead
compares the row dtypes: rows and queries are quantised once into 0 .. 255,
every requested dtype gets an index over those SAME values, centroids and list
assignment (int8 shifted by -128, which keeps every L2 distance), and per
n_probes (k = the first of --k) the dtypes alternate in one process: whole-call
queries per second, the staged scan and select seconds, and whether the
distances equal those of the first dtype bit for bit over the same probes.
--qg then sweeps every requested dtype.

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
    p.add_argument("--dtype", type=str, default="fp32",
                   help="comma-separated row dtypes (fp32, bf16, int8, uint8); anything "
                        "but the default compares them over the same quantised rows")
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

    torch_dtypes = {"fp32": torch.float32, "bf16": torch.bfloat16, "int8": torch.int8,
                    "uint8": torch.uint8}
    dtypes = args.dtype.split(",")
    if any(t not in torch_dtypes for t in dtypes):
        raise SystemExit(f"--dtype takes a comma-separated subset of {list(torch_dtypes)}")

    def compare_dtypes(data, x, q, params):
        """The same QUANTISED rows in every requested dtype: rows and queries
        are scaled and rounded once into 0 .. 255; fp32, bf16 and uint8 hold
        those values (integers up to 255 are exact in bf16), int8 holds them
        shifted by -128, which leaves every L2 distance unchanged. The
        centroids are trained once on the fp32 values (shifted for int8), so
        all indices hold the same lists."""
        lo, hi = float(torch.minimum(x.min(), q.min())), float(torch.maximum(x.max(), q.max()))
        quant = lambda t: ((t - lo) * (255.0 / (hi - lo))).round_().clamp_(0, 255)
        xq, qq = quant(x), quant(q)
        build_s, base = sync_time(lambda: ivf_flat_build(xq, params))
        cast = lambda t, name: ((t - 128.0) if name == "int8" else t).to(torch_dtypes[name])
        # one assignment for all: every index packs the rows under base's labels
        labels = torch.empty(n, dtype=torch.int64, device=dev)
        slots = (base.indices >= 0).nonzero().flatten()
        labels[base.indices[slots]] = torch.searchsorted(
            base.list_offsets[1:].contiguous(), slots, right=True)
        ids = torch.arange(n, device=dev)
        index, queries = {}, {}
        for t in dtypes:
            cent = base.centroids - 128.0 if t == "int8" else base.centroids
            index[t] = base if t == "fp32" else ivf_flat.IvfFlatIndex(
                cent, *ivf_flat._pack(cast(xq, t), ids, labels, args.n_lists, d),
                base.metric, d, n)
            queries[t] = cast(qq, t)
        del xq, qq, labels, ids
        out = {"metric": "IVF-Flat row dtypes over the same quantised rows",
               "data": data, "rows": n, "dim": d, "queries": nq, "n_lists": args.n_lists,
               "build_s_fp32": round(build_s, 3), "reps": args.reps, "rounds": args.rounds,
               "k": ks[0], "index_bytes": {t: index[t].data.numel() * index[t].data.element_size()
                                           for t in dtypes}, "n_probes": {}}
        k = ks[0]
        for n_probes in probe_counts:
            call = {t: (lambda t=t: ivf_flat_search(index[t], queries[t], k, n_probes))
                    for t in dtypes}
            ref = ivf_flat_search(index[dtypes[0]], queries[dtypes[0]], k, n_probes,
                                  return_probes=True)
            ts = {t: [] for t in dtypes}
            stages = {t: [] for t in dtypes}
            row = {}
            for t in dtypes:                                              # warm
                call[t]()
                # same probes, same rows: sums below 2^24 are exact in fp32 too
                got = ivf_flat_search(index[t], queries[t], k, probes=ref[2])
                row[t] = {"dists_equal_first_dtype": bool(torch.equal(got[0], ref[0]))}
            for _ in range(args.rounds):
                for t in dtypes:                                          # alternate
                    dt, _ = sync_time(lambda: [call[t]() for _ in range(args.reps)])
                    ts[t].append(dt / args.reps)
                    stages[t].append(staged_call(index[t], queries[t], k, n_probes))
            for t in dtypes:
                row[t].update(rate(ts[t]))
                for s in ("scan_s", "select_s"):
                    v = [c[s] for c in stages[t]]
                    row[t][s] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            out["n_probes"][n_probes] = row
            print(f"# {data} n_probes={n_probes}: {row}", file=sys.stderr, flush=True)
        if qgs:
            sweep = {}
            for t in dtypes:
                scans = {g: [] for g in qgs}
                for g in qgs:
                    staged_call(index[t], queries[t], 10, 32, qg=g)           # warm
                for _ in range(args.rounds):
                    for g in qgs:                                         # alternate
                        scans[g].append(
                            staged_call(index[t], queries[t], 10, 32, qg=g)["scan_s"])
                sweep[t] = {g: {"median": round(statistics.median(v), 5), "min": min(v),
                                "max": max(v)} for g, v in scans.items()}
            out["qg_scan_s_at_32_probes"] = sweep
        print(json.dumps(out), flush=True)

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
        if dtypes != ["fp32"]:
            compare_dtypes(data, x, q, params)
            del x, q
            torch.cuda.empty_cache()
            continue

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
