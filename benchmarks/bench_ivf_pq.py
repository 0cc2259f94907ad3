#!/usr/bin/env python3
"""IVF-PQ against IVF-Flat on one data set and one n_probes: 1M x 128 fp32
make_blobs rows (1024 centers), n_lists = 1024, 10,000 held-out queries.

It reports
  * the build time of both indices (IVF-PQ: coarse k-means, codebook training,
    encode, packing) and the bytes per row they store,
  * queries per second of the whole ivf_pq_search and ivf_flat_search calls at
    k = 10 and the given n_probes,
  * recall@10 of both against the brute-force ids. IVF-PQ ranks by the
    distance to the reconstructed rows; the plain search is NOT re-ranked,
  * per --refine-ratio r: queries per second and recall@10 of
    ivf_pq_search(..., dataset=x, refine_ratio=r), and the time of refine alone
    on that search's k * r candidates with engine="kernel" and engine="torch"
    (and the share of result slots in which the two return the same id).

Method (as bench_ivf_flat.py): every call is warmed at the timed shape; a timed
window is synchronised on both sides and holds --reps calls (--refine-reps of
refine alone); --rounds windows,
the calls alternating inside a round; median and min..max printed. One JSON
line.
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
    p.add_argument("--pq-dim", type=int, default=0)
    p.add_argument("--pq-bits", type=int, choices=(4, 8), default=8,
                   help="bits of one code: 8 (csrc/ivf_pq.hip) or 4 (csrc/ivf_pq4.hip)")
    p.add_argument("--n-probes", type=int, default=32)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--refine-ratio", type=int, nargs="*", default=[1, 2, 4])
    p.add_argument("--refine-reps", type=int, default=200,
                   help="calls in one timed window of refine alone (a call is short)")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd.neighbors import (BruteForceIndex, IvfFlatParams, IvfPqParams,
                                    ivf_flat_build, ivf_flat_search, ivf_pq_build,
                                    ivf_pq_search, refine)
    from raft_amd.random import RngState, make_blobs

    n, d, nq, k, n_probes = args.rows, args.dim, args.queries, args.k, args.n_probes

    def sync_time(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    allx, _, _ = make_blobs(n + nq, d, n_clusters=1024, state=RngState(seed=7), device=dev)
    allx = allx[torch.randperm(n + nq, device=dev,
                               generator=torch.Generator(dev).manual_seed(1))]
    x, q = allx[:n].contiguous(), allx[n:].contiguous()
    del allx

    warm = x[:max(args.n_lists * 8, n // 16)]
    ivf_flat_build(warm, IvfFlatParams(n_lists=args.n_lists))
    flat_s, flat = sync_time(lambda: ivf_flat_build(x, IvfFlatParams(n_lists=args.n_lists)))
    pq_params = IvfPqParams(n_lists=args.n_lists, pq_dim=args.pq_dim, pq_bits=args.pq_bits)
    ivf_pq_build(warm, pq_params)
    pq_s, pq = sync_time(lambda: ivf_pq_build(x, pq_params))
    print(f"# built: flat {flat_s:.2f} s, pq {pq_s:.2f} s (pq_dim {pq.pq_dim}, pq_bits {pq.pq_bits})",
          file=sys.stderr, flush=True)

    calls = {"ivf_pq": lambda: ivf_pq_search(pq, q, k, n_probes),
             "ivf_flat": lambda: ivf_flat_search(flat, q, k, n_probes)}
    alone, same_ids = {}, {}
    for r in args.refine_ratio:
        calls[f"ivf_pq_refine_x{r}"] = lambda r=r: ivf_pq_search(pq, q, k, n_probes, dataset=x,
                                                                 refine_ratio=r)
        cand = ivf_pq_search(pq, q, k * r, n_probes)[1]
        for engine in ("kernel", "torch"):
            alone[f"refine_{engine}_x{r}"] = lambda c=cand, e=engine: refine(x, q, c, k,
                                                                            engine=e)
        a, b = alone[f"refine_kernel_x{r}"](), alone[f"refine_torch_x{r}"]()
        # the engines add in different orders: near ties may swap
        same_ids[r] = round(float((a[1] == b[1]).float().mean()), 6)
    bf_ids = BruteForceIndex(x).search(q, k)[1]
    out = {"metric": "IVF-PQ vs IVF-Flat, queries per second", "data": "blobs", "rows": n,
           "dim": d, "queries": nq, "n_lists": args.n_lists, "n_probes": n_probes, "k": k,
           "reps": args.reps, "refine_reps": args.refine_reps, "rounds": args.rounds,
           "ivf_pq": {"build_s": round(pq_s, 3), "pq_dim": pq.pq_dim, "pq_len": pq.pq_len,
                      "pq_bits": pq.pq_bits, "bytes_per_row": pq.row_bytes},
           "ivf_flat": {"build_s": round(flat_s, 3), "bytes_per_row": 4 * flat.d_pad}}
    for r in args.refine_ratio:
        out[f"ivf_pq_refine_x{r}"] = {"n_cand": k * r, "engines_same_ids": same_ids[r]}
    times = {name: [] for name in list(calls) + list(alone)}
    for name, f in calls.items():
        ids = f()[1]                                          # warm this shape
        hit = 0
        for s in range(0, nq, 1024):
            hit += int((ids[s:s + 1024, :, None] == bf_ids[s:s + 1024, None, :])
                       .any(dim=2).sum())
        out[name]["recall"] = round(hit / (nq * k), 4)
    calls.update(alone)                                       # warmed above
    for _ in range(args.rounds):
        for name, f in calls.items():                         # alternate
            reps = args.refine_reps if name in alone else args.reps
            t, _ = sync_time(lambda: [f() for _ in range(reps)])
            times[name].append(t / reps)
    for name, ts in times.items():
        out.setdefault(name, {}).update(
            qps_median=round(nq / statistics.median(ts)), qps_min=round(nq / max(ts)),
            qps_max=round(nq / min(ts)), ms_median=round(1e3 * statistics.median(ts), 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
