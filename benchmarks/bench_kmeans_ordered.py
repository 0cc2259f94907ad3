#!/usr/bin/env python3
"""A/B of the two ways a verified k-means step orders its rows and updates:

  sorted   torch.sort(labels) + cast of the indices to int32 + torch.zeros +
           ext.kmeans_update_verify (gathers xn / dmin / dmin2 per row, stores
           dmin per row)
  ordered  ext.kmeans_order_rows + ext.kmeans_update_verify_ordered, with and
           without the write-back of dmin / amin

on the flagship's data (bench.py: make_blobs rows around k uniform centers,
centroids = centers + jitter) with labels from the 1-slice assignment engine.
Each stage is timed alone and the two paths are timed whole, as the k-means
loop runs them. Stages that repair dmin / amin in place start every call from
the assignment's outputs; that reset is timed alone so it can be taken off.

Method (as bench_l2nn_engines.py): every stage is warmed at the timed shape;
each timed window is synchronised on both sides and holds enough calls to last
>= --window seconds; the stages alternate inside one process for --repeats
rounds; median and min..max over the rounds go out as one JSON line. The
ordered outputs are compared with the sorted ones first (order, offsets, flag,
dmin, amin, counts exactly; sums and inertia to fp32 atomic-order noise).
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
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dim", type=int, default=256)
    p.add_argument("--k", type=int, default=1024)
    p.add_argument("--window", type=float, default=1.0)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--seed", type=int, default=42)
    args = p.parse_args()

    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda")
    from raft_amd._ext import require_ext
    from raft_amd.linalg.split_bf16 import SPLIT_BOUND
    from raft_amd.random import RngState, make_blobs
    from raft_amd.random.rng import uniform

    ext = require_ext()
    m, d, k = args.rows, args.dim, args.k
    centers = uniform((k, d), -10.0, 10.0, state=RngState(seed=args.seed), device=dev)
    x, _, _ = make_blobs(m, d, n_clusters=k, cluster_std=1.0, centers=centers,
                         state=RngState(seed=args.seed), device=dev)
    x = x.contiguous()
    c = centers + uniform((k, d), -0.5, 0.5, state=RngState(seed=args.seed + 777),
                          device=dev)
    xs = torch.empty((m, d), dtype=torch.bfloat16, device=dev)
    cs = torch.empty((k, d), dtype=torch.bfloat16, device=dev)
    xn = torch.empty(m, dtype=torch.float32, device=dev)
    cn = torch.empty(k, dtype=torch.float32, device=dev)
    cn_max = torch.zeros(1, dtype=torch.float32, device=dev)
    ext.split_bf16_norms(x, [xs], xn)
    ext.split_bf16_norms(c, [cs], cn, cn_max)
    dmin0, amin0, dmin2 = ext.fused_l2nn_split([xs], [cs], xn, cn)
    del xs
    lead, tail = SPLIT_BOUND[1]

    i32 = dict(dtype=torch.int32, device=dev)
    packed = torch.empty(k * d + k + 1, dtype=torch.float32, device=dev)
    sums, counts, inertia = packed[: k * d].view(k, d), packed[k * d: k * d + k], packed[-1:]
    dmin_w, amin_w = dmin0.clone(), amin0.clone()
    order, offsets = torch.empty(m, **i32), torch.empty(k + 1, **i32)
    table = torch.empty(ext.kmeans_order_rows_workspace(m, k), **i32)
    keys_sorted, perm = torch.sort(amin0, stable=True)
    perm32 = perm.to(torch.int32)

    def reset_all():
        dmin_w.copy_(dmin0)
        amin_w.copy_(amin0)
        packed.zero_()

    def sort_cast():
        ks, pm = torch.sort(amin0)
        return ks, pm.to(torch.int32)

    def update_sorted(ks=keys_sorted, pm=perm32, sm=sums, ct=counts, ia=inertia,
                      dm=dmin_w, am=amin_w):
        ext.kmeans_update_verify(x, pm, ks, c, xn, dm, am, dmin2, cn_max, sm, ct, ia,
                                 lead=lead, tail=tail)

    def order_rows():
        ext.kmeans_order_rows(amin0, dmin0, dmin2, xn, cn_max, lead, tail, k, offsets,
                              order, table)

    def update_ordered(write_back):
        ext.kmeans_update_verify_ordered(x, order, offsets, c, dmin_w, amin_w, sums,
                                         counts, inertia, write_back=write_back)

    # ---- the two paths must agree before anything is timed ------------------
    order_rows()
    reset_all()
    update_sorted()
    ref = dict(dmin=dmin_w.clone(), amin=amin_w.clone(), packed=packed.clone())
    near = (dmin2 - dmin0) < 2.0 * (lead * (xn * cn_max).clamp_min(0).sqrt()
                                    + tail * (xn + cn_max))
    hist = torch.bincount(amin0, minlength=k)
    agree = {
        "order": bool(torch.equal((order & 0x7FFFFFFF).long(), perm)),
        "offsets": bool(torch.equal(offsets[1:].long(), hist.cumsum(0))
                        and int(offsets[0]) == 0),
        "flag_vs_torch_formula_mismatches": int(((order < 0) != near[perm]).sum()),
        "rescan_rows": int((order < 0).sum()),
    }
    for wb in (True, False):
        reset_all()
        update_ordered(wb)
        tag = "wb" if wb else "nowb"
        agree[f"{tag}_counts"] = bool(torch.equal(counts, ref["packed"][k * d: k * d + k]))
        agree[f"{tag}_sums_max_abs_diff"] = float(
            (sums - ref["packed"][: k * d].view(k, d)).abs().max())
        agree[f"{tag}_inertia_rel_diff"] = float(
            ((inertia - ref["packed"][-1:]).abs() / ref["packed"][-1:]).item())
        same = torch.equal(dmin_w, ref["dmin"]) and torch.equal(amin_w, ref["amin"])
        untouched = torch.equal(dmin_w, dmin0) and torch.equal(amin_w, amin0)
        agree[f"{tag}_dmin_amin"] = "equal sorted" if same else (
            "untouched" if untouched else "DIFFERENT")

    def path_sorted():
        # as _FastLoop._local_update ran it: nothing reads dmin / amin after
        ks, pm = torch.sort(amin_w)
        pk = torch.zeros(k * d + k + 1, dtype=torch.float32, device=dev)
        update_sorted(ks, pm.to(torch.int32), pk[: k * d].view(k, d),
                      pk[k * d: k * d + k], pk[-1:])

    def path_sorted_with_reset():
        dmin_w.copy_(dmin0)
        amin_w.copy_(amin0)
        path_sorted()

    def path_ordered():
        packed.zero_()
        order_rows()
        update_ordered(False)

    def reset_dmin_amin():
        dmin_w.copy_(dmin0)
        amin_w.copy_(amin0)

    stages = {
        "sort_cast": sort_cast,
        "order_rows": order_rows,
        "reset_all": reset_all,
        "reset_packed": lambda: packed.zero_(),
        "reset_dmin_amin": reset_dmin_amin,
        "update_sorted+reset_all": lambda: (reset_all(), update_sorted()),
        "update_ordered_wb+reset_all": lambda: (reset_all(), update_ordered(True)),
        "update_ordered_nowb+reset_packed": lambda: (packed.zero_(), update_ordered(False)),
        "path_sorted+reset_dmin_amin": path_sorted_with_reset,
        "path_ordered": path_ordered,
    }

    def timed(f, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    reps = {}
    for name, f in stages.items():
        timed(f, 1)                                  # warm this shape
        reps[name] = max(1, math.ceil(args.window / max(timed(f, 1), 1e-6)))
    times = {name: [] for name in stages}
    for _ in range(args.repeats):
        for name, f in stages.items():               # alternate in one process
            times[name].append(timed(f, reps[name]))

    ms = {name: {"median": round(statistics.median(v) * 1e3, 4),
                 "min": round(min(v) * 1e3, 4), "max": round(max(v) * 1e3, 4)}
          for name, v in times.items()}
    med = {name: statistics.median(v) * 1e3 for name, v in times.items()}
    net = {
        "update_sorted": round(med["update_sorted+reset_all"] - med["reset_all"], 4),
        "update_ordered_wb": round(med["update_ordered_wb+reset_all"] - med["reset_all"], 4),
        "update_ordered_nowb": round(med["update_ordered_nowb+reset_packed"]
                                     - med["reset_packed"], 4),
        "path_sorted": round(med["path_sorted+reset_dmin_amin"] - med["reset_dmin_amin"], 4),
        "path_ordered": round(med["path_ordered"], 4),
    }
    print(json.dumps({
        "metric": "k-means row ordering + update/verify, ms per call",
        "rows": m, "dim": d, "k": k, "agree": agree, "calls_per_window": reps,
        "repeats": args.repeats, "ms": ms, "ms_net_of_resets": net,
    }), flush=True)


if __name__ == "__main__":
    main()
