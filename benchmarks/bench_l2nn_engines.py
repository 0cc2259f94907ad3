#!/usr/bin/env python3
"""A/B of named fused L2-NN engines on the k-means assignment shape, and of
the fused update/verify kernel that follows it in a k-means step.

Data is the flagship's (bench.py): make_blobs rows around k uniform centers,
centroids = centers + jitter, one bf16 slice. Each --variants entry is
ENGINE:GT (csrc/l2nn_engine.h names; GT 0 = the engine's default) and is run
through ext.fused_l2nn_split(engine=, gt=). --update-verify adds
ext.kmeans_update_verify on the same rows (labels from the first variant,
sorted as the k-means step sorts them).

Rates come from the shapes, not from counters:
  MFMA FLOP   = 2 * rows * k * dim
  least bytes = X and C once in bf16, xn and cn, the three outputs
  update/verify least bytes = X once in fp32 + 6 per-row words + sums
and are printed against the time per call.

Method: every variant is warmed at the timed shape; each timed window is
synchronised on both sides and holds enough calls to last >= --window seconds;
the variants alternate inside one process for --repeats rounds; the median and
the min..max spread over the rounds are printed as one JSON line. The outputs
of every variant are compared with the first one's (torch.equal).
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
    p.add_argument("--variants", type=str, default="2d:8,2d_xreg:8,2d_xring:8")
    p.add_argument("--update-verify", action="store_true")
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

    variants, resolved, outs = {}, {}, {}
    for spec in args.variants.split(","):
        engine, _, gt = spec.partition(":")
        gt = int(gt or 0)
        resolved[spec] = list(ext.l2nn_resolve_engine(1, m, k, d, engine=engine, gt=gt))

        def run(engine=engine, gt=gt, spec=spec):
            outs[spec] = ext.fused_l2nn_split([xs], [cs], xn, cn, engine=engine, gt=gt)
        variants[spec] = run

    flop = 2.0 * m * k * d
    l2nn_bytes = 2.0 * (m + k) * d + 4.0 * (m + k) + 12.0 * m
    uv_bytes = 4.0 * m * d + 24.0 * m + 4.0 * k * d

    if args.update_verify:
        first = next(iter(variants))
        variants[first]()
        dmin0, amin0, dmin2 = outs[first]
        keys_sorted, perm = torch.sort(amin0)
        perm = perm.to(torch.int32)
        lead, tail = SPLIT_BOUND[1]
        packed = torch.empty(k * d + k + 1, dtype=torch.float32, device=dev)
        dmin_w, amin_w = dmin0.clone(), amin0.clone()

        def run_uv():
            # the kernel repairs dmin / amin in place: start every call from
            # the assignment's own outputs
            dmin_w.copy_(dmin0)
            amin_w.copy_(amin0)
            packed.zero_()
            ext.kmeans_update_verify(x, perm, keys_sorted, c, xn, dmin_w, amin_w, dmin2,
                                     cn_max, packed[: k * d].view(k, d),
                                     packed[k * d: k * d + k], packed[-1:],
                                     lead=lead, tail=tail)

        def run_uv_reset():
            dmin_w.copy_(dmin0)
            amin_w.copy_(amin0)
            packed.zero_()
        variants["update_verify"] = run_uv
        variants["update_verify_reset_only"] = run_uv_reset

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

    ref = next(iter(outs))
    same = {spec: all(torch.equal(a, b) for a, b in zip(outs[spec], outs[ref]))
            for spec in outs}
    seconds, rates = {}, {}
    for name, v in times.items():
        med = statistics.median(v)
        seconds[name] = {"median": round(med, 6), "min": round(min(v), 6),
                         "max": round(max(v), 6)}
        if name in resolved:
            rates[name] = {"mfma_tflops": round(flop / med / 1e12, 1),
                           "least_bytes_tb_per_s": round(l2nn_bytes / med / 1e12, 3)}
    if args.update_verify:
        net = (statistics.median(times["update_verify"])
               - statistics.median(times["update_verify_reset_only"]))
        rates["update_verify"] = {"seconds_net_of_reset": round(net, 6),
                                  "least_bytes_tb_per_s": round(uv_bytes / net / 1e12, 3)}
    out = {
        "metric": "fused L2-NN seconds per call (1 bf16 slice)",
        "rows": m, "dim": d, "k": k, "resolved": resolved,
        "mfma_flop": flop, "l2nn_least_bytes": l2nn_bytes,
        "update_verify_least_bytes": uv_bytes if args.update_verify else None,
        "outputs_equal_first_variant": same,
        "calls_per_window": reps, "repeats": args.repeats,
        "seconds": seconds, "rates": rates,
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
