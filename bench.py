#!/usr/bin/env python3
"""Flagship benchmark: k-means fit (BASELINE config 3) on 1..8 MI355X.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 the
driver launches via torch.distributed.run with one rank per GPU over RCCL.
Rank 0 prints ONE JSON line with the whole-job metric.

Workload: kmeans::fit on synthetic make_blobs data, 10M x 256 fp32, k=1024 —
the BASELINE.json config. Strong scaling: the 10M rows are sharded across
ranks; metric = Lloyd iterations/sec of the WHOLE job (one iteration = full
assignment of all 10M rows + centroid update + allreduce).

fp32 on CDNA4 has no MFMA; the default engine is bf16x2v — split-bf16
emulation on the 2.5 PF bf16 matrix cores with the in-kernel second-best
margin + exact-fp32 rescan that makes the argmin provably fp32-exact
(tests/test_gpu_kernels.py). --fp32-mode native uses rocBLAS SGEMM (157 TF
vector ALU) for comparison.

A plain run does only what the headline figure needs: set up, warm up, time
the steps, optionally --dump-outputs, print the JSON line. --full adds the
secondary measurements: the pairwise-L2 Gdist/s figure (skip it with
--no-pairwise) and, with --check, the assignment agreement vs the native
engine over ALL local rows.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--rows", type=int, default=10_000_000, help="total rows (global)")
    p.add_argument("--dim", type=int, default=256)
    p.add_argument("--k", type=int, default=1024)
    p.add_argument("--fp32-mode", default="auto",
                   choices=["auto", "bf16x2v", "bf16x1v", "bf16x3", "bf16x2",
                            "native"],
                   help="fp32 GEMM engine for the assignment step; auto = "
                        "adaptive verified engine (starts 1-product bf16x1v, "
                        "widens to bf16x2v if >2%% of rows hit the exact "
                        "rescan) — exact fp32 argmin either way")
    p.add_argument("--chunk-rows", type=int, default=262144)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (pairwise-L2 "
                        "Gdist/s; --check) after the timed steps")
    p.add_argument("--check", action="store_true",
                   help="with --full: cross-check the final assignment vs "
                        "the native-fp32 engine")
    p.add_argument("--no-pairwise", action="store_true",
                   help="with --full: skip the secondary pairwise-L2 Gdist/s "
                        "measurement")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step returned (centroids, inertia) as DIR/<name>.npy")
    args = p.parse_args()
    if args.check and not args.full:
        p.error("--check is part of the extended run: pass --full --check")
    return args


def dump_outputs(out_dir, centroids, inertia):
    """Write the timed path's return values — the final centroids [k, dim]
    (fp32) and the last step's inertia (scalar, fp64) — as .npy files."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "centroids.npy"),
            centroids.detach().to("cpu", torch.float32).numpy())
    np.save(os.path.join(out_dir, "inertia.npy"),
            np.asarray(inertia, dtype=np.float64))


def measure_pairwise_gdist(dev) -> float:
    """BASELINE config 2 (the other half of the headline metric): pairwise
    L2-expanded 1M x 128 fp32, the FULL 1e12 distances computed in output
    tiles with the fused MFMA tile kernel (epilogue fused, each tile written
    once). Returns Gdist/s."""
    from raft_amd.random import make_blobs, RngState
    from raft_amd._ext import require_ext
    from raft_amd.linalg.gemm import _split_bf16

    ext = require_ext()
    n, d = 1_000_000, 128
    x, _, _ = make_blobs(n, d, n_clusters=1000, cluster_std=1.0,
                         state=RngState(seed=1), device=dev)
    x = x.contiguous()
    xn = (x * x).sum(dim=1)
    slices = _split_bf16(x, 2)
    tq, ti = 50000, 100000
    out = torch.empty((tq, ti), dtype=torch.float32, device=dev)

    def tile(q0, i0):
        sq = [s[q0:q0 + tq] for s in slices]
        si = [s[i0:i0 + ti] for s in slices]
        ext.pairwise_l2_mfma(sq, si, xn[q0:q0 + tq].contiguous(),
                             xn[i0:i0 + ti].contiguous(), out)

    tile(0, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for q0 in range(0, n, tq):
        for i0 in range(0, n, ti):
            tile(q0, i0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out, slices, x, xn
    return n * float(n) / dt / 1e9


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    use_gpu = torch.cuda.is_available()
    if use_gpu:
        torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
        device = torch.device("cuda")
    else:
        device = torch.device("cpu")

    from raft_amd.comms import init_comms as comms_init
    from raft_amd.comms import LoopbackComms
    from raft_amd.cluster.kmeans import kmeans_iterate, kmeans_iter_state
    from raft_amd.random import make_blobs, RngState
    from raft_amd.neighbors.fused_l2nn import fused_l2nn

    if world > 1:
        comms = comms_init()
    else:
        comms = LoopbackComms()

    # ---- synthetic data: this rank's shard of the global 10M x 256 ----------
    rows_local = args.rows // world + (1 if rank < args.rows % world else 0)
    state = RngState(seed=args.seed + rank)  # independent shards, same blob centers
    centers_state = RngState(seed=args.seed)
    from raft_amd.random.rng import uniform
    true_centers = uniform((args.k, args.dim), -10.0, 10.0, state=centers_state,
                           device=device)
    x, _, _ = make_blobs(rows_local, args.dim, n_clusters=args.k, cluster_std=1.0,
                         centers=true_centers, state=state, device=device)
    x = x.contiguous()

    # ---- init centroids: rank 0's first k rows of blob centers + jitter -----
    centroids = true_centers.clone()
    jit = RngState(seed=args.seed + 777)
    centroids += uniform((args.k, args.dim), -0.5, 0.5, state=jit, device=device)
    if world > 1:
        comms.bcast(centroids, root=0)

    def sync():
        if world > 1:
            comms.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    # ---- warmup (the X bf16-slices/norms are once-per-fit preprocessing,
    # computed here like the reference precomputes row norms) ---------------
    iter_state = kmeans_iter_state(x, args.fp32_mode)
    c = centroids.clone()
    c, _ = kmeans_iterate(x, c, max(args.warmup, 0), comms=comms,
                          fp32_mode=args.fp32_mode, chunk_rows=args.chunk_rows,
                          state=iter_state)
    sync()

    # ---- timed: EXACTLY args.steps iterations -------------------------------
    t0 = time.perf_counter()
    c, inertia = kmeans_iterate(x, c, args.steps, comms=comms,
                                fp32_mode=args.fp32_mode, chunk_rows=args.chunk_rows,
                                state=iter_state)
    sync()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    if world > 1:
        # MAX over ranks via the comms_t layer (device follows the backend:
        # RCCL needs a device tensor, gloo a host tensor)
        from raft_amd.comms import ReduceOp
        t_dev = device if torch.distributed.get_backend() == "nccl" \
            else torch.device("cpu")
        t = torch.tensor([elapsed], dtype=torch.float64, device=t_dev)
        comms.allreduce(t, op=ReduceOp.MAX)
        elapsed = float(t.item())

    iters_per_sec = args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    result = {
        "metric": f"kmeans-fit iters/sec ({args.rows} x {args.dim} fp32, k={args.k})",
        "value": round(iters_per_sec, 6),
        "unit": "iters/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic make_blobs (random-init centers, generated on-device)",
        "config": {
            "model": "kmeans-lloyd",
            "global_batch": args.rows,
            "seq_len": args.dim,
            "n_clusters": args.k,
            "parallelism": f"dp{world}",
            "fp32_engine": args.fp32_mode,
            "inertia": inertia,
        },
    }

    if args.dump_outputs and rank == 0:
        # centroids/inertia are already allreduced: identical on every rank
        dump_outputs(args.dump_outputs, c, inertia)

    if args.full and args.check and use_gpu:
        # assignment agreement between emulated and native fp32 engines
        d_emul, a_emul = fused_l2nn(x, c, fp32_mode=args.fp32_mode)
        d_nat, a_nat = fused_l2nn(x, c, fp32_mode="native")
        agree = float((a_emul == a_nat).float().mean().item())
        result["config"]["assign_agreement_vs_native_fp32"] = agree

    if args.full and use_gpu and rank == 0 and not args.no_pairwise:
        # secondary metric: the pairwise half of BASELINE's
        # headline, measured in the same process as the flagship
        try:
            gd = measure_pairwise_gdist(device)
            result["config"]["pairwise_l2_1Mx128_fp32_gdist_per_s"] = round(gd, 1)
        except Exception as e:  # never fail the primary metric
            result["config"]["pairwise_l2_1Mx128_fp32_gdist_per_s"] = f"error: {e}"

    if rank == 0:
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
