#!/usr/bin/env python3
"""A/B + correctness for the 256^2 counted-vmcnt L2-NN engine.

Usage (on the GPU box):
  RAFT_AMD_L2NN_256=1 python benchmarks/ab_l2nn_256.py --mode check
  python benchmarks/ab_l2nn_256.py --mode ab
The env is read once per process, so the ab mode shells out per engine.
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def run_engine(m, n, d, steps):
    from raft_amd._ext import require_ext
    ext = require_ext()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    x = torch.randn(m, d, device=dev)
    c = torch.randn(n, d, device=dev)
    from raft_amd.linalg.split_bf16 import split_bf16_slices
    xs = split_bf16_slices(x, 2)
    cs = split_bf16_slices(c, 2)
    xn = (x * x).sum(dim=1)
    cn = (c * c).sum(dim=1)
    # warmup + timed
    dmin, amin, dmin2 = ext.fused_l2nn_split(xs, cs, xn, cn)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dmin, amin, dmin2 = ext.fused_l2nn_split(xs, cs, xn, cn)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dmin, amin, dmin2, dt


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", default="check", choices=["check", "ab", "one"])
    p.add_argument("--m", type=int, default=1_000_000)
    p.add_argument("--n", type=int, default=1024)
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--out", default="")
    args = p.parse_args()

    if args.mode == "one":
        dmin, amin, dmin2, dt = run_engine(args.m, args.n, args.d, args.steps)
        if args.out:
            torch.save({"dmin": dmin.cpu(), "amin": amin.cpu(),
                        "dmin2": dmin2.cpu()}, args.out)
        print(json.dumps({
            "engine": os.environ.get("RAFT_AMD_L2NN_256", "a"),
            "ms": dt * 1000,
            "dmin_sum": float(dmin.double().sum()),
            "amin_sum": int(amin.to(torch.int64).sum()),
            "dmin2_sum": float(dmin2.double().sum()),
        }), flush=True)
        return

    if args.mode == "check":
        # correctness: 256-engine vs 2d-engine vs torch oracle, incl. ragged m
        for (m, n, d) in [(70000, 512, 64), (100001, 1024, 256),
                          (65536, 256, 128), (299777, 2048, 192)]:
            outs, meta = {}, {}
            for eng in ("1", "0"):
                env = dict(os.environ, RAFT_AMD_L2NN_256=eng)
                path = f"/tmp/l2nn256_{eng}.pt"
                r = subprocess.run(
                    [sys.executable, __file__, "--mode", "one", "--m", str(m),
                     "--n", str(n), "--d", str(d), "--steps", "1",
                     "--out", path],
                    capture_output=True, text=True, env=env, timeout=600)
                assert r.returncode == 0, r.stdout + r.stderr
                outs[eng] = torch.load(path)
                meta[eng] = json.loads(r.stdout.strip().splitlines()[-1])
            a, b = outs["1"], outs["0"]
            # accumulation ORDER differs between engines -> fp32 near-ties may
            # flip; everything else must agree tightly
            dok = torch.allclose(a["dmin"], b["dmin"], rtol=1e-4, atol=1e-3)
            agree = float((a["amin"] == b["amin"]).float().mean())
            difr = (a["amin"] != b["amin"]).nonzero(as_tuple=True)[0]
            tie_ok = bool((a["dmin"][difr] - b["dmin"][difr]).abs().max() < 1e-2) \
                if difr.numel() else True
            d2ok = torch.allclose(a["dmin2"], b["dmin2"], rtol=1e-4, atol=1e-3)
            ok = dok and agree > 0.9999 and tie_ok and d2ok
            print(f"m={m} n={n} d={d}: 256={meta['1']['ms']:.2f}ms "
                  f"2d={meta['0']['ms']:.2f}ms agree={agree:.6f} "
                  f"ok={ok}", flush=True)
            if not ok:
                print(f"  MISMATCH dok={dok} d2ok={d2ok} tie_ok={tie_ok} "
                      f"ndiff={difr.numel()}", flush=True)
        return

    # ab: flagship shape
    for eng in ("0", "1"):
        env = dict(os.environ, RAFT_AMD_L2NN_256=eng)
        r = subprocess.run(
            [sys.executable, __file__, "--mode", "one", "--m", str(args.m),
             "--n", str(args.n), "--d", str(args.d), "--steps", str(args.steps)],
            capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        j = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"engine={'256' if eng == '1' else '2d '}: {j['ms']:.2f} ms "
              f"(dmin_sum {j['dmin_sum']:.6e})", flush=True)


if __name__ == "__main__":
    main()
