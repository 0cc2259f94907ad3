#!/usr/bin/env python3
"""Brute-force bitwise-Hamming kNN over bit-packed rows (csrc/pairwise_bits.hip)
against what a user could do before it: the bits unpacked to 0 / 1 uint8 and
knn with squared L2 on the int8 path (the same numbers, 8x the index bytes,
at most 4096 bits).

Sign bits of clustered embeddings (1024 centres + N(0, 1) noise, packed by
pack_bits on the GPU). Per shape the two paths alternate in one process: both
warmed at shape, then `--windows` windows per path of as many calls as fill
`--window-s` seconds, each window ended by a device synchronise. One JSON line
per (rows, bits) with the median, minimum and maximum window of each path in
queries per second, both index sizes, whether the two paths returned the same
distances, and the share of query rows whose candidate buffer under- or
overflowed and went to the tiled path. A shape above 4096 bits has no baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_knn_int8 import summary, windows  # noqa: E402


def make_bits(rows, bits, centres, gen, dev):
    """uint8 [rows, bits / 8]: sign bits of centre + N(0, 1), in chunks."""
    from raft_amd.distance import pack_bits
    out = torch.empty((rows, bits // 8), dtype=torch.uint8, device=dev)
    step = max(1, (1 << 28) // bits)
    for s in range(0, rows, step):
        e = min(s + step, rows)
        lab = torch.randint(0, centres.shape[0], (e - s,), generator=gen, device=dev)
        out[s:e] = pack_bits(centres[lab] + torch.randn((e - s, bits), generator=gen,
                                                        device=dev))
    return out


def unpack(packed):
    """uint8 [rows, 8 * nbytes] of 0 / 1, little bit order, in chunks."""
    rows, nbytes = packed.shape
    shifts = torch.arange(8, dtype=torch.uint8, device=packed.device)
    out = torch.empty((rows, 8 * nbytes), dtype=torch.uint8, device=packed.device)
    for s in range(0, rows, 1_000_000):
        out[s:s + 1_000_000] = ((packed[s:s + 1_000_000, :, None] >> shifts) & 1).flatten(1)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="1000000x1024,10000000x1024,1000000x8192",
                   help="rows x bits, comma separated")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--queries", type=int, default=10_000)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--window-s", type=float, default=1.0)
    args = p.parse_args()

    assert torch.cuda.is_available(), "bench_knn_bits needs a GPU"
    dev = torch.device("cuda")
    from raft_amd.neighbors.brute_force import BruteForceIndex, _knn_bits

    k, nq = args.k, args.queries
    for rows, bits in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
        gen = torch.Generator(device=dev).manual_seed(11)
        centres = torch.randn((1024, bits), generator=gen, device=dev)
        x, q = make_bits(rows, bits, centres, gen, dev), make_bits(nq, bits, centres, gen, dev)
        index = BruteForceIndex(x, metric="bitwise_hamming")
        stats = {}
        d_bits, _ = _knn_bits(index.x, q, k, None, pre=index._bits, stats=stats)
        line = {"bench": "knn_bits", "rows": rows, "bits": bits, "k": k, "queries": nq,
                "index_bytes": x.numel(), "tiled_share": round(stats["tiled_share"], 5)}
        base = bits <= 4096
        if base:
            index_u8, q_u8 = BruteForceIndex(unpack(x)), unpack(q)
            line["unpacked_index_bytes"] = index_u8.x.numel()
            line["distances_equal"] = bool(torch.equal(d_bits, index_u8.search(q_u8, k)[0]))
        r_bits, r_u8 = [], []
        for _ in range(args.windows):  # the two paths alternate
            a, calls = windows(lambda: index.search(q, k), 1, args.window_s, nq)
            r_bits += a
            line["calls_per_window"] = [calls]
            if base:
                b, calls_u8 = windows(lambda: index_u8.search(q_u8, k), 1, args.window_s, nq)
                r_u8 += b
                line["calls_per_window"].append(calls_u8)
        line["bits_qps"] = summary(r_bits)
        line["bits_gpairs_per_s"] = round(statistics.median(r_bits) * rows / 1e9, 1)
        if base:
            line["unpacked_u8_qps"] = summary(r_u8)
            line["bits_over_unpacked"] = round(statistics.median(r_bits)
                                               / statistics.median(r_u8), 3)
        print(json.dumps(line), flush=True)
        del index, x, q
        if base:
            del index_u8, q_u8


if __name__ == "__main__":
    main()
