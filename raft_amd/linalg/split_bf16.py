"""Split-bf16 operands: the one recipe behind every fp32-on-MFMA op.

CDNA4 has no fp32-input MFMA, so the GEMM-shaped fp32 ops (pairwise L2, fused
L2-NN, k-means, kNN filter, eps-neighborhood, masked L2-NN) run their dot term
on bf16 matrix cores: the feature dimension is zero-padded to the MFMA K
granularity, every row is split into 1, 2 or 3 bf16 slices with
x ≈ sum(slices), and the squared row norms ride along in fp32. How many slices
a mode name means, and the provable error envelope of that slice count, are
tabulated here once; what "auto" means stays each op's own decision.
"""
from __future__ import annotations

import torch

from raft_amd._ext import require_ext

#: slices per fp32 mode name ("auto" is resolved by each op before the lookup)
MODE_NSLICE = {"bf16x1v": 1, "bf16x2": 2, "bf16x2v": 2, "bf16x3": 3,
               "fused": 3, "mfma": 3}
#: modes that run an exact-fp32 verification/repair pass: rows (or pairs)
#: inside the split-error margin are re-decided in fp32
VERIFY_MODES = {"bf16x2v", "bf16x1v", "auto"}
#: provable |Δdot| <= lead*sqrt(xn*yn) + tail*(xn+yn) envelope of the split
#: emulation, as (lead, tail) per slice count (derivation: csrc/kmeans.hip
#: l2nn_verify_repair_kernel). One slice does a single MFMA product (1/3 the
#: matrix work of two) against a 2^6-wider bound; verified results are the
#: same, only the rescan fraction grows on data with near-tied neighbors.
SPLIT_BOUND = {1: (2.0 ** -7, 2.0 ** -12),
               2: (2.0 ** -13, 2.0 ** -18),
               3: (2.0 ** -21, 2.0 ** -24)}


def split_bf16_slices(t: torch.Tensor, nslice: int):
    """fp32 -> bf16 slices with t ≈ sum(slices). Iteration-invariant for the
    k-means X matrix, so callers may precompute (see kmeans_iterate)."""
    slices = []
    resid = t
    for i in range(nslice):
        s = resid.to(torch.bfloat16)
        slices.append(s.contiguous())
        if i + 1 < nslice:
            resid = resid - s.to(torch.float32)
    return slices


def pad_features(t: torch.Tensor, mult: int = 64) -> torch.Tensor:
    """Zero-pad the last dimension to a multiple of mult (the MFMA K
    granularity). Zero feature columns change no distance, dot product or
    norm. Returns t itself when no pad is needed."""
    dp = (-t.shape[-1]) % mult
    return torch.nn.functional.pad(t, (0, dp)) if dp else t


def row_sqnorms(t: torch.Tensor) -> torch.Tensor:
    """Squared L2 norm of every row, in fp32 (one native pass on the GPU)."""
    if t.is_cuda and t.dtype == torch.bfloat16:
        # native kernel: a torch float() chain would materialize a 2x-size
        # fp32 copy (51 GB for the 100M-row index — allocation-bound)
        return require_ext().rows_sqnorm_bf16(t.contiguous())
    if t.is_cuda and t.dtype == torch.float32:
        return require_ext().reduce_rows(t.contiguous(), 1)
    return t.float().pow(2).sum(dim=1).contiguous()
