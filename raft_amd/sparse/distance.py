"""Pairwise distances between the rows of two CSR matrices.

Reference parity: RAFT's historical raft/sparse/distance. Every supported
metric is a sum over features of f(a_c, b_c) with f(0, 0) = 0, so

    sum_c f(a_c, b_c) = sum_c f(a_c, 0) + sum_c f(0, b_c)
                      + sum_{c stored in both} g(a_c, b_c),
    g(a, b) = f(a, b) - f(a, 0) - f(0, b)

The first two terms are per-row statistics (O(nnz), once per matrix); only the
third is pairwise, and it touches only the columns stored in both rows. On GPU
it is ONE kernel (csrc/sparse_pairwise.hip): a block stages four A rows in LDS
(a dense column-window slab or one hash table per row), streams B's CSR past
them and writes the finished distances. Nothing is ever densified on GPU.

Input contract: column ids within a row need not be sorted but must be unique
(run dedupe_coo first if unsure); duplicates give an unspecified finite
result. Stored explicit zeros are allowed and change nothing.
"""
from __future__ import annotations

import torch

from raft_amd._ext import require_ext
from raft_amd.distance.pairwise import DistanceType, _metric_from_str, pairwise_distance
from .types import CSR

# metric codes of ext.csr_row_stats / ext.csr_pairwise
# (SparseDistanceCode in include/raft_amd/sparse.hpp)
_SPARSE_CODES = {
    DistanceType.InnerProduct: 0,
    DistanceType.L2Expanded: 1, DistanceType.L2Unexpanded: 1,
    DistanceType.L2SqrtExpanded: 2, DistanceType.L2SqrtUnexpanded: 2,
    DistanceType.CosineExpanded: 3,
    DistanceType.CorrelationExpanded: 4,
    DistanceType.L1: 5,
    DistanceType.LpUnexpanded: 6,
    DistanceType.Canberra: 7,
    DistanceType.HammingUnexpanded: 8,
    DistanceType.JensenShannon: 9,
    DistanceType.HellingerExpanded: 10,
    DistanceType.JaccardExpanded: 11,
    DistanceType.DiceExpanded: 12,
    DistanceType.RusselRaoExpanded: 13,
}
_UNSUPPORTED = {
    DistanceType.Linf: "a maximum over features, not a sum",
    DistanceType.KLDivergence: "its A-only terms cancel catastrophically in fp32",
    DistanceType.BrayCurtis: "it needs two intersection sums",
    DistanceType.Haversine: "it is defined for d == 2 only",
}
# metrics whose CPU evaluation broadcasts [chunk, n, d]
_BROADCAST = {DistanceType.L1, DistanceType.LpUnexpanded, DistanceType.Canberra,
              DistanceType.HammingUnexpanded, DistanceType.JensenShannon,
              DistanceType.RusselRaoExpanded}

_STRATEGIES = {"auto": 0, "dense": 1, "hash": 2}
# limits of the two LDS staging strategies (include/raft_amd/sparse.hpp)
DENSE_WINDOW_MAX = 8192
DENSE_AUTO_MAX = 4096  # "auto": a 64 KiB slab still lets two blocks share a CU
HASH_CAPACITY_MIN = 64
HASH_CAPACITY_MAX = 4096
_CPU_BROADCAST_BYTES = 256 << 20


def _resolve_metric(metric) -> DistanceType:
    if isinstance(metric, str):
        metric = _metric_from_str(metric)
    if metric in _UNSUPPORTED:
        raise ValueError(f"sparse distance does not support {metric.name} "
                         f"({metric.value}): {_UNSUPPORTED[metric]}")
    if metric not in _SPARSE_CODES:
        raise ValueError(f"unknown metric {metric!r}")
    return metric


def _is_pow2(v: int) -> bool:
    return v > 0 and (v & (v - 1)) == 0


def _resolve_strategy(strategy, hash_capacity, dense_window, d: int):
    """(strategy code, kernel parameter) after validating the overrides."""
    if strategy not in _STRATEGIES:
        raise ValueError(f"unknown strategy {strategy!r}; expected one of "
                         f"{sorted(_STRATEGIES)}")
    if hash_capacity is not None:
        hash_capacity = int(hash_capacity)
        if (not _is_pow2(hash_capacity)
                or not HASH_CAPACITY_MIN <= hash_capacity <= HASH_CAPACITY_MAX):
            raise ValueError(
                f"hash_capacity must be a power of two in [{HASH_CAPACITY_MIN}, "
                f"{HASH_CAPACITY_MAX}], got {hash_capacity}")
    if dense_window is not None:
        dense_window = int(dense_window)
        if not _is_pow2(dense_window) or dense_window > DENSE_WINDOW_MAX:
            raise ValueError(f"dense_window must be a power of two <= "
                             f"{DENSE_WINDOW_MAX}, got {dense_window}")
    code = _STRATEGIES[strategy]
    if code == 0:
        # one window over all of d while the slab stays small enough for two
        # blocks per CU (measured cross-over, docs/performance.md)
        code = 1 if d <= DENSE_AUTO_MAX else 2
    param = dense_window if code == 1 else hash_capacity
    return code, int(param or 0)


def _densify_rows(a: CSR, start: int, stop: int, dtype) -> torch.Tensor:
    """Rows [start, stop) of a CPU CSR matrix as a dense [stop - start, d] block."""
    indptr = a.indptr.to(torch.int64)
    lo, hi = int(indptr[start]), int(indptr[stop])
    lengths = indptr[start + 1:stop + 1] - indptr[start:stop]
    rows = torch.repeat_interleave(torch.arange(stop - start), lengths)
    out = torch.zeros((stop - start, a.n_cols), dtype=dtype)
    out[rows, a.indices[lo:hi].to(torch.int64)] = a.values[lo:hi].to(dtype)
    return out


def _pairwise_cpu(a: CSR, b: CSR, metric: DistanceType, p: float) -> torch.Tensor:
    """Oracle path: densify in row chunks, dense fp64 pairwise_distance."""
    m, n, d = a.n_rows, b.n_rows, a.n_cols
    out = torch.empty((m, n), dtype=a.dtype)
    if m == 0 or n == 0:
        return out
    bd = _densify_rows(b, 0, n, torch.float64)
    per_row = n * d * 8 if metric in _BROADCAST else d * 8
    chunk = max(1, min(m, _CPU_BROADCAST_BYTES // max(per_row, 1)))
    for s in range(0, m, chunk):
        e = min(s + chunk, m)
        ad = _densify_rows(a, s, e, torch.float64)
        out[s:e] = pairwise_distance(ad, bd, metric, p=p).to(a.dtype)
    return out


def _gpu_csr(a: CSR):
    """(indptr int32, indices int32, values fp32), contiguous, for the kernels."""
    if a.dtype == torch.float64:
        raise TypeError("sparse_pairwise_distance has no fp64 GPU kernel; pass "
                        "fp32 / bf16 / fp16 values or move the matrices to the CPU")
    if a.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"unsupported value dtype {a.dtype}")
    if a.nnz >= 2 ** 31 or a.n_cols >= 2 ** 31:
        raise ValueError("sparse_pairwise_distance needs nnz < 2^31 and d < 2^31")
    return (a.indptr.to(torch.int32).contiguous(),
            a.indices.to(torch.int32).contiguous(),
            a.values.float().contiguous())  # bf16 / fp16 widen exactly


def sparse_pairwise_distance(a: CSR, b: CSR | None = None,
                             metric: DistanceType | str = DistanceType.L2Expanded,
                             p: float = 2.0, *, strategy: str = "auto",
                             hash_capacity: int | None = None,
                             dense_window: int | None = None) -> torch.Tensor:
    """Distance matrix [m, n] between the rows of CSR a [m, d] and CSR b [n, d].

    b=None is a self-join. Supported metrics: inner product, the four L2
    forms, cosine, correlation, L1, Lp, Canberra, Hamming, Jensen-Shannon,
    Hellinger, Jaccard, Dice and Russel-Rao, with the definitions (clamps and
    zero-denominator rules included) of the dense pairwise_distance. Linf,
    KL divergence, Bray-Curtis and Haversine raise ValueError.

    Column ids within a row need not be sorted but must be unique; duplicates
    give an unspecified finite result.

    GPU: fp32 values run the native kernels and return fp32; bf16 / fp16
    values are widened exactly and return fp32; fp64 values raise. int64
    indptr / indices are narrowed (nnz and d must be below 2^31).
    strategy: "auto" | "dense" | "hash" picks how a block stages its A rows in
    LDS: a dense slab over windows of dense_window columns ("auto" when d <=
    4096), or per-row hash tables of hash_capacity slots (any d; rows longer
    than half the capacity take several chunks). hash_capacity (power of two
    in [64, 4096]) and dense_window (power of two <= 8192) override the
    defaults; results do not depend on them beyond fp32 summation order.

    CPU: the oracle path. Rows are densified in chunks and evaluated by the
    dense pairwise_distance in fp64; the result has the input dtype.
    """
    metric = _resolve_metric(metric)
    self_join = b is None
    if self_join:
        b = a
    if a.n_cols != b.n_cols:
        raise ValueError(f"column counts differ: a has {a.n_cols}, b has {b.n_cols}")
    code, param = _resolve_strategy(strategy, hash_capacity, dense_window, a.n_cols)

    if not (a.values.is_cuda or b.values.is_cuda):
        if a.dtype != b.dtype:
            raise TypeError(f"value dtypes differ: {a.dtype} and {b.dtype}")
        return _pairwise_cpu(a, b, metric, float(p))
    if not (a.values.is_cuda and b.values.is_cuda):
        raise ValueError("a and b must live on the same device")

    ext = require_ext()
    m, n, d = a.n_rows, b.n_rows, a.n_cols
    if d == 0:
        raise ValueError("sparse_pairwise_distance needs at least one column")
    mcode = _SPARSE_CODES[metric]
    a_ptr, a_idx, a_val = _gpu_csr(a)
    a_stats = ext.csr_row_stats(a_ptr, a_idx, a_val, m, mcode, float(p))
    if self_join:
        b_ptr, b_idx, b_val, b_stats = a_ptr, a_idx, a_val, a_stats
    else:
        b_ptr, b_idx, b_val = _gpu_csr(b)
        b_stats = ext.csr_row_stats(b_ptr, b_idx, b_val, n, mcode, float(p))
    return ext.csr_pairwise(a_ptr, a_idx, a_val, m, b_ptr, b_idx, b_val, n,
                            a_stats, b_stats, d, mcode, float(p), code, param)
