"""refine: exact re-rank of kNN candidates against the original vectors.

Reference parity: raft::neighbors::refine (dataset, queries, candidate ids in;
top-k out). An approximate search (ivf_pq_search ranks by the distance to the
RECONSTRUCTED rows) is run with a larger k and its ids are ranked here by the
exact fp32 distance to the rows of the data set.

MI355X design (csrc/refine.hip): one block per query gathers the candidate
rows with sub-waves of 8 to 64 lanes (16-byte loads, several rows in flight
per lane), keeps the query in LDS, packs (distance, id) into 64-bit keys and
sorts them in LDS; neither the gathered rows nor the [q, n_cand] distances
reach memory. The data set is read in its own dtype and with its own row
stride.

CPU tensors run the same algorithm in plain torch (gather, fp32 distances, a
sort by (value, id)), chunked over queries. On a GPU a shape outside
kernel_serves takes that torch path; a GPU call without the native extension
raises.
"""
from __future__ import annotations

import torch

from raft_amd._ext import require_ext
from raft_amd.distance import DistanceType
from raft_amd.utils import row_chunks

from .ivf_flat import _METRIC_CODES, _resolve_metric

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
#: the shapes csrc/refine.hip serves: 32 KiB of query and 32 KiB of keys in LDS
_MAX_KERNEL_D = 8192
_MAX_KERNEL_CAND = 4096
_MIN_KEY_SLOTS = 256
_ENGINES = ("auto", "kernel", "torch")
#: fp32 elements one torch-path chunk gathers
_TORCH_CHUNK_ELEMS = 1 << 24


def key_slots(n_cand: int) -> int:
    """Keys the kernel sorts: n_cand rounded up to a power of two, at least 256."""
    return max(_MIN_KEY_SLOTS, 1 << max(0, int(n_cand) - 1).bit_length())


def kernel_serves(d: int, n_cand: int, k: int) -> bool:
    """Whether csrc/refine.hip serves rows of d features, n_cand candidates per
    query and k results (refine and its tests read this one predicate)."""
    return 1 <= d <= _MAX_KERNEL_D and 1 <= n_cand <= _MAX_KERNEL_CAND and k <= key_slots(n_cand)


def _refine_torch(dataset, q32, candidates, dists, ids, metric):
    n, d = dataset.shape
    q, n_cand = candidates.shape
    k = dists.shape[1]
    if n == 0:
        return
    ip = metric == DistanceType.InnerProduct
    bad = float("-inf") if ip else float("inf")
    top = min(k, n_cand)
    for s0, s1 in row_chunks(q, max(1, _TORCH_CHUNK_ELEMS // (n_cand * max(d, 1)))):
        c = candidates[s0:s1]
        ok = (c >= 0) & (c < n)
        # by id first (invalid last), then a stable sort by value: (value, id)
        c, by_id = torch.where(ok, c, torch.iinfo(torch.int64).max).sort(dim=1, stable=True)
        ok = ok.gather(1, by_id)
        rows = dataset[c.clamp(max=n - 1)].float()                 # [qc, n_cand, d]
        qv = q32[s0:s1].unsqueeze(1)
        val = (rows * qv).sum(dim=2) if ip else ((rows - qv) ** 2).sum(dim=2)
        val = torch.where(val.isnan(), torch.full_like(val, bad), val)
        rank = torch.where(ok, -val if ip else val, torch.full_like(val, float("inf")))
        pick = rank.argsort(dim=1, stable=True)[:, :top]
        ok = ok.gather(1, pick)
        val = val.gather(1, pick)
        if metric == DistanceType.L2SqrtExpanded:
            val = val.sqrt()
        dists[s0:s1, :top] = torch.where(ok, val, torch.full_like(val, bad))
        ids[s0:s1, :top] = torch.where(ok, c.gather(1, pick), torch.full_like(pick, -1))


def refine(dataset: torch.Tensor, queries: torch.Tensor, candidates: torch.Tensor, k: int,
           metric="sqeuclidean", *, engine: str = "auto"):
    """The k best of every query's candidates by EXACT distance to the data set
    rows (reference raft::neighbors::refine).

    dataset [n, d] is fp32, bf16 or fp16 with stride(1) == 1 and any row
    stride (a row- or column-sliced view is read in place, in its own dtype);
    n < 2^32 - 1. queries [q, d] is fp32, bf16 or fp16 and is widened to fp32.
    candidates [q, n_cand] int64 are data set row numbers, typically the ids
    of an approximate search with a larger k; dataset[id] must be the vector
    that search indexed under id. metric is sqeuclidean, euclidean or
    inner_product.

    Returns (dists [q, k] fp32, ids [q, k] int64), best first: smallest
    distance, or largest product for inner_product; equal values are ordered
    by the smaller id (for euclidean the order is that of the squared
    distance), so the result does not depend on the order of a row of
    candidates. Squared L2 is the unexpanded fp32 sum of (x - q)^2, inner
    product the fp32 sum of x * q; euclidean is the square root of the final
    value.

    An id < 0 or >= n is not a candidate (-1 slots of a search pass through).
    A row with fewer than k valid candidates, n_cand < k included, is filled
    with +inf (-inf for inner_product) and id -1. A candidate whose distance is
    NaN keeps its id, gets that bad value and ranks after every number and
    before the missing slots. A REPEATED id is returned repeatedly, as the
    reference does: pass unique candidates for unique results.

    engine: "kernel" is csrc/refine.hip and raises where kernel_serves is
    false or the tensors are on the CPU; "torch" is the plain form (a
    [q chunk, n_cand, d] gather); "auto" is the kernel on a GPU wherever it
    serves. CPU tensors always run the torch path.
    """
    k = int(k)
    if k <= 0:
        raise ValueError(f"k must be positive, got {k}")
    if engine not in _ENGINES:
        raise ValueError(f"engine must be one of {_ENGINES}, got {engine!r}")
    metric = _resolve_metric(metric)
    if dataset.dim() != 2 or dataset.dtype not in _DTYPES:
        raise ValueError("dataset must be an fp32, bf16 or fp16 tensor [n, d]")
    n, d = dataset.shape
    if d > 1 and dataset.stride(1) != 1:
        raise ValueError("dataset must have stride(1) == 1 (any row stride)")
    if n >= 2 ** 32 - 1:
        raise ValueError(f"dataset must have fewer than 2^32 - 1 rows, got {n}")
    if queries.dim() != 2 or queries.shape[1] != d or queries.dtype not in _DTYPES:
        raise ValueError(f"queries must be fp32, bf16 or fp16 [q, {d}], "
                         f"got {tuple(queries.shape)}")
    q = queries.shape[0]
    if candidates.dim() != 2 or candidates.shape[0] != q or candidates.dtype != torch.int64:
        raise ValueError(f"candidates must be int64 [{q}, n_cand]")
    dev = dataset.device
    if queries.device != dev or candidates.device != dev:
        raise ValueError("dataset, queries and candidates must be on one device")
    n_cand = candidates.shape[1]
    gpu = dev.type == "cuda"
    if gpu:
        require_ext()
    serves = gpu and kernel_serves(d, n_cand, k)
    if engine == "kernel" and not serves and q and n_cand:
        raise ValueError(f"engine='kernel' serves GPU tensors with d <= {_MAX_KERNEL_D}, "
                         f"n_cand <= {_MAX_KERNEL_CAND} and k <= {key_slots(n_cand)}; got "
                         f"{dev.type} tensors, d = {d}, n_cand = {n_cand}, k = {k}")

    bad = float("-inf") if metric == DistanceType.InnerProduct else float("inf")
    dists = torch.full((q, k), bad, dtype=torch.float32, device=dev)
    ids = torch.full((q, k), -1, dtype=torch.int64, device=dev)
    if q == 0 or n_cand == 0:
        return dists, ids
    q32 = queries.float().contiguous()
    if serves and engine != "torch":
        require_ext().refine_topk(dataset, q32, candidates.contiguous(), dists, ids,
                                  _METRIC_CODES[metric])
    else:
        _refine_torch(dataset, q32, candidates, dists, ids, metric)
    return dists, ids
