"""Brute-force k-nearest-neighbors over CSR matrices.

Reference parity: RAFT's historical raft/sparse/neighbors brute-force kNN:
for every (query batch, index batch) pair compute the sparse pairwise
distance tile, select k per row, and merge with the running best. The full
[q, n] matrix never exists.
"""
from __future__ import annotations

import torch

from raft_amd.distance.pairwise import DistanceType
from raft_amd.matrix.select_k import select_k
from raft_amd.utils import row_chunks
from .distance import _resolve_metric, sparse_pairwise_distance
from .op import slice_csr_rows
from .types import CSR


def sparse_knn(index: CSR, queries: CSR, k: int,
               metric: DistanceType | str = DistanceType.L2Expanded, p: float = 2.0, *,
               batch_size_index: int | None = None,
               batch_size_query: int | None = None, res=None):
    """k nearest rows of CSR index [n, d] for each row of CSR queries [q, d].

    Returns (dists [q, k], idx [q, k] int64), each row sorted best first.
    InnerProduct selects the k largest values, every other metric the k
    smallest. dists are fp32 on GPU and have the input dtype on CPU, as
    sparse_pairwise_distance does. k > n raises ValueError.

    batch_size_index / batch_size_query bound the distance tile; the defaults
    come from the workspace budget of res (or of the default resources of the
    queries' device), as for the dense knn.
    """
    metric = _resolve_metric(metric)
    n, q = index.n_rows, queries.n_rows
    k = int(k)
    if index.n_cols != queries.n_cols:
        raise ValueError(f"column counts differ: index has {index.n_cols}, "
                         f"queries have {queries.n_cols}")
    if k <= 0 or k > n:
        raise ValueError(f"k={k} out of range for an index of {n} rows")
    if batch_size_index is None or batch_size_query is None:
        from raft_amd.core.resources import get_resources
        from raft_amd.neighbors.brute_force import _tiles_from_budget
        r = get_resources(res if res is not None else queries.device)
        qc, ic = _tiles_from_budget(r.workspace_budget(), q, n, index.n_cols, k)
        batch_size_query = batch_size_query or qc
        batch_size_index = batch_size_index or ic
    if batch_size_index <= 0 or batch_size_query <= 0:
        raise ValueError("batch sizes must be positive")
    select_min = metric != DistanceType.InnerProduct

    one_index_batch = batch_size_index >= n
    out_d, out_i = [], []
    for qs, qe in row_chunks(q, batch_size_query):
        qb = queries if (qs, qe) == (0, q) else slice_csr_rows(queries, qs, qe)
        best_d = best_i = None
        for is_, ie in row_chunks(n, batch_size_index):
            ib = index if one_index_batch else slice_csr_rows(index, is_, ie)
            dist = sparse_pairwise_distance(qb, ib, metric, p)
            dd, ii = select_k(dist, min(k, ie - is_), select_min=select_min)
            ii = ii + is_
            if best_d is not None:
                # running best merged with this batch's best: [q_b, <= 2k]
                dcat = torch.cat([best_d, dd], dim=1)
                icat = torch.cat([best_i, ii], dim=1)
                dd, pos = select_k(dcat, min(k, dcat.shape[1]), select_min=select_min)
                ii = torch.gather(icat, 1, pos)
            best_d, best_i = dd, ii
        out_d.append(best_d)
        out_i.append(best_i)
    if not out_d:
        dt = torch.float32 if queries.values.is_cuda else queries.dtype
        return (torch.empty((0, k), dtype=dt, device=queries.device),
                torch.empty((0, k), dtype=torch.int64, device=queries.device))
    return torch.cat(out_d, dim=0), torch.cat(out_i, dim=0)
