"""Inputs and literal references of the NN-descent tests (CPU and GPU).

Data are cagra_inputs.integer_rows: every value is exact in bf16, fp16 and fp32,
so "equal" is torch.equal on ids and values.
"""
import torch

from raft_amd.neighbors import knn
from raft_amd.neighbors.nn_descent import (init_lists, local_join, merge_candidates, row_sqnorms,
                                           sample_lists)


def torch_rounds(x, K, S, rounds, metric="sqeuclidean"):
    """The CPU torch path run for `rounds` iterations and sampled once more:
    (lists, NEW, OLD, triples of the next join)."""
    norms = row_sqnorms(x)
    lists = init_lists(x, K, metric)
    for _ in range(rounds):
        new, old = sample_lists(*lists, S)
        lists = merge_candidates(*lists, *local_join(x, norms, new, old, metric))[:3]
    lists = tuple(t.clone() for t in lists)
    new, old = sample_lists(*lists, S)
    return lists, new, old, local_join(x, norms, new, old, metric)


def random_samples(n, m, S, seed):
    """NEW / OLD int32 [m, 2S] of ids in [-1, n): -1 pads, a repeated id, an id in
    both lists, a node without NEW rows and one without OLD rows."""
    g = torch.Generator().manual_seed(seed)
    new = torch.randint(-1, n, (m, 2 * S), generator=g).int()
    old = torch.randint(-1, n, (m, 2 * S), generator=g).int()
    new[:, 1], old[:, 0] = new[:, 0], new[:, 0]
    new[3], old[5] = -1, -1
    return new, old


def join_reference(x, new_ids, old_ids, metric):
    """local_join written from its definition in fp64: plain loops."""
    x = x.double()
    ip = metric == "inner_product"
    m, S2 = new_ids.shape
    tgt = torch.full((m, 3 * S2), -1, dtype=torch.int32)
    cid, val = tgt.clone(), torch.full((m, 3 * S2), float("inf"), dtype=torch.float32)
    for c in range(m):
        new, old = new_ids[c].tolist(), old_ids[c].tolist()
        for part, (us, vs) in enumerate([(new, new), (new, old), (old, new)]):
            for p, u in enumerate(us):
                seen = [(float(-(x[u] @ x[v]) if ip
                               else (x[u] @ x[u] + x[v] @ x[v]) - 2 * (x[u] @ x[v])), v)
                        for v in vs if u >= 0 and v >= 0 and v != u]
                if seen:
                    j = part * S2 + p
                    tgt[c, j], (val[c, j], cid[c, j]) = u, min(seen)
    return tgt, cid, val


def merge_reference(vals, ids, flags, tgt, cid, val):
    """merge_candidates written from its definition: per target a dict and a sort."""
    n, K = ids.shape
    vals, ids, flags = vals.clone(), ids.clone(), flags.clone()
    offers = [dict() for _ in range(n)]
    for u, c, v in zip(tgt.reshape(-1).tolist(), cid.reshape(-1).tolist(), val.reshape(-1).tolist()):
        if u >= 0 and c >= 0 and c != u:
            offers[u][c] = min(v, offers[u].get(c, float("inf")))
    for u in range(n):
        row = {i: (v, i, f) for v, i, f in zip(vals[u].tolist(), ids[u].tolist(), flags[u].tolist())
               if i >= 0}
        for c, v in offers[u].items():
            row.setdefault(c, (v, c, True))
        row = (sorted(row.values()) + [(float("inf"), -1, False)] * K)[:K]
        vals[u], ids[u], flags[u] = (torch.tensor(col) for col in zip(*row))
    return vals, ids, flags


def check_invariants(dists, ids, k, descending=False):
    """k distinct ids != the row, best first."""
    n = ids.shape[0]
    assert (dists.dtype, ids.dtype) == (torch.float32, torch.int64)
    assert bool(((ids >= 0) & (ids < n) & (ids != torch.arange(n).unsqueeze(1))).all())
    assert bool((ids.sort(dim=1).values.diff(dim=1) > 0).all())
    assert bool(((-dists if descending else dists).diff(dim=1) >= 0).all())


def recall(ids, x, k):
    """Against exact knn, the row itself left out of both."""
    exact = knn(x.float(), x.float(), k + 1)[1][:, 1:]
    return float((ids[:, :, None] == exact[:, None, :]).any(dim=2).float().mean())
