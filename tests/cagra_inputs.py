"""Inputs and literal references of the CAGRA tests (CPU and GPU).

Data are integers in [-4, 4]: every distance is exact in fp32 and representable
in bf16 / fp16, ties are plentiful, and "equal" is torch.equal on ids and dists.
"""
import functools

import torch

from raft_amd.neighbors import CagraParams, cagra_build, knn

METRICS = ("sqeuclidean", "euclidean", "inner_product")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def integer_rows(n, d, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (n, d), generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def cpu_index(n, d, g, metric="sqeuclidean", dtype=torch.float32):
    """A CPU-built index over integer rows (shared, never modified) and 70 queries."""
    x = integer_rows(n + 70, d, 100 * n + d, dtype)
    params = CagraParams(graph_degree=g, intermediate_graph_degree=2 * g,
                         build_algo="brute_force", metric=metric)
    return cagra_build(x[:n], params), x[n:]


@functools.lru_cache(maxsize=None)
def knn_graph(n, kd, tails):
    """[n, kd] from CPU knn on integer rows; with `tails` n <= kd and rows end in -1."""
    x = integer_rows(n, 6, n + kd)
    k = min(kd + 1, n)
    ids = knn(x, x, k)[1]
    own = ids == torch.arange(n).unsqueeze(1)
    own[:, k - 1] |= ~own.any(dim=1)
    graph = torch.full((n, kd), -1, dtype=torch.int64)
    graph[:, :k - 1] = ids[~own].reshape(n, k - 1)
    assert tails == bool((graph < 0).any())
    return graph


def optimize_reference(graph, g):
    """cagra_optimize written from its definition: plain loops over lists."""
    graph = graph.tolist()
    n, kd = len(graph), len(graph[0])
    pruned = []
    for a in range(n):
        detour = [0] * kd
        for k_ab in range(kd):
            b = graph[a][k_ab]
            for k_bd in range(kd if 0 <= b < n else 0):
                dn = graph[b][k_bd]
                for k_ad in range(kd if 0 <= dn < n else 0):
                    if graph[a][k_ad] == dn and k_ab < k_ad and k_bd < k_ad:
                        detour[k_ad] += 1
        ranks = sorted(range(kd), key=lambda r: (not 0 <= graph[a][r] < n, detour[r], r))[:g]
        pruned.append([graph[a][r] if 0 <= graph[a][r] < n else -1 for r in ranks])
    rev = [[] for _ in range(n)]
    for b, _, a in sorted((b, r, a) for a in range(n) for r, b in enumerate(pruned[a]) if b >= 0):
        if len(rev[b]) < g:
            rev[b].append(a)
    final = []
    for a in range(n):
        row = []
        for v in pruned[a][:g // 2] + rev[a] + pruned[a][g // 2:]:
            if v >= 0 and v not in row:
                row.append(v)
        final.append((row + [-1] * g)[:g])
    return torch.tensor(final, dtype=torch.int32)


def search_reference(index, queries, k, L, w, seeds, max_iterations=0):
    """cagra_search written from its definition: per query a set and a sorted list."""
    x, graph = index.dataset.double(), index.graph.tolist()
    n = x.shape[0]
    ip = index.metric.value == "inner_product"
    bad = float("-inf") if ip else float("inf")
    dists = torch.full((len(queries), k), bad, dtype=torch.float32)
    ids = torch.full((len(queries), k), -1, dtype=torch.int64)
    for i, qv in enumerate(queries.double()):
        cand = (seeds if seeds.dim() == 1 else seeds[i]).tolist()
        visited, entries = set(), []                    # [sort value, id, expanded]
        for _ in range(max_iterations or L // w + 10):
            for c in cand:
                if 0 <= c < n and c not in visited:
                    visited.add(c)
                    v = float((x[c] * qv).sum()) if ip else float(((x[c] - qv) ** 2).sum())
                    entries.append([-v if ip else v, c, False])
            entries = sorted(entries, key=lambda e: (e[0], e[1]))[:L]
            parents = [e for e in entries if not e[2]][:w]
            if not parents:
                break
            cand = []
            for e in parents:
                e[2] = True
                cand += graph[e[1]]
        for j, e in enumerate(entries[:k]):
            dists[i, j], ids[i, j] = (-e[0] if ip else e[0]), e[1]
    if index.metric.value == "euclidean":
        dists = dists.double().sqrt().float()           # the correctly rounded fp32 root
    return dists, ids
