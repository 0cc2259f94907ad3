"""CAGRA: a fixed-degree graph index, detour-pruned build and greedy search.

Reference parity: cuvs::neighbors::cagra (index_params, build, optimize,
search with the single-CTA algorithm). A kNN graph of intermediate_graph_degree
is pruned to graph_degree by detour counts and merged with its reverse edges;
a query walks the graph from a few seed rows, keeping the itopk_size best rows
seen and expanding the search_width best unexpanded ones per round.

MI355X design (csrc/cagra.hip): cagra_search is one 256-thread block per
query that keeps the query, the sorted (distance, id) list, the candidate
keys and a bounded visited table in LDS; candidate rows are gathered with
refine's sub-wave scheme, sorted and bitonic-merged into the list. cagra_prune
is one block per node with an id -> rank table and the detour counters in LDS.

The plain-torch functions of this file DEFINE the results; the kernels
reproduce them (bit for bit where every distance is exact in fp32). CPU
tensors run torch; on a GPU a shape outside search_kernel_serves /
optimize_kernel_serves takes the torch path under engine="auto", and a GPU
call without the native extension raises.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from raft_amd._ext import require_ext
from raft_amd.distance import DistanceType
from raft_amd.utils import row_chunks

from .ivf_flat import _METRIC_CODES, _resolve_metric

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_ENGINES = ("auto", "kernel", "torch")
_BUILD_ALGOS = ("auto", "brute_force", "ivf_pq")
#: the shapes csrc/cagra.hip serves
_MAX_KERNEL_D = 4096
_MAX_ITOPK = 512
_MAX_CANDIDATES = 512
_MAX_SEEDS = 512
_MAX_HASH_SLOTS = 8192
_MAX_PRUNE_DEGREE = 256
#: rows above which build_algo="auto" takes IVF-PQ. NOT measured: brute force
#: is exact and its cost grows with n^2, nobody has timed the crossover
_AUTO_BRUTE_FORCE_ROWS = 131072
#: elements one chunk of a torch path holds
_TORCH_CHUNK_ELEMS = 1 << 24
_I64_MAX = torch.iinfo(torch.int64).max


def _pow2(v: int) -> int:
    return 1 << max(0, int(v) - 1).bit_length()


def search_kernel_serves(d: int, itopk_size: int, search_width: int, graph_degree: int,
                         k: int) -> bool:
    """Whether csrc/cagra.hip's search kernel serves this shape (cagra_search
    and its tests read this one predicate)."""
    return (1 <= d <= _MAX_KERNEL_D and 1 <= itopk_size <= _MAX_ITOPK and search_width >= 1
            and 1 <= search_width * graph_degree <= _MAX_CANDIDATES and 1 <= k <= itopk_size)


def optimize_kernel_serves(kd: int, graph_degree: int) -> bool:
    """Whether csrc/cagra.hip's prune kernel serves a kNN graph of degree kd."""
    return 1 <= graph_degree <= kd <= _MAX_PRUNE_DEGREE


def auto_hash_slots(itopk_size: int, n_candidates: int, n_seeds: int, iterations: int) -> int:
    """The visited-table size cagra_search picks for hash_slots=0: room for
    the list and min(iterations, 32) rounds of candidates at half load, within
    [the smallest legal table, 8192]."""
    least = _pow2(2 * (itopk_size + max(n_candidates, n_seeds)))
    want = _pow2(2 * (itopk_size + n_candidates * min(iterations, 32)))
    return max(least, min(want, _MAX_HASH_SLOTS))


@dataclass
class CagraParams:
    """Build parameters (reference cagra::index_params). build_algo "auto" is
    brute force up to 131072 rows and IVF-PQ above; that threshold has not
    been measured."""
    graph_degree: int = 64
    intermediate_graph_degree: int = 128
    build_algo: str = "auto"
    metric: DistanceType | str = "sqeuclidean"
    seed: int = 0


class CagraIndex:
    """dataset [n, d] (fp32, bf16 or fp16, stride(1) == 1, any row stride, kept
    as given), graph int32 [n, graph_degree] with -1 for "no edge", seeds int32
    [min(n, 512)] distinct row numbers, metric."""

    def __init__(self, dataset, graph, seeds, metric):
        metric = _resolve_metric(metric)
        if dataset.dim() != 2 or dataset.dtype not in _DTYPES:
            raise ValueError("dataset must be an fp32, bf16 or fp16 tensor [n, d]")
        n, d = dataset.shape
        if d > 1 and dataset.stride(1) != 1:
            raise ValueError("dataset must have stride(1) == 1 (any row stride)")
        if n >= 2 ** 31:
            raise ValueError(f"dataset must have fewer than 2^31 rows, got {n}")
        if graph.dim() != 2 or graph.shape[0] != n or graph.dtype != torch.int32:
            raise ValueError(f"graph must be int32 [{n}, graph_degree]")
        if seeds.dim() != 1 or seeds.dtype != torch.int32 or seeds.numel() > _MAX_SEEDS:
            raise ValueError(f"seeds must be int32 [<= {_MAX_SEEDS}]")
        if graph.device != dataset.device or seeds.device != dataset.device:
            raise ValueError("dataset, graph and seeds must be on one device")
        self.dataset, self.graph = dataset, graph.contiguous()
        self.seeds, self.metric = seeds, metric

    @property
    def n_rows(self) -> int:
        return self.dataset.shape[0]

    @property
    def dim(self) -> int:
        return self.dataset.shape[1]

    @property
    def graph_degree(self) -> int:
        return self.graph.shape[1]

    @property
    def device(self) -> torch.device:
        return self.dataset.device

    def to(self, device) -> "CagraIndex":
        return CagraIndex(self.dataset.to(device), self.graph.to(device), self.seeds.to(device),
                          self.metric)


# ---- optimize ---------------------------------------------------------------

def _prune_torch(graph: torch.Tensor, g: int) -> torch.Tensor:
    """Steps 1-2 in torch: graph int64 [n, kd] with -1 for absent -> int64 [n, g]."""
    n, kd = graph.shape
    dev = graph.device
    out = torch.empty((n, g), dtype=torch.int64, device=dev)
    rank = torch.arange(kd, device=dev)
    for s0, s1 in row_chunks(n, max(1, _TORCH_CHUNK_ELEMS // (kd * kd))):
        row = graph[s0:s1]                                          # [c, kd]
        c = row.shape[0]
        # the row sorted by id (absent last) answers "at which rank does D sit"
        sv, sr = torch.where(row >= 0, row, _I64_MAX).sort(dim=1)
        two = graph[row.clamp(min=0)]                               # [c, kAB, kBD]
        two = torch.where((row >= 0).unsqueeze(2), two, -1).reshape(c, kd * kd)
        pos = torch.searchsorted(sv, two.contiguous()).clamp(max=kd - 1)
        hit = (two >= 0) & (sv.gather(1, pos) == two)
        k_ad = sr.gather(1, pos).reshape(c, kd, kd)
        hit = (hit.reshape(c, kd, kd) & (rank.view(1, kd, 1) < k_ad)
               & (rank.view(1, 1, kd) < k_ad))
        detour = torch.zeros((c, kd), dtype=torch.int64, device=dev)
        detour.scatter_add_(1, k_ad.reshape(c, -1), hit.reshape(c, -1).long())
        key = torch.where(row >= 0, detour * kd + rank, _I64_MAX)
        out[s0:s1] = row.gather(1, key.argsort(dim=1, stable=True)[:, :g])
    return out


def _merge_reverse(pruned: torch.Tensor) -> torch.Tensor:
    """Steps 3-4: pruned int64 [n, g] (-1 absent) -> final int64 [n, g]."""
    n, g = pruned.shape
    dev = pruned.device
    # edges in (r, A) order, then a stable sort by B: every B's sources by (r, A)
    dst = pruned.t().reshape(-1)
    src = torch.arange(n, device=dev).repeat(g)
    keep = dst >= 0
    dst, src = dst[keep], src[keep]
    order = dst.argsort(stable=True)
    dst, src = dst[order], src[order]
    start = torch.searchsorted(dst, torch.arange(n, device=dev))
    pos = torch.arange(dst.numel(), device=dev) - start[dst]
    rev = torch.full((n, g), -1, dtype=torch.int64, device=dev)
    first = pos < g
    rev[dst[first], pos[first]] = src[first]

    both = torch.cat([pruned[:, :g // 2], rev, pruned[:, g // 2:]], dim=1)     # [n, 2g]
    # a repeat is an entry equal to its predecessor in a stable sort by id
    sv, by_id = both.sort(dim=1, stable=True)
    dup_sorted = torch.zeros_like(sv, dtype=torch.bool)
    dup_sorted[:, 1:] = sv[:, 1:] == sv[:, :-1]
    dup = torch.zeros_like(dup_sorted).scatter_(1, by_id, dup_sorted)
    good = (both >= 0) & ~dup
    pick = (~good).long().argsort(dim=1, stable=True)[:, :g]
    return torch.where(good.gather(1, pick), both.gather(1, pick), -1)


def cagra_optimize(knn_graph: torch.Tensor, graph_degree: int, *, engine: str = "auto"):
    """Prune a kNN graph [n, kd] (int32 or int64; every row lists distinct ids
    nearest first, no self-loops; -1 or any id outside [0, n) is absent) to a
    search graph int32 [n, graph_degree] (reference cagra::optimize).

    1. detour[A][kAD] counts the pairs (kAB, kBD) with B = graph[A][kAB],
       D = graph[B][kBD] = graph[A][kAD], kAB < kAD and kBD < kAD: routes
       A -> B -> D that make the edge A -> D redundant.
    2. pruned[A] is the graph_degree ranks with the smallest (detour, rank),
       in that order; absent entries are worst.
    3. every pruned edge (A, r, B) offers A to B; rev[B] is the first
       graph_degree offered sources by (r, A).
    4. final[A] is the first graph_degree distinct present ids of
       pruned[A][:g // 2], rev[A], pruned[A][g // 2:], padded with -1.

    engine: "kernel" runs steps 1-2 in csrc/cagra.hip (kd <= 256) and raises
    on CPU tensors or a larger kd; "torch" is the plain form; "auto" is the
    kernel on a GPU wherever it serves. Steps 3-4 are integer sorts and
    scatters in torch on either device.
    """
    g = int(graph_degree)
    if engine not in _ENGINES:
        raise ValueError(f"engine must be one of {_ENGINES}, got {engine!r}")
    if knn_graph.dim() != 2 or knn_graph.dtype not in (torch.int32, torch.int64):
        raise ValueError("knn_graph must be an int32 or int64 tensor [n, kd]")
    n, kd = knn_graph.shape
    if not 1 <= g <= kd:
        raise ValueError(f"graph_degree must be in [1, {kd}], got {g}")
    if n >= 2 ** 31:
        raise ValueError(f"the graph must have fewer than 2^31 rows, got {n}")
    gpu = knn_graph.device.type == "cuda"
    if gpu:
        require_ext()
    serves = gpu and optimize_kernel_serves(kd, g)
    if engine == "kernel" and not serves:
        raise ValueError(f"engine='kernel' serves GPU graphs with graph_degree <= kd <= "
                         f"{_MAX_PRUNE_DEGREE}; got {knn_graph.device.type}, kd = {kd}")
    if n == 0:
        return torch.empty((0, g), dtype=torch.int32, device=knn_graph.device)
    graph = torch.where((knn_graph >= 0) & (knn_graph < n), knn_graph, -1)
    if serves and engine != "torch":
        pruned = torch.empty((n, g), dtype=torch.int32, device=graph.device)
        require_ext().cagra_prune(graph.int().contiguous(), pruned)
        pruned = pruned.long()
    else:
        pruned = _prune_torch(graph.long(), g)
    return _merge_reverse(pruned).int()


# ---- build ------------------------------------------------------------------

def _knn_graph(x, kd, algo, metric, seed):
    from .brute_force import knn
    n, d = x.shape
    k = kd + 1
    out = torch.empty((n, k), dtype=torch.int64, device=x.device)
    ip = metric == DistanceType.InnerProduct
    if algo == "brute_force":
        xs = x.float().contiguous()                     # widening is exact
        for s0, s1 in row_chunks(n, 8192):
            # the largest products are the smallest products with -q
            out[s0:s1] = (knn(xs, -xs[s0:s1], k, DistanceType.InnerProduct)[1] if ip
                          else knn(xs, xs[s0:s1], k)[1])
        return out
    from .ivf_pq import IvfPqParams, ivf_pq_build, ivf_pq_search
    x32 = x.float().contiguous()
    n_lists = max(1, min(n // 64, int(n ** 0.5)))
    index = ivf_pq_build(x32, IvfPqParams(n_lists=n_lists, metric=metric, seed=seed))
    n_probes = max(1, min(n_lists, max(8, n_lists // 16)))
    for s0, s1 in row_chunks(n, 16384):
        out[s0:s1] = ivf_pq_search(index, x32[s0:s1], k, n_probes, dataset=x, refine_ratio=2)[1]
    return out


def cagra_build(dataset: torch.Tensor, params: CagraParams | None = None, *,
                knn_graph: torch.Tensor | None = None) -> CagraIndex:
    """Build the graph index of dataset [n, d] (reference cagra::build).

    knn_graph, an int32 or int64 [n, kd] graph as cagra_optimize takes it with
    kd >= graph_degree (the ids of neighbors.nn_descent, say), replaces the kNN
    search and the own-id drop described next; build_algo is not read then.

    A kNN graph of degree kd = min(intermediate_graph_degree, n - 1) is
    searched with k = kd + 1: build_algo "brute_force" is knn(x, x, k) in row
    chunks, "ivf_pq" is ivf_pq_build and ivf_pq_search(..., dataset=x,
    refine_ratio=2) in query chunks, "auto" is brute force up to 131072 rows
    and IVF-PQ above (a threshold nobody has measured). Every row then drops
    its own id where it appears, else its last entry, and the graph goes
    through cagra_optimize to min(graph_degree, kd) columns. seeds are
    min(n, 512) distinct rows from a CPU generator seeded with params.seed.
    The dataset is kept as given, in its dtype and with its row stride.
    """
    params = params or CagraParams()
    if params.build_algo not in _BUILD_ALGOS:
        raise ValueError(f"build_algo must be one of {_BUILD_ALGOS}, got {params.build_algo!r}")
    metric = _resolve_metric(params.metric)
    if dataset.dim() != 2 or dataset.dtype not in _DTYPES:
        raise ValueError("dataset must be an fp32, bf16 or fp16 tensor [n, d]")
    n, d = dataset.shape
    if n < 2:
        raise ValueError(f"cagra_build needs at least 2 rows, got {n}")
    if n >= 2 ** 31:
        raise ValueError(f"dataset must have fewer than 2^31 rows, got {n}")
    if params.graph_degree < 1 or params.intermediate_graph_degree < params.graph_degree:
        raise ValueError("need 1 <= graph_degree <= intermediate_graph_degree")
    dev = dataset.device
    if dev.type == "cuda":
        require_ext()
    if knn_graph is not None:
        if (knn_graph.dim() != 2 or knn_graph.dtype not in (torch.int32, torch.int64)
                or knn_graph.shape[0] != n or knn_graph.shape[1] < params.graph_degree
                or knn_graph.device != dev):
            raise ValueError(f"knn_graph must be int32 or int64 [{n}, kd >= graph_degree] on "
                             f"the device of the dataset")
        kd = knn_graph.shape[1]
    else:
        kd = min(int(params.intermediate_graph_degree), n - 1)
        algo = params.build_algo
        if algo == "auto":
            algo = "brute_force" if n <= _AUTO_BRUTE_FORCE_ROWS else "ivf_pq"
        nbrs = _knn_graph(dataset, kd, algo, metric, params.seed)           # [n, kd + 1]
        # drop the own id where it appears, else the last entry; -1 stays
        own = nbrs == torch.arange(n, device=dev).unsqueeze(1)
        own[:, kd] |= ~own.any(dim=1)
        knn_graph = nbrs[~own].reshape(n, kd)
    graph = cagra_optimize(knn_graph, min(int(params.graph_degree), kd))
    gen = torch.Generator().manual_seed(int(params.seed))
    seeds = torch.randperm(n, generator=gen)[:min(n, _MAX_SEEDS)].int().to(dev)
    return CagraIndex(dataset, graph, seeds, metric)


# ---- search -----------------------------------------------------------------

def _sort_entries(val, ids, flag, ip, top):
    """The first `top` entries by (distance, id); id -1 marks an empty entry."""
    ok = ids >= 0
    ids, by_id = torch.where(ok, ids, _I64_MAX).sort(dim=1, stable=True)
    val, flag, ok = val.gather(1, by_id), flag.gather(1, by_id), ok.gather(1, by_id)
    # by id, then stable by value, then stable "empty last": a bad value (+inf
    # after the sign flip) still comes before the empty entries
    order = (-val if ip else val).argsort(dim=1, stable=True)
    order = order.gather(1, (~ok).long().gather(1, order).argsort(dim=1, stable=True))[:, :top]
    ok = ok.gather(1, order)
    return (val.gather(1, order), torch.where(ok, ids.gather(1, order), -1),
            flag.gather(1, order) & ok)


def _search_torch(index, q32, seeds, dists, ids, L, w, max_it):
    x, graph = index.dataset, index.graph
    n, d = x.shape
    g = graph.shape[1]
    ip = index.metric == DistanceType.InnerProduct
    bad = float("-inf") if ip else float("inf")
    dev = q32.device
    k = dists.shape[1]
    width = max(w * g, seeds.shape[1])
    for s0, s1 in row_chunks(q32.shape[0], max(1, _TORCH_CHUNK_ELEMS // max(n, width * d))):
        qc = s1 - s0
        qv = q32[s0:s1].unsqueeze(1)
        cand = (seeds[s0:s1] if seeds.shape[0] > 1 else seeds.expand(qc, -1)).long()
        visited = torch.zeros((qc, n), dtype=torch.bool, device=dev)
        lval = torch.full((qc, L), bad, dtype=torch.float32, device=dev)
        lid = torch.full((qc, L), -1, dtype=torch.int64, device=dev)
        lflag = torch.zeros((qc, L), dtype=torch.bool, device=dev)
        for _ in range(max_it):
            # 1. absent ids, visited ids and repeats within the batch drop out
            cand, _ = torch.where((cand >= 0) & (cand < n), cand, _I64_MAX).sort(dim=1)
            ok = cand < n
            ok[:, 1:] &= cand[:, 1:] != cand[:, :-1]
            cand = cand.clamp(max=n - 1)
            ok &= ~visited.gather(1, cand)
            new = ok.nonzero(as_tuple=True)
            visited[new[0], cand[new]] = True
            # 2. distances of the rest, merged into the sorted list
            rows = x[cand].float()
            val = (rows * qv).sum(dim=2) if ip else ((rows - qv) ** 2).sum(dim=2)
            val = torch.where(val.isnan(), torch.full_like(val, bad), val)
            lval, lid, lflag = _sort_entries(
                torch.cat([lval, val], dim=1), torch.cat([lid, torch.where(ok, cand, -1)], dim=1),
                torch.cat([lflag, torch.zeros_like(ok)], dim=1), ip, L)
            # 3. the first w unexpanded entries become parents
            open_ = (lid >= 0) & ~lflag
            parent = open_ & (open_.long().cumsum(dim=1) <= w)
            if not bool(parent.any()):
                break
            lflag |= parent
            # 4. their graph rows are the next candidates
            order = (~parent).long().argsort(dim=1, stable=True)[:, :w]
            chosen = parent.gather(1, order)
            cand = graph[lid.gather(1, order).clamp(min=0)].long()               # [qc, w, g]
            cand = torch.where(chosen.unsqueeze(2), cand, -1).reshape(qc, -1)
        top = min(k, L)
        out = lval[:, :top]
        if index.metric == DistanceType.L2SqrtExpanded:
            # the fp64 root rounded once: correctly rounded on every device, which
            # torch's fp32 sqrt is not
            out = out.double().sqrt().float()
        dists[s0:s1, :top] = torch.where(lid[:, :top] >= 0, out, torch.full_like(out, bad))
        ids[s0:s1, :top] = lid[:, :top]


def cagra_search(index: CagraIndex, queries: torch.Tensor, k: int, *, itopk_size: int = 64,
                 search_width: int = 1, max_iterations: int = 0, n_seeds: int = 0,
                 seeds: torch.Tensor | None = None, hash_slots: int = 0, engine: str = "auto"):
    """k approximate nearest rows of every query by a greedy walk of the graph
    (reference cagra::search, single-CTA). Returns (dists [q, k] fp32, ids
    [q, k] int64), best first; missing slots hold +inf (-inf for
    inner_product) and id -1. k <= itopk_size.

    Per query, with L = itopk_size and w = search_width: a list of the L best
    rows seen is kept sorted by (distance, smaller id). Round 0 takes the
    seeds as candidates: index.seeds[:n_seeds] (n_seeds = 0 means
    min(L, len(index.seeds))), or the caller's `seeds`, an integer tensor [S]
    for all queries or [q, S] per query, S <= 512. Every round drops absent
    ids (-1 or outside [0, n)), ids whose distance was computed before and
    repeats, computes the rest, merges them into the list, marks the first w
    unexpanded entries expanded and takes their graph rows as the next
    candidates. The walk stops when nothing is unexpanded or after
    max_iterations rounds (0 means L // w + 10, an unmeasured default).

    Squared L2 is the unexpanded fp32 sum of (x - q)^2, inner product the fp32
    sum of x * q (largest first); euclidean takes the correctly rounded fp32
    square root of the final values. A NaN distance becomes the bad value and keeps its id.

    engine: "kernel" is csrc/cagra.hip and raises where search_kernel_serves
    is false or the tensors are on the CPU; "torch" is the plain form; "auto"
    is the kernel on a GPU wherever it serves. hash_slots sizes the kernel's
    visited table, a power of two with 2 * (L + max(w * graph_degree, S)) <=
    hash_slots <= 8192; 0 picks auto_hash_slots. The table is cleared and
    refilled from the list when it is half full, which does not change a
    result: a row outside the list can never re-enter it.
    """
    k, L, w = int(k), int(itopk_size), int(search_width)
    if engine not in _ENGINES:
        raise ValueError(f"engine must be one of {_ENGINES}, got {engine!r}")
    if L < 1 or w < 1 or not 1 <= k <= L:
        raise ValueError(f"need itopk_size >= 1, search_width >= 1 and 1 <= k <= itopk_size; "
                         f"got {L}, {w}, {k}")
    n, d, g = index.n_rows, index.dim, index.graph_degree
    dev = index.device
    if queries.dim() != 2 or queries.shape[1] != d or queries.dtype not in _DTYPES:
        raise ValueError(f"queries must be fp32, bf16 or fp16 [q, {d}], "
                         f"got {tuple(queries.shape)}")
    if queries.device != dev:
        raise ValueError("queries must be on the device of the index")
    q = queries.shape[0]
    if seeds is None:
        n_seeds = int(n_seeds) or min(L, index.seeds.numel())
        if not 1 <= n_seeds <= index.seeds.numel():
            raise ValueError(f"n_seeds must be in [1, {index.seeds.numel()}], got {n_seeds}")
        seeds = index.seeds[:n_seeds]
    if seeds.dtype not in (torch.int32, torch.int64) or seeds.device != dev:
        raise ValueError("seeds must be an int32 or int64 tensor on the device of the index")
    if seeds.dim() == 1:
        seeds = seeds.unsqueeze(0)
    if seeds.dim() != 2 or seeds.shape[0] not in (1, q) or not 1 <= seeds.shape[1] <= _MAX_SEEDS:
        raise ValueError(f"seeds must be [S] or [{q}, S] with 1 <= S <= {_MAX_SEEDS}")
    S = seeds.shape[1]
    max_it = int(max_iterations) or L // w + 10
    if max_it < 1:
        raise ValueError(f"max_iterations must not be negative, got {max_iterations}")
    gpu = dev.type == "cuda"
    if gpu:
        require_ext()
    serves = gpu and search_kernel_serves(d, L, w, g, k)
    if engine == "kernel" and not serves and q:
        raise ValueError(f"engine='kernel' serves GPU tensors with d <= {_MAX_KERNEL_D}, "
                         f"itopk_size <= {_MAX_ITOPK}, search_width * graph_degree <= "
                         f"{_MAX_CANDIDATES} and k <= itopk_size; got {dev.type}, d = {d}, "
                         f"itopk_size = {L}, candidates = {w * g}, k = {k}")
    H = int(hash_slots)
    if H and (H & (H - 1) or not 2 * (L + max(w * g, S)) <= H <= _MAX_HASH_SLOTS):
        raise ValueError(f"hash_slots must be a power of two in [{2 * (L + max(w * g, S))}, "
                         f"{_MAX_HASH_SLOTS}], got {H}")

    bad = float("-inf") if index.metric == DistanceType.InnerProduct else float("inf")
    dists = torch.full((q, k), bad, dtype=torch.float32, device=dev)
    ids = torch.full((q, k), -1, dtype=torch.int64, device=dev)
    if q == 0 or n == 0:
        return dists, ids
    q32 = queries.float().contiguous()
    if serves and engine != "torch":
        # an id beyond int32 is absent either way
        s32 = torch.where((seeds >= 0) & (seeds < n), seeds, -1).int().contiguous()
        require_ext().cagra_search(index.dataset, index.graph, q32, s32, dists, ids, L, w, max_it,
                                   H or auto_hash_slots(L, w * g, S, max_it),
                                   _METRIC_CODES[index.metric])
    else:
        _search_torch(index, q32, seeds, dists, ids, L, w, max_it)
    return dists, ids
