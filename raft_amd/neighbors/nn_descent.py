"""NN-descent: an all-neighbours kNN graph by iterated local joins.

Reference parity: cuvs::neighbors::nn_descent (the GNND builder behind
cagra::build). Every row keeps a list of its k best rows seen so far; per
iteration every node joins a sample of its new neighbours with its sampled
neighbours and reverse neighbours, and every pair so met offers itself to both
lists. No n^2 distances are computed and nothing is trained.

MI355X design (csrc/nn_descent.hip): nn_descent_join is one block per node, a
64 x 128 bf16 MFMA tile over rows gathered by id in the data set's own dtype
and row stride, double-buffered through XOR-swizzled LDS, with the best
partner per row and column reduced in registers and LDS; nn_descent_merge is
one block per target that removes repeats and bitonic-sorts the list with its
candidates in LDS. The distance tile never reaches memory.

The plain-torch functions of this file DEFINE the results; the kernels
reproduce them (bit for bit where every value is exact in bf16 and fp32).
Every step is a set function or a fixed-order sort, nothing depends on
scheduling.

State per row, K = k entries (sort value fp32, id int32, new flag), ascending
by (value, id); an absent slot is (+inf, -1, False). The sort value is the
squared L2 distance, or -dot for inner_product. "Ordered value bits" are the
fp32 bits mapped to ascend as unsigned, NaN as +inf and -0 as +0.

1. Init. Row i draws K ids u % (n - 1), raised by one where >= i, with u the
   PCG32 draws of random/rng.py at flat index i * K + j (seed, subsequence 0):
   equal on CPU and GPU. neighbors.refine gives their exact values; repeats
   are dropped; every entry is flagged new.
2. Sample, S = n_samples (integer torch ops on both paths). F_new(i) is the
   first S new-flagged entries of row i in list order, F_old(i) the first S
   old ones. R_new(j) is the i with j in F_new(i): the first S after a stable
   sort of the row-major flattened pairs by (j, ordered value bits); R_old
   likewise. The F_new entries lose their new flag. NEW_c = F_new(c) ++
   R_new(c) and OLD_c = F_old(c) ++ R_old(c), 2S ids each, -1 padded, repeats
   allowed.
3. Local join, per node c; pairs with equal ids or a -1 are skipped. Every u
   in NEW_c gets its best v in NEW_c and its best v in OLD_c, every u in OLD_c
   its best v in NEW_c; best is the smallest (value(u, v), v) with value =
   (|u|^2 + |v|^2) - 2 u.v, the norms in fp32 and summed first. The output is
   6S triples (target u, id v, value) at fixed positions [NEW|NEW, NEW|OLD,
   OLD|NEW], (-1, -1, +inf) where there is none. The join reads the sample
   lists and the data set, never the neighbour lists.
4. Merge, per target u: the new list is the K smallest (value, id) with
   distinct ids over the old list and the triples aimed at u. An id already
   listed keeps its entry and flag; of several triples with one id the
   smallest value counts; an inserted id is flagged new; u never enters its
   own list.
5. Stop after max_iterations, or when the update count of an iteration, the
   new-flagged entries after the merge minus those left after step 2, is at
   most termination_threshold * n * K.
6. Finish. neighbors.refine re-ranks every row's ids by exact fp32 distance;
   euclidean takes the correctly rounded root of those.

Steps 3 and 4 are set functions and the join does not read the lists, so nodes
are processed in chunks (join a chunk, merge it) sized from the workspace
budget, with the same results where the values are exact.

CPU tensors run torch; on a GPU a shape outside nn_descent_kernel_serves takes
the torch path under engine="auto", and a GPU call without the native
extension raises.
"""
from __future__ import annotations

import torch

from raft_amd._ext import require_ext
from raft_amd.distance import DistanceType
from raft_amd.linalg.split_bf16 import row_sqnorms
from raft_amd.random.rng import _pcg32_block
from raft_amd.utils import row_chunks

from .ivf_flat import _METRIC_CODES, _resolve_metric
from .refine import refine

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_ENGINES = ("auto", "kernel", "torch")
#: the shapes csrc/nn_descent.hip serves
_MAX_KERNEL_D = 4096
_MAX_KERNEL_K = 256
_MAX_KERNEL_SAMPLES = 32
#: elements one chunk of a torch path holds
_TORCH_CHUNK_ELEMS = 1 << 24
#: bytes per triple a node chunk is sized with: the triple, its sort and gather
_TRIPLE_BYTES = 48
_I64_MAX = torch.iinfo(torch.int64).max


def nn_descent_kernel_serves(d: int, k: int, n_samples: int) -> bool:
    """Whether csrc/nn_descent.hip serves this shape (nn_descent and its tests
    read this one predicate)."""
    return (1 <= d <= _MAX_KERNEL_D and 1 <= k <= _MAX_KERNEL_K
            and 1 <= n_samples <= _MAX_KERNEL_SAMPLES)


def _ordered_bits(val: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 in [0, 2^32) ascending with the value; NaN as +inf, -0 as +0."""
    val = torch.where(val.isnan(), torch.full_like(val, float("inf")), val) + 0.0
    b = val.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return torch.where(b >= 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


def _pick_engine(engine, dev, serves, what):
    if engine not in _ENGINES:
        raise ValueError(f"engine must be one of {_ENGINES}, got {engine!r}")
    gpu = dev.type == "cuda"
    if gpu:
        require_ext()
    if engine == "kernel" and not (gpu and serves):
        raise ValueError(f"engine='kernel' serves GPU tensors with {what}; got {dev.type} tensors")
    return gpu and serves and engine != "torch"


def _check_dataset(dataset):
    if dataset.dim() != 2 or dataset.dtype not in _DTYPES:
        raise ValueError("dataset must be an fp32, bf16 or fp16 tensor [n, d]")
    n, d = dataset.shape
    if d < 1 or (d > 1 and dataset.stride(1) != 1):
        raise ValueError("dataset must have d >= 1 and stride(1) == 1 (any row stride)")
    if n >= 2 ** 31:
        raise ValueError(f"dataset must have fewer than 2^31 rows, got {n}")


def _norms(x):
    rows = max(1, _TORCH_CHUNK_ELEMS // x.shape[1])
    return torch.cat([row_sqnorms(x[s0:s1]) for s0, s1 in row_chunks(x.shape[0], rows)])


# ---- step 1 -----------------------------------------------------------------

def init_lists(x, K, metric="sqeuclidean", seed=0, refine_engine="auto"):
    """Step 1: (vals fp32, ids int32, flags bool), each [n, K]."""
    metric = _resolve_metric(metric)
    n, d = x.shape
    dev = x.device
    ip = metric == DistanceType.InnerProduct
    vals = torch.full((n, K), float("inf"), dtype=torch.float32, device=dev)
    ids = torch.full((n, K), -1, dtype=torch.int32, device=dev)
    flags = torch.zeros((n, K), dtype=torch.bool, device=dev)
    if n < 2:
        return vals, ids, flags
    cols = torch.arange(K, device=dev)
    for s0, s1 in row_chunks(n, max(1, _TORCH_CHUNK_ELEMS // (K * d))):
        rows = torch.arange(s0, s1, device=dev).unsqueeze(1)
        draw = _pcg32_block(int(seed), 0, (rows * K + cols).reshape(-1)).reshape(s1 - s0, K)
        cand = draw % (n - 1)
        cand = cand + (cand >= rows)
        dist, got = refine(x, x[s0:s1], cand, K, metric, engine=refine_engine)
        # refine sorts by (value, id): a repeat follows its first occurrence
        dup = torch.zeros_like(got, dtype=torch.bool)
        dup[:, 1:] = got[:, 1:] == got[:, :-1]
        order = dup.long().argsort(dim=1, stable=True)
        keep = ~dup.gather(1, order)
        val = (-dist if ip else dist).gather(1, order)
        vals[s0:s1] = torch.where(keep, val, torch.full_like(val, float("inf")))
        ids[s0:s1] = torch.where(keep, got.gather(1, order), -1).int()
        flags[s0:s1] = keep
    return vals, ids, flags


# ---- step 2 -----------------------------------------------------------------

def sample_lists(vals, ids, flags, n_samples):
    """Step 2: (NEW, OLD) int32 [n, 2S] of the lists; clears the new flag of the
    sampled new entries IN PLACE."""
    n, K = ids.shape
    S = int(n_samples)
    dev = ids.device
    valid = ids >= 0
    rows = torch.arange(n, device=dev)
    out = []
    sampled_new = None
    for sel in (valid & flags, valid & ~flags):
        pos = (~sel).long().argsort(dim=1, stable=True)[:, :S]
        ok = sel.gather(1, pos)
        f_id = torch.where(ok, ids.gather(1, pos).long(), -1)
        both = torch.full((n, 2 * S), -1, dtype=torch.int64, device=dev)
        both[:, :pos.shape[1]] = f_id
        # reverse samples: the pairs in row-major order, stably sorted by (j, value)
        dst, src = f_id[ok], rows.unsqueeze(1).expand_as(f_id)[ok]
        order = ((dst << 32) | _ordered_bits(vals.gather(1, pos)[ok])).argsort(stable=True)
        dst, src = dst[order].contiguous(), src[order]
        rank = torch.arange(dst.numel(), device=dev) - torch.searchsorted(dst, rows)[dst]
        first = rank < S
        both[dst[first], S + rank[first]] = src[first]
        out.append(both.int())
        if sampled_new is None:
            sampled_new = torch.zeros_like(flags).scatter_(1, pos, ok)
    flags &= ~sampled_new
    return out[0], out[1]


# ---- step 3 -----------------------------------------------------------------

def _best(val, ok, vid, dim):
    """Per slice along dim: (smallest value, smallest id at that value, any valid)."""
    val = torch.where(ok, val, torch.full_like(val, float("inf")))
    vmin = val.min(dim=dim, keepdim=True).values
    bid = torch.where(ok & (val == vmin), vid, _I64_MAX).min(dim=dim).values
    return vmin.squeeze(dim), bid, ok.any(dim=dim)


def _join_torch(x, norms, new_ids, old_ids, ip, target, cand_id, cand_val):
    n, d = x.shape
    m, S2 = new_ids.shape
    inf = float("inf")
    for s0, s1 in row_chunks(m, max(1, _TORCH_CHUNK_ELEMS // (3 * S2 * max(d, 2 * S2)))):
        a, o = new_ids[s0:s1].long(), old_ids[s0:s1].long()
        a = torch.where((a >= 0) & (a < n), a, -1)
        o = torch.where((o >= 0) & (o < n), o, -1)
        b = torch.cat([a, o], dim=1)
        ga, gb = a.clamp(min=0), b.clamp(min=0)
        dot = torch.bmm(x[ga].float(), x[gb].float().transpose(1, 2))       # [c, 2S, 4S]
        val = -dot if ip else (norms[ga].unsqueeze(2) + norms[gb].unsqueeze(1)) - 2.0 * dot
        val = torch.where(val.isnan(), torch.full_like(val, inf), val) + 0.0
        ok = (a >= 0).unsqueeze(2) & (b >= 0).unsqueeze(1) & (a.unsqueeze(2) != b.unsqueeze(1))
        parts = [_best(val[:, :, :S2], ok[:, :, :S2], a.unsqueeze(1), 2) + (a,),
                 _best(val[:, :, S2:], ok[:, :, S2:], o.unsqueeze(1), 2) + (a,),
                 _best(val[:, :, S2:], ok[:, :, S2:], a.unsqueeze(2), 1) + (o,)]
        for p, (v, i, hit, u) in enumerate(parts):
            target[s0:s1, p * S2:(p + 1) * S2] = torch.where(hit, u, -1)
            cand_id[s0:s1, p * S2:(p + 1) * S2] = torch.where(hit, i, -1)
            cand_val[s0:s1, p * S2:(p + 1) * S2] = torch.where(hit, v, torch.full_like(v, inf))


def local_join(dataset, norms, new_ids, old_ids, metric="sqeuclidean", *, engine="auto"):
    """Step 3 for the nodes whose sample lists are new_ids / old_ids (int32
    [m, 2S], -1 or any id outside [0, n) is no row); norms fp32 [n] are the
    squared row norms. Returns (target int32, id int32, value fp32), each
    [m, 6S]. engine as in nn_descent."""
    metric = _resolve_metric(metric)
    _check_dataset(dataset)
    n, d = dataset.shape
    if (new_ids.dim() != 2 or new_ids.dtype != torch.int32 or new_ids.shape[1] % 2
            or new_ids.shape[1] < 2 or old_ids.shape != new_ids.shape
            or old_ids.dtype != torch.int32):
        raise ValueError("new_ids and old_ids must be int32 [m, 2 * n_samples]")
    if norms.shape != (n,) or norms.dtype != torch.float32:
        raise ValueError(f"norms must be fp32 [{n}]")
    dev = dataset.device
    if norms.device != dev or new_ids.device != dev or old_ids.device != dev:
        raise ValueError("all tensors must be on one device")
    m, S2 = new_ids.shape
    kernel = _pick_engine(engine, dev, 1 <= d <= _MAX_KERNEL_D and S2 <= 2 * _MAX_KERNEL_SAMPLES
                          and n >= 1, f"d <= {_MAX_KERNEL_D} and n_samples <= "
                          f"{_MAX_KERNEL_SAMPLES}")
    target = torch.full((m, 3 * S2), -1, dtype=torch.int32, device=dev)
    cand_id = torch.full((m, 3 * S2), -1, dtype=torch.int32, device=dev)
    cand_val = torch.full((m, 3 * S2), float("inf"), dtype=torch.float32, device=dev)
    if m == 0 or n == 0:
        return target, cand_id, cand_val
    if kernel:
        require_ext().nn_descent_join(dataset, norms.contiguous(), new_ids.contiguous(),
                                      old_ids.contiguous(), target, cand_id, cand_val,
                                      _METRIC_CODES[metric])
    else:
        _join_torch(dataset, norms, new_ids, old_ids, metric == DistanceType.InnerProduct,
                    target, cand_id, cand_val)
    return target, cand_id, cand_val


# ---- step 4 -----------------------------------------------------------------

def _two_key_order(major, minor):
    """The permutation that sorts by (major, minor), stable."""
    order = minor.argsort(stable=True)
    return order[major[order].argsort(stable=True)]


def _merge_torch(vals, ids, flags, target, cand_id, cand_val):
    """Step 4 in place on the rows that are targets; returns the update count."""
    n, K = ids.shape
    dev = ids.device
    t, c, v = target.reshape(-1).long(), cand_id.reshape(-1).long(), cand_val.reshape(-1)
    keep = (t >= 0) & (c >= 0) & (c < n) & (c != t)
    t, c, v = t[keep], c[keep], v[keep]
    if t.numel() == 0:
        return 0
    rows = t.unique()                                               # ascending
    r = rows.numel()
    ev, ei, ef = vals[rows], ids[rows].long(), flags[rows]
    ok = ei >= 0
    before = int((ok & ef).sum())
    listed = ok.sum()
    row = torch.cat([torch.arange(r, device=dev).unsqueeze(1).expand(r, K)[ok],
                     torch.searchsorted(rows, t)])
    eid = torch.cat([ei[ok], c])
    bits = torch.cat([_ordered_bits(ev[ok]), _ordered_bits(v)])
    flag = torch.cat([ef[ok], torch.ones_like(c, dtype=torch.bool)])
    src = (torch.arange(row.numel(), device=dev) >= listed).long()
    # by (row, id, source, value): the first of every (row, id) stays
    order = _two_key_order((row << 31) | eid, (src << 32) | bits)
    key = ((row << 31) | eid)[order]
    firsts = torch.ones_like(key, dtype=torch.bool)
    firsts[1:] = key[1:] != key[:-1]
    sel = order[firsts]
    # by (row, value, id): the first K of every row
    sel = sel[_two_key_order(row[sel], (bits[sel] << 31) | eid[sel])]
    rr = row[sel].contiguous()
    rank = torch.arange(rr.numel(), device=dev) - torch.searchsorted(
        rr, torch.arange(r, device=dev))[rr]
    sel, rr, rank = sel[rank < K], rr[rank < K], rank[rank < K]
    nv = torch.full((r, K), float("inf"), dtype=torch.float32, device=dev)
    ni = torch.full((r, K), -1, dtype=torch.int32, device=dev)
    nf = torch.zeros((r, K), dtype=torch.bool, device=dev)
    b = bits[sel]
    b = torch.where(b >= 0x80000000, b ^ 0x80000000, b ^ 0xFFFFFFFF)
    nv[rr, rank] = torch.where(b >= 0x80000000, b - (1 << 32), b).int().view(torch.float32)
    ni[rr, rank] = eid[sel].int()
    nf[rr, rank] = flag[sel]
    vals[rows], ids[rows], flags[rows] = nv, ni, nf
    return int(nf.sum()) - before


def _merge_kernel(vals, ids, flags, target, cand_id, cand_val, counter):
    """Step 4 in place through csrc/nn_descent.hip; counter int64 [1] gains the update count."""
    n = ids.shape[0]
    # triples grouped by target: a stable sort of the target column, segment offsets
    ts, order = target.reshape(-1).sort(stable=True)
    seg_off = torch.searchsorted(ts, torch.arange(n + 1, dtype=torch.int32, device=ts.device))
    require_ext().nn_descent_merge(vals, ids, flags, seg_off,
                                   cand_id.reshape(-1)[order].contiguous(),
                                   cand_val.reshape(-1)[order].contiguous(), counter)


def merge_candidates(vals, ids, flags, target, cand_id, cand_val, *, engine="auto"):
    """Step 4: the lists (vals fp32, ids int32, flags bool, each [n, K]) with the
    triples of local_join merged in. Returns (vals, ids, flags, update count);
    the inputs are left as they are. engine as in nn_descent."""
    if (vals.dim() != 2 or vals.dtype != torch.float32 or ids.dtype != torch.int32
            or flags.dtype != torch.bool or ids.shape != vals.shape or flags.shape != vals.shape):
        raise ValueError("vals fp32, ids int32 and flags bool must be [n, K]")
    if (target.dtype != torch.int32 or cand_id.dtype != torch.int32
            or cand_val.dtype != torch.float32 or target.shape != cand_id.shape
            or target.shape != cand_val.shape):
        raise ValueError("target int32, cand_id int32 and cand_val fp32 must have one shape")
    n, K = ids.shape
    kernel = _pick_engine(engine, vals.device, 1 <= K <= _MAX_KERNEL_K and n < 2 ** 31,
                          f"K <= {_MAX_KERNEL_K}")
    vals, ids, flags = vals.clone(), ids.clone(), flags.clone()
    if n == 0 or target.numel() == 0:
        return vals, ids, flags, 0
    if kernel:
        counter = torch.zeros(1, dtype=torch.int64, device=vals.device)
        _merge_kernel(vals, ids, flags, target, cand_id, cand_val, counter)
        return vals, ids, flags, int(counter)
    return vals, ids, flags, _merge_torch(vals, ids, flags, target, cand_id, cand_val)


# ---- the driver -------------------------------------------------------------

def nn_descent(dataset: torch.Tensor, k: int, *, n_samples: int = 32, max_iterations: int = 20,
               termination_threshold: float = 1e-4, metric="sqeuclidean", seed: int = 0,
               engine: str = "auto", res=None):
    """The approximate k nearest rows of every row of dataset [n, d] (fp32, bf16
    or fp16, stride(1) == 1, any row stride, read in place), by the algorithm
    of this module's docstring. Returns (dists [n, k] fp32, ids [n, k] int64):
    row i holds k distinct ids != i, ascending by (sort value, id), with the
    exact fp32 distance (the product for inner_product, largest first); rows
    are padded with (+inf, -1) (-inf for inner_product) when n - 1 < k.

    metric is sqeuclidean, euclidean (the root taken at the very end) or
    inner_product. seed must be in [0, 2^63).

    engine: "kernel" is csrc/nn_descent.hip and raises where
    nn_descent_kernel_serves is false or the tensors are on the CPU; "torch" is
    the plain form; "auto" is the kernel on a GPU wherever it serves. The node
    chunk of steps 3-4 comes from half the workspace budget of res.
    """
    from raft_amd.core.resources import get_resources
    k, S = int(k), int(n_samples)
    metric = _resolve_metric(metric)
    _check_dataset(dataset)
    if k < 1 or S < 1 or int(max_iterations) < 0:
        raise ValueError(f"need k >= 1, n_samples >= 1 and max_iterations >= 0; got {k}, {S}, "
                         f"{max_iterations}")
    n, d = dataset.shape
    dev = dataset.device
    kernel = _pick_engine(engine, dev, nn_descent_kernel_serves(d, k, S),
                          f"d <= {_MAX_KERNEL_D}, k <= {_MAX_KERNEL_K} and n_samples <= "
                          f"{_MAX_KERNEL_SAMPLES}")
    step = "kernel" if kernel else "torch"
    ip = metric == DistanceType.InnerProduct
    work_metric = DistanceType.InnerProduct if ip else DistanceType.L2Expanded
    refine_engine = "torch" if engine == "torch" else "auto"

    vals, ids, flags = init_lists(dataset, k, work_metric, seed, refine_engine)
    if n >= 2:
        norms = _norms(dataset)
        budget = get_resources(res if res is not None else dev).workspace_budget() // 2
        chunk = int(max(1, min(n, budget // (6 * S * _TRIPLE_BYTES))))
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(int(max_iterations)):
            new_ids, old_ids = sample_lists(vals, ids, flags, S)
            counter.zero_()
            for s0, s1 in row_chunks(n, chunk):
                triples = local_join(dataset, norms, new_ids[s0:s1], old_ids[s0:s1], work_metric,
                                     engine=step)
                if kernel:
                    _merge_kernel(vals, ids, flags, *triples, counter)
                else:
                    counter += _merge_torch(vals, ids, flags, *triples)
            if int(counter) <= termination_threshold * n * k:     # the one host read
                break

    bad = float("-inf") if ip else float("inf")
    dists = torch.full((n, k), bad, dtype=torch.float32, device=dev)
    out = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    for s0, s1 in row_chunks(n, max(1, _TORCH_CHUNK_ELEMS // (k * d))):
        dists[s0:s1], out[s0:s1] = refine(dataset, dataset[s0:s1], ids[s0:s1].long(), k,
                                          work_metric, engine=refine_engine)
    if metric == DistanceType.L2SqrtExpanded:
        # the fp64 root rounded once: correctly rounded on every device
        dists = dists.double().sqrt().float()
    return dists, out
