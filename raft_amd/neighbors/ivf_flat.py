"""IVF-Flat: an inverted-file index over uncompressed vectors.

Reference parity: the historical raft::neighbors::ivf_flat::{build, extend,
search, serialize}. The data set is partitioned by a balanced k-means into
n_lists lists; a search ranks the list centroids (the coarse step), scans only
the n_probes best lists of every query and selects the k best rows among them.

Storage is ONE layout on CPU and GPU. Rows are sorted by list, every list is
padded to a multiple of 64 rows (the wave width) and rows are interleaved in
groups of 64: with V = 16 bytes of elements (4 fp32, 8 bf16) and d_pad = d
rounded up to V with zeros, element (group g, chunk j, row r, v) lives at

    ((g * (d_pad / V) + j) * 64 + r) * V + v

so a wave that reads chunk j of a group reads 1 KiB contiguous, 16 B per lane,
lane = row. Packing is plain torch (gather, view, permute); IvfFlatIndex
.unpack_list is its inverse.

MI355X design (csrc/ivf_flat_scan.hip): the scan is LIST-major. The
(query, probe) pairs of a query chunk are sorted by list with device-side torch
ops and cut into groups of at most QG queries; one block stages its group's
queries in LDS and streams the list once for all of them, accumulating the
unexpanded fp32 sum of squares (or the dot product) with lane = row and no
cross-lane reduction. Distances go to a ragged candidate buffer (one row per
query: its padded probed lists in probe order) taken from the Resources
workspace, and the generic ragged-row select engine picks the k best. The
buffer is sized from n_probes * the longest padded list, so a query chunk
needs no host sync.

CPU tensors, and GPU indices with d_pad > 4096 or fp32_mode="native", run the
same algorithm with plain torch ops over unpack_list (on the GPU the select
still uses the native engine). A GPU search without the native extension
raises.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import torch

from raft_amd._ext import require_ext
from raft_amd.core.bitset import Bitset
from raft_amd.core.serialize import deserialize_mdspan, serialize_mdspan
from raft_amd.distance import DistanceType, pairwise_distance
from raft_amd.matrix.select_k import select_k
from raft_amd.utils import row_chunks

_GROUP = 64
#: metric -> code of ext.ivf_flat_scan
_METRIC_CODES = {DistanceType.L2Expanded: 0, DistanceType.L2SqrtExpanded: 1,
                 DistanceType.InnerProduct: 2}
_DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1}
#: queries one block stages: 8 measured faster than 4, 16 and 32
#: (docs/performance.md, "IVF-Flat"); the LDS tier ext.ivf_flat_scan_max_qg
#: lowers it for wide rows
_DEFAULT_QG = 8
_QG_CHOICES = (4, 8, 16, 32)
#: widest padded row the scan kernel stages; wider indices take the torch path
_MAX_KERNEL_D_PAD = 4096
#: blocks one launch aims for, the masked L2-NN's policy
_TARGET_BLOCKS = 1024
_MAGIC = b"RAFTAMD_IVFFLAT\x00"
_VERSION = 1
_HEADER = "<16s6q16s"


def _resolve_metric(metric) -> DistanceType:
    if isinstance(metric, str):
        for m in _METRIC_CODES:
            if metric == m.value or metric.lower() == m.name.lower():
                return m
        raise ValueError(f"ivf_flat supports sqeuclidean, euclidean and inner_product, "
                         f"got {metric!r}")
    if metric not in _METRIC_CODES:
        raise ValueError(f"ivf_flat supports L2Expanded, L2SqrtExpanded and "
                         f"InnerProduct, got {metric!r}")
    return metric


@dataclass
class IvfFlatParams:
    """Build parameters (reference ivf_flat::index_params).

    The centroids are trained by kmeans_balanced_fit on a
    kmeans_trainset_fraction sample drawn with seed, ALWAYS with plain L2,
    also for InnerProduct (rows are assigned to their L2-nearest centroid; the
    coarse step of a search ranks centroids by the index metric)."""
    n_lists: int = 1024
    metric: DistanceType | str = "sqeuclidean"
    kmeans_n_iters: int = 20
    kmeans_trainset_fraction: float = 0.5
    add_data_on_build: bool = True
    seed: int = 0
    fp32_mode: str = "auto"


class IvfFlatIndex:
    """The index: centroids [n_lists, d] fp32, list_offsets int64 [n_lists+1]
    in rows (multiples of 64), list_sizes int64 [n_lists] (true sizes), data
    (the flat interleaved buffer, fp32 or bf16), indices int64 [padded rows]
    (dataset ids, -1 in pad slots), metric, dim, n_rows."""

    def __init__(self, centroids, list_offsets, list_sizes, data, indices, metric,
                 dim, n_rows, fp32_mode="auto"):
        self.centroids = centroids
        self.list_offsets = list_offsets
        self.list_sizes = list_sizes
        self.data = data
        self.indices = indices
        self.metric = _resolve_metric(metric)
        self.dim = int(dim)
        self.n_rows = int(n_rows)
        self.fp32_mode = fp32_mode
        padded = list_offsets[1:] - list_offsets[:-1]
        #: longest padded list, known on the host: sizes the candidate buffer
        self.max_list_pad = int(padded.max()) if padded.numel() else 0

    @property
    def n_lists(self) -> int:
        return self.centroids.shape[0]

    @property
    def dtype(self) -> torch.dtype:
        return self.data.dtype

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def vec(self) -> int:
        """Elements in one 16-byte chunk."""
        return 16 // self.data.element_size()

    @property
    def d_pad(self) -> int:
        return -(-self.dim // self.vec) * self.vec

    def to(self, device) -> "IvfFlatIndex":
        return IvfFlatIndex(self.centroids.to(device), self.list_offsets.to(device),
                            self.list_sizes.to(device), self.data.to(device),
                            self.indices.to(device), self.metric, self.dim,
                            self.n_rows, self.fp32_mode)

    def _padded_rows(self) -> torch.Tensor:
        """All padded rows [total, dim] in slot order (de-interleaved copy)."""
        total = self.indices.numel()
        v, dp = self.vec, self.d_pad
        rows = self.data.view(total // _GROUP, dp // v, _GROUP, v).permute(0, 2, 1, 3)
        return rows.reshape(total, dp)[:, :self.dim]

    def unpack_list(self, l: int):
        """The rows [size, d] and dataset ids [size] of list l."""
        r0 = int(self.list_offsets[l])
        r1 = int(self.list_offsets[l + 1])
        size = int(self.list_sizes[l])
        v, dp = self.vec, self.d_pad
        g = self.data.view(-1, dp // v, _GROUP, v)[r0 // _GROUP:r1 // _GROUP]
        rows = g.permute(0, 2, 1, 3).reshape(r1 - r0, dp)[:size, :self.dim]
        return rows.contiguous(), self.indices[r0:r0 + size]


def _pack(rows, ids, labels, n_lists, dim):
    """Sort rows by list, pad every list to 64 rows, interleave."""
    dev = rows.device
    n = rows.shape[0]
    v = 16 // rows.element_size()
    d_pad = -(-dim // v) * v
    sizes = torch.bincount(labels, minlength=n_lists)
    padded = (sizes + (_GROUP - 1)) // _GROUP * _GROUP
    offsets = torch.zeros(n_lists + 1, dtype=torch.int64, device=dev)
    offsets[1:] = padded.cumsum(0)
    total = int(offsets[-1])
    order = torch.argsort(labels, stable=True)
    sl = labels[order]
    starts = sizes.cumsum(0) - sizes
    dest = offsets[sl] + (torch.arange(n, device=dev) - starts[sl])
    buf = torch.zeros((total, d_pad), dtype=rows.dtype, device=dev)
    buf[dest, :dim] = rows[order]
    indices = torch.full((total,), -1, dtype=torch.int64, device=dev)
    indices[dest] = ids[order]
    data = (buf.view(total // _GROUP, _GROUP, d_pad // v, v).permute(0, 2, 1, 3)
            .contiguous().view(-1))
    return offsets, sizes, data, indices


def _check_vectors(x, what):
    if x.dim() != 2 or not x.dtype.is_floating_point:
        raise ValueError(f"{what} must be a 2-D floating-point tensor [rows, features]")
    if x.dtype == torch.float16:
        x = x.float()   # exact widening, as everywhere else
    if x.dtype not in _DTYPE_CODES:
        raise ValueError(f"{what} must be fp32, bf16 or fp16, got {x.dtype}")
    return x


def ivf_flat_build(x: torch.Tensor, params: IvfFlatParams | None = None, *,
                   centroids: torch.Tensor | None = None, res=None) -> IvfFlatIndex:
    """Build an IVF-Flat index over x [n, d] (reference ivf_flat::build).

    x is fp32 or bf16 (fp16 is widened to fp32, which is exact); centroids and
    returned distances are fp32. The centroids come from kmeans_balanced_fit
    on a params.kmeans_trainset_fraction sample with params.seed, always with
    plain L2 (also for InnerProduct); rows are assigned with kmeans_predict.
    centroids= [n_lists, d] skips the training (an index built elsewhere, or
    forced list shapes) and overrides params.n_lists.
    params.add_data_on_build=False returns an index with empty lists.
    """
    from raft_amd.cluster.kmeans import kmeans_balanced_fit
    params = params if params is not None else IvfFlatParams()
    metric = _resolve_metric(params.metric)
    x = _check_vectors(x, "x")
    n, d = x.shape
    if d < 1:
        raise ValueError("x needs at least one feature")
    if centroids is None:
        n_lists = int(params.n_lists)
        if n_lists < 1 or n_lists > n:
            raise ValueError(f"n_lists must be in [1, {n}], got {n_lists}")
        model = kmeans_balanced_fit(x.float(), n_lists, max_iter=params.kmeans_n_iters,
                                    seed=params.seed,
                                    sample_fraction=params.kmeans_trainset_fraction,
                                    fp32_mode=params.fp32_mode)
        centroids = model.centroids
    elif centroids.dim() != 2 or centroids.shape[1] != d or centroids.shape[0] < 1:
        raise ValueError(f"centroids must be [n_lists, {d}]")
    centroids = centroids.to(x.device, torch.float32).contiguous()
    n_lists = centroids.shape[0]
    dev = x.device
    index = IvfFlatIndex(
        centroids, torch.zeros(n_lists + 1, dtype=torch.int64, device=dev),
        torch.zeros(n_lists, dtype=torch.int64, device=dev),
        torch.empty(0, dtype=x.dtype, device=dev),
        torch.empty(0, dtype=torch.int64, device=dev), metric, d, 0, params.fp32_mode)
    if params.add_data_on_build:
        return ivf_flat_extend(index, x, res=res)
    return index


def ivf_flat_extend(index: IvfFlatIndex, new_vectors: torch.Tensor,
                    new_indices: torch.Tensor | None = None, *, res=None) -> IvfFlatIndex:
    """Add rows to an index (reference ivf_flat::extend). Functional: returns
    a NEW index and leaves the centroids unchanged. The new rows are assigned
    with kmeans_predict, appended to their lists and the whole buffer is
    repacked. new_indices defaults to arange(n_rows, n_rows + m)."""
    from raft_amd.cluster.kmeans import kmeans_predict
    new_vectors = _check_vectors(new_vectors, "new_vectors")
    if new_vectors.shape[1] != index.dim:
        raise ValueError(f"new_vectors has {new_vectors.shape[1]} features, the index "
                         f"has {index.dim}")
    if new_vectors.dtype != index.dtype:
        raise ValueError(f"new_vectors is {new_vectors.dtype}, the index holds "
                         f"{index.dtype}")
    if new_vectors.device != index.device:
        raise ValueError("new_vectors must be on the device of the index")
    dev = index.device
    m = new_vectors.shape[0]
    if new_indices is None:
        new_indices = torch.arange(index.n_rows, index.n_rows + m, device=dev)
    elif new_indices.dim() != 1 or new_indices.shape[0] != m:
        raise ValueError(f"new_indices must be an integer tensor [{m}]")
    new_indices = new_indices.to(dev, torch.int64)
    if m:
        labels = kmeans_predict(index.centroids, new_vectors.float(),
                                fp32_mode=index.fp32_mode).to(torch.int64)
    else:
        labels = torch.empty(0, dtype=torch.int64, device=dev)
    total = index.indices.numel()
    if total:
        keep = (index.indices >= 0).nonzero().flatten()
        slot_list = torch.searchsorted(index.list_offsets[1:].contiguous(), keep,
                                       right=True)
        rows = torch.cat([index._padded_rows()[keep], new_vectors])
        ids = torch.cat([index.indices[keep], new_indices])
        labels = torch.cat([slot_list, labels])   # stable sort: old rows first
    else:
        rows, ids = new_vectors, new_indices
    offsets, sizes, data, indices = _pack(rows, ids, labels, index.n_lists, index.dim)
    return IvfFlatIndex(index.centroids, offsets, sizes, data, indices, index.metric,
                        index.dim, index.n_rows + m, index.fp32_mode)


def _filter_parts(filter, dev):
    """(packed int32 words, n_bits, dense bool) of a Bitset / bool mask."""
    if isinstance(filter, Bitset):
        words = filter.words.to(dev).contiguous()
        return words, filter.n_bits, None
    if isinstance(filter, torch.Tensor) and filter.dtype == torch.bool and filter.dim() == 1:
        return None, filter.numel(), filter.to(dev)
    raise ValueError("filter must be a core.Bitset or a 1-D torch.bool tensor over "
                     "dataset ids")


def _chunk_layout(index, probes):
    """Ragged candidate layout of one query chunk: row_off int64 [qc + 1] and
    pair_off int64 [qc, n_probes], the offset of every probed list's padded
    rows (probe order)."""
    padded = index.list_offsets[1:] - index.list_offsets[:-1]
    plen = padded[probes]
    ends = plen.cumsum(1)
    row_off = torch.zeros(probes.shape[0] + 1, dtype=torch.int64, device=probes.device)
    row_off[1:] = ends[:, -1].cumsum(0)
    return row_off, row_off[:-1, None] + (ends - plen)


def _scan_kernel(index, q32, probes, pair_off, cand, fwords, fbits, qg):
    """List-major scan of one query chunk on the GPU (no host sync)."""
    ext = require_ext()
    dev = q32.device
    qc, n_probes = probes.shape
    n_pairs = qc * n_probes
    n_lists = index.n_lists
    flat = probes.reshape(-1)
    _, order = torch.sort(flat, stable=True)
    pair_query = order // n_probes
    pair_out_off = pair_off.reshape(-1)[order].contiguous()
    cnt = torch.bincount(flat, minlength=n_lists)
    groups = (cnt + (qg - 1)) // qg
    gend = groups.cumsum(0)
    # the host knows only the bound; blocks past n_items exit
    max_items = -(-n_pairs // qg) + min(n_lists, n_pairs)
    i = torch.arange(max_items, device=dev)
    il = torch.searchsorted(gend, i, right=True).clamp_(max=n_lists - 1)
    j = i - (gend - groups)[il]
    begin = (cnt.cumsum(0) - cnt)[il] + j * qg
    count = (cnt[il] - j * qg).clamp_(max=qg)
    y_split = max(1, min(-(-_TARGET_BLOCKS // max_items), index.max_list_pad // _GROUP))
    ext.ivf_flat_scan(index.data, index.list_offsets, index.indices, q32, il, begin,
                      count, gend[-1:].contiguous(), pair_query, pair_out_off, fwords,
                      fbits, cand, _METRIC_CODES[index.metric], qg, y_split)


def _scan_torch(index, q32, probes, pair_off, cand, fdense, bad):
    """The same candidate buffer with torch ops over unpack_list."""
    dev = q32.device
    cand.fill_(bad)
    ip = index.metric == DistanceType.InnerProduct
    for l in torch.unique(probes).tolist():
        rows, ids = index.unpack_list(l)
        size = rows.shape[0]
        if size == 0:
            continue
        x = rows.float()
        ok = None
        if fdense is not None:
            ok = (ids < fdense.numel()) & fdense[ids.clamp(max=fdense.numel() - 1)]
        qi, pi = (probes == l).nonzero(as_tuple=True)
        cols = torch.arange(size, device=dev)
        sub = max(1, (1 << 22) // (size * index.dim))
        for s0, s1 in row_chunks(qi.numel(), sub):
            qv = q32[qi[s0:s1]]
            if ip:
                dist = (x.unsqueeze(0) * qv.unsqueeze(1)).sum(dim=2)
            else:
                diff = x.unsqueeze(0) - qv.unsqueeze(1)
                dist = (diff * diff).sum(dim=2)
                if index.metric == DistanceType.L2SqrtExpanded:
                    dist = dist.sqrt()
            if ok is not None:
                dist = torch.where(ok.unsqueeze(0), dist, torch.full_like(dist, bad))
            cand[pair_off[qi[s0:s1], pi[s0:s1]].unsqueeze(1) + cols] = dist


def _select(cand, row_off, k, select_min, bad):
    """Per ragged row the k best (value, position); (bad, -1) past the row.
    GPU: the generic ragged-row select engine; CPU: a dense torch.topk."""
    if cand.is_cuda:
        return require_ext().select_k_generic(cand, row_off, k=k, select_min=select_min)
    lens = row_off[1:] - row_off[:-1]
    qc = lens.numel()
    vals = torch.full((qc, k), bad, dtype=cand.dtype, device=cand.device)
    pos = torch.full((qc, k), -1, dtype=torch.int64, device=cand.device)
    maxlen = int(lens.max()) if qc else 0
    if maxlen == 0:
        return vals, pos
    ar = torch.arange(maxlen, device=cand.device)
    at = (row_off[:-1, None] + ar).clamp_(max=cand.numel() - 1)
    dense = torch.where(ar < lens[:, None], cand[at], torch.full_like(cand[:1], bad))
    kk = min(k, maxlen)
    v, p = torch.topk(dense, kk, dim=1, largest=not select_min)
    vals[:, :kk] = v
    pos[:, :kk] = torch.where(p < lens[:, None], p, torch.full_like(p, -1))
    return vals, pos


def _finish(index, vals, pos, probes, row_off, pair_off, select_min, bad):
    """Within-row positions -> (probe, row in list) -> dataset ids; rows sorted
    best first (equal distances by id), missing slots (bad, -1) last."""
    rel = (pair_off - row_off[:-1, None]).contiguous()
    p = pos.clamp_min(0)
    pr = (torch.searchsorted(rel, p, right=True) - 1).clamp_(min=0)
    slot = index.list_offsets[probes.gather(1, pr)] + (p - rel.gather(1, pr))
    ids = index.indices[slot.clamp_(max=index.indices.numel() - 1)]
    missing = (pos < 0) | (vals == bad) | (ids < 0)
    ids = torch.where(missing, torch.full_like(ids, -1), ids)
    vals = torch.where(missing, torch.full_like(vals, bad), vals)
    o = torch.argsort(ids, dim=1, stable=True)
    vals, ids = vals.gather(1, o), ids.gather(1, o)
    o = torch.argsort(vals, dim=1, descending=not select_min, stable=True)
    return vals.gather(1, o), ids.gather(1, o)


def ivf_flat_search(index: IvfFlatIndex, queries: torch.Tensor, k: int,
                    n_probes: int = 20, *, filter=None, return_probes: bool = False,
                    res=None, probes: torch.Tensor | None = None, qg: int | None = None):
    """k nearest indexed rows among the n_probes best lists of every query
    (reference ivf_flat::search).

    Returns (dists [q, k] fp32, ids [q, k] int64), best first, plus the probed
    lists [q, n_probes] int64 with return_probes=True. InnerProduct returns
    the LARGEST products. A query whose probed lists hold fewer than k
    admissible rows gets +inf (-inf for InnerProduct) and id -1 in the missing
    slots. n_probes is clamped to n_lists.

    filter: a core.Bitset or a torch.bool [>= max id + 1] over dataset ids; a
    row whose bit is clear is never returned.
    probes: int64 [q, n_probes] lists to scan instead of the coarse step.
    qg: queries one scan block stages (4, 8, 16 or 32; default 8, lowered to
    what 64 KiB of LDS holds: at most 16 at d = 1024, 8 at 2048, 4 at 4096).

    The coarse step is pairwise_distance(queries, centroids) in the index
    metric and the index's fp32_mode, then select_k. Queries are taken in
    chunks whose candidate buffer fits half of res.workspace_budget(). L2
    distances are the unexpanded fp32 sum: within (d + 3) * 2^-24 relative of
    the exact value. GPU indices with d_pad > 4096 or fp32_mode="native", and
    CPU tensors, run the scan with torch ops instead of the list-scan kernel.
    """
    from raft_amd.core.resources import get_resources
    k = int(k)
    if k <= 0:
        raise ValueError(f"k must be positive, got {k}")
    if queries.dim() != 2 or queries.shape[1] != index.dim:
        raise ValueError(f"queries must be [q, {index.dim}], got {tuple(queries.shape)}")
    if queries.device != index.device:
        raise ValueError("queries must be on the device of the index")
    dev = index.device
    ext = require_ext() if dev.type == "cuda" else None
    q32 = queries.float().contiguous()
    q = q32.shape[0]
    ip = index.metric == DistanceType.InnerProduct
    select_min = not ip
    bad = float("-inf") if ip else float("inf")

    if probes is None:
        n_probes = int(n_probes)
        if n_probes <= 0:
            raise ValueError(f"n_probes must be positive, got {n_probes}")
        n_probes = min(n_probes, index.n_lists)
        coarse = pairwise_distance(q32, index.centroids, metric=index.metric,
                                   fp32_mode=index.fp32_mode)
        probes = select_k(coarse, n_probes, select_min=select_min)[1]
    elif (probes.dim() != 2 or probes.shape[0] != q or probes.shape[1] < 1
          or probes.dtype != torch.int64):
        raise ValueError("probes must be int64 [q, n_probes]")
    probes = probes.to(dev).contiguous()
    n_probes = probes.shape[1]

    fwords = fdense = None
    fbits = 0
    if filter is not None:
        fwords, fbits, fdense = _filter_parts(filter, dev)

    dists = torch.full((q, k), bad, dtype=torch.float32, device=dev)
    ids = torch.full((q, k), -1, dtype=torch.int64, device=dev)
    if q == 0 or index.indices.numel() == 0:
        return (dists, ids, probes) if return_probes else (dists, ids)

    use_kernel = (dev.type == "cuda" and index.d_pad <= _MAX_KERNEL_D_PAD
                  and index.fp32_mode != "native")
    if use_kernel:
        qg = _DEFAULT_QG if qg is None else int(qg)
        if qg not in _QG_CHOICES:
            raise ValueError(f"qg must be one of {_QG_CHOICES}, got {qg}")
        qg = min(qg, ext.ivf_flat_scan_max_qg(index.d_pad))
        if fdense is not None:
            fwords = Bitset.from_dense(fdense).words.contiguous()
    elif fwords is not None:
        fdense = Bitset(fbits, words=fwords).to_dense()

    res = get_resources(res if res is not None else dev)
    per_query = 4 * n_probes * index.max_list_pad
    q_chunk = int(max(1, min(q, (res.workspace_budget() // 2) // per_query)))
    ws = res.get_workspace((q_chunk * n_probes * index.max_list_pad,), torch.float32)
    try:
        for s0, s1 in row_chunks(q, q_chunk):
            pc = probes[s0:s1]
            cand = ws.view(((s1 - s0) * n_probes * index.max_list_pad,), torch.float32)
            row_off, pair_off = _chunk_layout(index, pc)
            if use_kernel:
                _scan_kernel(index, q32[s0:s1], pc, pair_off, cand, fwords, fbits, qg)
            else:
                _scan_torch(index, q32[s0:s1], pc, pair_off, cand, fdense, bad)
            vals, pos = _select(cand, row_off, k, select_min, bad)
            dists[s0:s1], ids[s0:s1] = _finish(index, vals, pos, pc, row_off, pair_off,
                                               select_min, bad)
    finally:
        ws.free()
    return (dists, ids, probes) if return_probes else (dists, ids)


def ivf_flat_save(index: IvfFlatIndex, path: str) -> None:
    """Write the index to one file (reference ivf_flat::serialize): a header
    (magic, version, metric, dim, n_rows, dtype, n_lists, fp32_mode), then
    centroids, list_offsets, list_sizes, data and indices as .npy records.
    bf16 data is stored as its 16-bit patterns."""
    data = index.data
    if data.dtype == torch.bfloat16:
        data = data.view(torch.int16)
    with open(path, "wb") as f:
        f.write(struct.pack(_HEADER, _MAGIC, _VERSION, _METRIC_CODES[index.metric],
                            index.dim, index.n_rows, _DTYPE_CODES[index.dtype],
                            index.n_lists, index.fp32_mode.encode("ascii")))
        for t in (index.centroids, index.list_offsets, index.list_sizes, data,
                  index.indices):
            serialize_mdspan(f, t)


def ivf_flat_load(path: str, device=None) -> IvfFlatIndex:
    """Read an index written by ivf_flat_save onto device (default: CPU)."""
    with open(path, "rb") as f:
        raw = f.read(struct.calcsize(_HEADER))
        if len(raw) != struct.calcsize(_HEADER):
            raise ValueError(f"{path} is not an IVF-Flat index file")
        magic, version, metric, dim, n_rows, dtype, n_lists, mode = struct.unpack(
            _HEADER, raw)
        if magic != _MAGIC:
            raise ValueError(f"{path} is not an IVF-Flat index file")
        if version != _VERSION:
            raise ValueError(f"{path}: unsupported IVF-Flat file version {version}")
        centroids, offsets, sizes, data, indices = (
            deserialize_mdspan(f, device=device) for _ in range(5))
    metrics = {c: m for m, c in _METRIC_CODES.items()}
    dtypes = {c: t for t, c in _DTYPE_CODES.items()}
    if metric not in metrics or dtype not in dtypes or centroids.shape[0] != n_lists:
        raise ValueError(f"{path}: corrupt IVF-Flat header")
    if dtypes[dtype] == torch.bfloat16:
        data = data.view(torch.bfloat16)
    return IvfFlatIndex(centroids, offsets, sizes, data, indices, metrics[metric], dim,
                        n_rows, mode.rstrip(b"\x00").decode("ascii"))
