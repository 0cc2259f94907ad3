"""IVF-PQ: an inverted-file index over product-quantised residuals.

Reference parity: the historical raft::neighbors::ivf_pq::{build, extend,
search, serialize} with per-subspace codebooks and pq_bits = 8 or 4. The data
set is partitioned like IVF-Flat; a row is stored as pq_dim codes: its residual
to the list centroid is cut into pq_dim sub-vectors of pq_len = ceil(d / pq_dim)
features (d_rot = pq_dim * pq_len, features past d are zero) and every
sub-vector is replaced by the number of its nearest entry among the book_size =
2^pq_bits (256 or 16) of that subspace's codebook. A row costs pq_dim bytes (half
that with 4-bit codes) instead of 4 * d, and a search scores it with pq_dim
table look-ups instead of d FMAs.

Distances are ASYMMETRIC (ADC): from the exact query to the RECONSTRUCTED row
centroid + decoded residual, not to the original vector. ivf_pq_search(...,
dataset=x, refine_ratio=r) re-ranks k * r such candidates against the original
vectors with neighbors.refine and returns exact distances.

Storage is the IVF-Flat layout (neighbors/ivf_flat.py) with uint8 elements: a
stored row is row_bytes bytes, lists are padded to 64 rows, byte (group g,
chunk j, row r, b) at

    ((g * (row_bytes / 16) + j) * 64 + r) * 16 + b.

8-bit codes: byte t of a row is the code of subspace t; row_bytes = pq_dim_pad =
pq_dim rounded up to 16 with zero pad bytes, 16 subspaces per 16-byte chunk.
4-bit codes: byte t of a row holds subspace 2t in bits 0..3 and subspace 2t + 1
in bits 4..7; the pad nibble of an odd pq_dim is 0; row_bytes = ceil(pq_dim / 2)
rounded up to 16 with zero pad bytes, 32 subspaces per chunk.

Codebooks are fp32 [pq_dim, pq_len, book_size], entry-minor, which the kernels
read coalesced. unpack_list returns one code per byte for either width.

MI355X design (csrc/ivf_pq.hip): ivf_pq_encode forms the residual sub-vector in
registers and walks a subspace's codebook staged in LDS; ivf_pq_scan is
PAIR-major: one block per (query, probe) pair builds the pair's full fp32
look-up table in LDS (up to 128 KiB of CDNA4's 160 KiB) and gathers from it
with lane = row. Candidates go to the ragged buffer of IVF-Flat and the same
select and id mapping finish the search. 4-bit codes have kernels of their own
(csrc/ivf_pq4.hip): a 16-entry table row is 64 bytes, so ivf_pq4_scan is
LIST-major like the flat scan: a block holds the tables of up to 8 queries
that probe one list (within 64 KiB of LDS) and reads the list's codes once for
all of them; ivf_pq4_encode writes one packed 16-byte chunk per thread.

CPU tensors run the same algorithm in plain torch (a cdist argmin per subspace
to encode, table plus gather to scan). A GPU index with pq_len > 32, or with
pq_dim > 128 (8-bit) or pq_dim > 256 (4-bit), takes that torch path on the GPU
(the select is still native). A GPU call without the native extension raises.
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

from .ivf_flat import (_GROUP, _METRIC_CODES, _TARGET_BLOCKS, _check_vectors, _chunk_layout,
                       _filter_parts, _finish, _pack, _resolve_metric, _scan_items, _select)

_BOOKS = {8: 256, 4: 16}    # pq_bits -> entries of one codebook
_CHUNK = 16                 # bytes in one chunk
#: the shapes csrc/ivf_pq.hip serves: a 128 KiB table, a 32-register residual
_MAX_KERNEL_PQ_DIM = 128
_MAX_KERNEL_PQ_LEN = 32
#: the shapes csrc/ivf_pq4.hip serves (and ext.ivf_pq4_scan_max_qg admits)
_MAX_KERNEL_PQ4_DIM = 256
_MAGIC = b"RAFTAMD_IVFPQ\x00\x00\x00"
_VERSION = 1                # 8-bit codes; a 4-bit index is written as version 2
_VERSION_PQ4 = 2
_HEADER = "<16s6q16s"


@dataclass
class IvfPqParams:
    """Build parameters (reference ivf_pq::index_params); the first seven are
    IvfFlatParams'. pq_dim: subspaces = codes per row, any value in [1, d];
    0 means ceil(d / 2) rounded up to a multiple of 16, capped at 128 and at d.
    pq_bits: 8 or 4, the bits of one code; a codebook has 2^pq_bits entries.
    Every codebook is one kmeans_fit of pq_kmeans_n_iters iterations on at
    most 2^pq_bits * max_train_points_per_pq_code residuals."""
    n_lists: int = 1024
    metric: DistanceType | str = "sqeuclidean"
    kmeans_n_iters: int = 20
    kmeans_trainset_fraction: float = 0.5
    add_data_on_build: bool = True
    seed: int = 0
    fp32_mode: str = "auto"
    pq_dim: int = 0
    pq_kmeans_n_iters: int = 25
    max_train_points_per_pq_code: int = 256
    pq_bits: int = 8


class IvfPqIndex:
    """The index: centroids [n_lists, d] fp32, codebooks [pq_dim, pq_len,
    book_size] fp32 (book_size 256: pq_bits 8; 16: pq_bits 4), list_offsets /
    list_sizes / indices as in IvfFlatIndex, codes (the flat interleaved uint8
    buffer, row_bytes per row), metric, dim, pq_dim, n_rows, fp32_mode."""

    def __init__(self, centroids, codebooks, list_offsets, list_sizes, codes, indices,
                 metric, dim, n_rows, fp32_mode="auto"):
        self.centroids = centroids
        self.codebooks = codebooks
        self.list_offsets = list_offsets
        self.list_sizes = list_sizes
        self.codes = codes
        self.indices = indices
        self.metric = _resolve_metric(metric)
        self.dim = int(dim)
        self.pq_dim = int(codebooks.shape[0])
        self.pq_len = int(codebooks.shape[1])
        self.book_size = int(codebooks.shape[2])
        self.pq_bits = _pq_bits_of(self.book_size)
        self.n_rows = int(n_rows)
        self.fp32_mode = fp32_mode
        padded = list_offsets[1:] - list_offsets[:-1]
        #: longest padded list, known on the host: sizes the candidate buffer
        self.max_list_pad = int(padded.max()) if padded.numel() else 0

    @property
    def n_lists(self) -> int:
        return self.centroids.shape[0]

    @property
    def device(self) -> torch.device:
        return self.centroids.device

    @property
    def d_rot(self) -> int:
        return self.pq_dim * self.pq_len

    @property
    def pq_dim_pad(self) -> int:
        return -(-self.pq_dim // _CHUNK) * _CHUNK

    @property
    def row_bytes(self) -> int:
        """Padded bytes of one stored row."""
        return _row_bytes(self.pq_dim, self.pq_bits)

    @property
    def kernels_serve(self) -> bool:
        """Whether csrc/ivf_pq.hip (8-bit) or csrc/ivf_pq4.hip (4-bit) encodes
        and scans this shape on the GPU."""
        if self.device.type != "cuda" or self.pq_len > _MAX_KERNEL_PQ_LEN:
            return False
        if self.pq_bits == 8:
            return self.pq_dim <= _MAX_KERNEL_PQ_DIM
        return (self.pq_dim <= _MAX_KERNEL_PQ4_DIM
                and require_ext().ivf_pq4_scan_max_qg(self.pq_dim, self.pq_len) >= 1)

    def to(self, device) -> "IvfPqIndex":
        return IvfPqIndex(self.centroids.to(device), self.codebooks.to(device),
                          self.list_offsets.to(device), self.list_sizes.to(device),
                          self.codes.to(device), self.indices.to(device), self.metric,
                          self.dim, self.n_rows, self.fp32_mode)

    def _padded_codes(self) -> torch.Tensor:
        """All padded rows' stored bytes [total, row_bytes] in slot order."""
        total = self.indices.numel()
        pp = self.row_bytes
        rows = self.codes.view(total // _GROUP, pp // _CHUNK, _GROUP, _CHUNK)
        return rows.permute(0, 2, 1, 3).reshape(total, pp)

    def unpack_list(self, l: int):
        """The codes [size, pq_dim] uint8 and dataset ids [size] of list l."""
        r0 = int(self.list_offsets[l])
        size = int(self.list_sizes[l])
        g = self.codes.view(-1, self.row_bytes // _CHUNK, _GROUP, _CHUNK)
        g = g[r0 // _GROUP:(r0 + size + _GROUP - 1) // _GROUP]
        rows = g.permute(0, 2, 1, 3).reshape(g.shape[0] * _GROUP, self.row_bytes)[:size]
        if self.pq_bits == 4:
            rows = torch.stack([rows & 15, rows >> 4], dim=2).reshape(size, 2 * self.row_bytes)
        return rows[:, :self.pq_dim].contiguous(), self.indices[r0:r0 + size]

    def reconstruct_list(self, l: int):
        """The reconstructed rows [size, d] fp32 (centroid + decoded residual)
        and dataset ids of list l: what a search measures distances to."""
        codes, ids = self.unpack_list(l)
        s = torch.arange(self.pq_dim, device=codes.device)
        dec = self.codebooks.permute(0, 2, 1)[s, codes.long()]   # [size, pq_dim, pq_len]
        rows = dec.reshape(codes.shape[0], self.d_rot)[:, :self.dim]
        return rows + self.centroids[l], ids


def _pq_bits_of(book_size: int) -> int:
    for bits, book in _BOOKS.items():
        if book == book_size:
            return bits
    raise ValueError(f"a codebook has 16 (pq_bits 4) or 256 (pq_bits 8) entries, got "
                     f"{book_size}")


def _row_bytes(pq_dim: int, pq_bits: int) -> int:
    return -(-(pq_dim * pq_bits) // (8 * _CHUNK)) * _CHUNK


def _default_pq_dim(d: int) -> int:
    half = -(-d // 2)
    return min(-(-half // _CHUNK) * _CHUNK, 128, d)


def _subspaces(v, pq_dim, pq_len):
    """[m, d] -> [m, pq_dim, pq_len], the features past d zero."""
    m, d = v.shape
    if pq_dim * pq_len != d:
        v = torch.cat([v, v.new_zeros((m, pq_dim * pq_len - d))], dim=1)
    return v.view(m, pq_dim, pq_len)


def _encode(x32, labels, centroids, codebooks, use_kernel):
    """The stored rows [n, row_bytes] uint8 (pad nibbles and bytes 0): per
    subspace the entry nearest to x - centroids[labels]; exact ties go to the
    smallest entry."""
    n = x32.shape[0]
    pq_dim, pq_len, book = codebooks.shape
    pq_bits = _pq_bits_of(book)
    row_bytes = _row_bytes(pq_dim, pq_bits)
    if use_kernel:
        codes = torch.empty((n, row_bytes), dtype=torch.uint8, device=x32.device)
        encode = require_ext().ivf_pq_encode if pq_bits == 8 else require_ext().ivf_pq4_encode
        encode(x32.contiguous(), labels.contiguous(), centroids, codebooks, codes)
        return codes
    # one code per byte, an even count, then two to a byte for 4-bit codes
    codes = torch.zeros((n, row_bytes * (8 // pq_bits)), dtype=torch.uint8, device=x32.device)
    books = codebooks.permute(0, 2, 1).contiguous()                # [pq_dim, book, pq_len]
    for s0, s1 in row_chunks(n, max(1, (1 << 24) // (book * pq_dim))):
        r = _subspaces(x32[s0:s1] - centroids[labels[s0:s1]], pq_dim, pq_len)
        dist = torch.cdist(r.permute(1, 0, 2).contiguous(), books,
                           compute_mode="donot_use_mm_for_euclid_dist")
        codes[s0:s1, :pq_dim] = dist.argmin(dim=2).t().to(torch.uint8)
    if pq_bits == 4:
        codes = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return codes


def _train_codebooks(x32, centroids, params, pq_dim, pq_len, book):
    """One kmeans_fit with book clusters per subspace on the residuals of a
    seeded sample (always L2 residuals, also for InnerProduct)."""
    from raft_amd.cluster.kmeans import KMeansParams, kmeans_fit, kmeans_predict
    n = x32.shape[0]
    n_train = min(n, book * int(params.max_train_points_per_pq_code))
    if n_train < book:
        raise ValueError(f"codebook training needs at least {book} rows, got {n_train}")
    if n_train < n:
        # drawn on the host so that a CPU and a GPU build train on the same rows
        pick = torch.randperm(n, generator=torch.Generator().manual_seed(params.seed))
        x32 = x32[pick[:n_train].to(x32.device)]
    labels = kmeans_predict(centroids, x32, fp32_mode=params.fp32_mode).to(torch.int64)
    res = _subspaces(x32 - centroids[labels], pq_dim, pq_len)
    books = torch.empty((pq_dim, pq_len, book), dtype=torch.float32, device=x32.device)
    for s in range(pq_dim):
        model = kmeans_fit(res[:, s].contiguous(),
                           KMeansParams(n_clusters=book, max_iter=params.pq_kmeans_n_iters,
                                        seed=params.seed + 7919 * (s + 1), init="random",
                                        fp32_mode=params.fp32_mode))
        books[s] = model.centroids.t()
    return books


def ivf_pq_build(x: torch.Tensor, params: IvfPqParams | None = None, *,
                 centroids: torch.Tensor | None = None,
                 codebooks: torch.Tensor | None = None, res=None) -> IvfPqIndex:
    """Build an IVF-PQ index over x [n, d] (reference ivf_pq::build).

    x is fp32, bf16 or fp16 and is widened to fp32. The coarse centroids are
    trained as in ivf_flat_build. The codebooks are trained on the residuals
    of a seeded sample of at most book_size * params.max_train_points_per_pq_code
    rows (book_size = 2^params.pq_bits, 256 or 16): per subspace one kmeans_fit
    with book_size clusters, seeded from params.seed and the subspace number,
    always on L2 residuals (also for InnerProduct). centroids= [n_lists, d] and
    codebooks= [pq_dim, pq_len, 256 or 16] skip the respective training;
    codebooks= overrides params.pq_dim and, by its last extent, params.pq_bits.
    params.add_data_on_build=False returns an index with empty lists.
    """
    from raft_amd.cluster.kmeans import kmeans_balanced_fit
    params = params if params is not None else IvfPqParams()
    metric = _resolve_metric(params.metric)
    if int(params.pq_bits) not in _BOOKS:
        raise ValueError(f"pq_bits must be 4 or 8, got {params.pq_bits}")
    book = _BOOKS[int(params.pq_bits)]
    if codebooks is not None and codebooks.dim() == 3:
        book = int(codebooks.shape[2])
        _pq_bits_of(book)
    x32 = _check_vectors(x, "x").float()
    n, d = x32.shape
    if d < 1:
        raise ValueError("x needs at least one feature")
    pq_dim = int(codebooks.shape[0]) if codebooks is not None and codebooks.dim() == 3 \
        else int(params.pq_dim) or _default_pq_dim(d)
    if pq_dim < 1 or pq_dim > d:
        raise ValueError(f"pq_dim must be in [1, {d}], got {pq_dim}")
    pq_len = -(-d // pq_dim)
    if centroids is None:
        n_lists = int(params.n_lists)
        if n_lists < 1 or n_lists > n:
            raise ValueError(f"n_lists must be in [1, {n}], got {n_lists}")
        centroids = kmeans_balanced_fit(x32, n_lists, max_iter=params.kmeans_n_iters,
                                        seed=params.seed,
                                        sample_fraction=params.kmeans_trainset_fraction,
                                        fp32_mode=params.fp32_mode).centroids
    elif centroids.dim() != 2 or centroids.shape[1] != d or centroids.shape[0] < 1:
        raise ValueError(f"centroids must be [n_lists, {d}]")
    dev = x32.device
    centroids = centroids.to(dev, torch.float32).contiguous()
    if codebooks is None:
        codebooks = _train_codebooks(x32, centroids, params, pq_dim, pq_len, book)
    elif tuple(codebooks.shape) != (pq_dim, pq_len, book):
        raise ValueError(f"codebooks must be [pq_dim, {pq_len}, 16 or 256] with pq_dim in "
                         f"[1, {d}], got {tuple(codebooks.shape)}")
    codebooks = codebooks.to(dev, torch.float32).contiguous()
    n_lists = centroids.shape[0]
    index = IvfPqIndex(
        centroids, codebooks, torch.zeros(n_lists + 1, dtype=torch.int64, device=dev),
        torch.zeros(n_lists, dtype=torch.int64, device=dev),
        torch.empty(0, dtype=torch.uint8, device=dev),
        torch.empty(0, dtype=torch.int64, device=dev), metric, d, 0, params.fp32_mode)
    if params.add_data_on_build:
        return ivf_pq_extend(index, x32, res=res)
    return index


def ivf_pq_extend(index: IvfPqIndex, new_vectors: torch.Tensor,
                  new_indices: torch.Tensor | None = None, *, res=None) -> IvfPqIndex:
    """Add rows to an index (reference ivf_pq::extend). Functional: returns a
    NEW index; centroids and codebooks are unchanged. The new rows are
    assigned with kmeans_predict and encoded, the old codes are kept as they
    are (never re-encoded) and the whole buffer is repacked. new_indices
    defaults to arange(n_rows, n_rows + m)."""
    from raft_amd.cluster.kmeans import kmeans_predict
    new32 = _check_vectors(new_vectors, "new_vectors").float()
    if new32.shape[1] != index.dim:
        raise ValueError(f"new_vectors has {new32.shape[1]} features, the index "
                         f"has {index.dim}")
    if new32.device != index.device:
        raise ValueError("new_vectors must be on the device of the index")
    dev = index.device
    m = new32.shape[0]
    if new_indices is None:
        new_indices = torch.arange(index.n_rows, index.n_rows + m, device=dev)
    elif new_indices.dim() != 1 or new_indices.shape[0] != m:
        raise ValueError(f"new_indices must be an integer tensor [{m}]")
    new_indices = new_indices.to(dev, torch.int64)
    if m:
        labels = kmeans_predict(index.centroids, new32,
                                fp32_mode=index.fp32_mode).to(torch.int64)
    else:
        labels = torch.empty(0, dtype=torch.int64, device=dev)
    codes = _encode(new32, labels, index.centroids, index.codebooks, index.kernels_serve)
    if index.indices.numel():
        keep = (index.indices >= 0).nonzero().flatten()
        slot_list = torch.searchsorted(index.list_offsets[1:].contiguous(), keep,
                                       right=True)
        codes = torch.cat([index._padded_codes()[keep], codes])
        new_indices = torch.cat([index.indices[keep], new_indices])
        labels = torch.cat([slot_list, labels])   # stable sort: old rows first
    offsets, sizes, data, indices = _pack(codes, new_indices, labels, index.n_lists,
                                          index.row_bytes)
    return IvfPqIndex(index.centroids, index.codebooks, offsets, sizes, data, indices,
                      index.metric, index.dim, index.n_rows + m, index.fp32_mode)


def _scan_kernel(index, q32, probes, pair_off, cand, fwords, fbits):
    """Pair-major LUT scan of one query chunk on the GPU (no host sync)."""
    n_pairs = probes.numel()
    # a block's four waves take one 64-row group each
    y_split = max(1, min(-(-_TARGET_BLOCKS // n_pairs),
                         -(-index.max_list_pad // (4 * _GROUP))))
    require_ext().ivf_pq_scan(index.codes, index.list_offsets, index.indices, q32,
                              index.centroids, index.codebooks, probes,
                              pair_off.contiguous(), fwords, fbits, cand,
                              _METRIC_CODES[index.metric], y_split)


def _scan_kernel4(index, q32, probes, pair_off, cand, fwords, fbits):
    """List-major LUT scan of one query chunk of a 4-bit index (no host sync):
    the work items of the flat scan, the group size from the LDS budget."""
    ext = require_ext()
    qg = ext.ivf_pq4_scan_max_qg(index.pq_dim, index.pq_len)
    il, begin, count, n_items, pair_query, pair_out_off = _scan_items(
        probes, pair_off, index.n_lists, qg)
    # a block's four waves take one 64-row group each
    y_split = max(1, min(-(-_TARGET_BLOCKS // il.numel()),
                         -(-index.max_list_pad // (4 * _GROUP))))
    ext.ivf_pq4_scan(index.codes, index.list_offsets, index.indices, q32, index.centroids,
                     index.codebooks, il, begin, count, n_items, pair_query, pair_out_off,
                     fwords, fbits, cand, _METRIC_CODES[index.metric], qg, y_split)


def _scan_torch(index, q32, probes, pair_off, cand, fdense, bad):
    """The same candidate buffer with torch ops: table, then gather."""
    dev = q32.device
    cand.fill_(bad)
    ip = index.metric == DistanceType.InnerProduct
    books = index.codebooks.unsqueeze(0)                   # [1, pq_dim, pq_len, book]
    for l in torch.unique(probes).tolist():
        codes, ids = index.unpack_list(l)
        size = codes.shape[0]
        if size == 0:
            continue
        at = codes.long().t().unsqueeze(0)                 # [1, pq_dim, size]
        ok = None
        if fdense is not None:
            ok = (ids < fdense.numel()) & fdense[ids.clamp(max=fdense.numel() - 1)]
        qi, pi = (probes == l).nonzero(as_tuple=True)
        cols = torch.arange(size, device=dev)
        c = index.centroids[l]
        sub = max(1, (1 << 22) // (index.book_size * index.d_rot + size * index.pq_dim))
        for s0, s1 in row_chunks(qi.numel(), sub):
            qv = q32[qi[s0:s1]]
            if ip:
                r = _subspaces(qv, index.pq_dim, index.pq_len).unsqueeze(3)
                lut = (r * books).sum(dim=2)               # [nq, pq_dim, book]
            else:
                r = _subspaces(qv - c, index.pq_dim, index.pq_len).unsqueeze(3)
                lut = ((r - books) ** 2).sum(dim=2)
            dist = lut.gather(2, at.expand(s1 - s0, -1, -1)).sum(dim=1)
            if ip:
                dist = dist + (qv * c).sum(dim=1, keepdim=True)
            elif index.metric == DistanceType.L2SqrtExpanded:
                dist = dist.sqrt()
            if ok is not None:
                dist = torch.where(ok.unsqueeze(0), dist, torch.full_like(dist, bad))
            cand[pair_off[qi[s0:s1], pi[s0:s1]].unsqueeze(1) + cols] = dist


def ivf_pq_search(index: IvfPqIndex, queries: torch.Tensor, k: int, n_probes: int = 20, *,
                  filter=None, return_probes: bool = False,
                  probes: torch.Tensor | None = None, res=None,
                  dataset: torch.Tensor | None = None, refine_ratio: int = 2):
    """k nearest indexed rows among the n_probes best lists of every query
    (reference ivf_pq::search).

    Returns (dists [q, k] fp32, ids [q, k] int64), best first, plus the probed
    lists [q, n_probes] int64 with return_probes=True. The distances are the
    asymmetric (ADC) distances from the query to the RECONSTRUCTED rows
    (IvfPqIndex.reconstruct_list), not to the original vectors. InnerProduct
    returns the LARGEST products. Missing slots hold +inf (-inf for
    InnerProduct) and id -1. n_probes is clamped to n_lists.

    dataset= [n, d] (fp32, bf16 or fp16; dataset[id] must be the vector that
    was indexed under id) re-ranks: the search runs with k * refine_ratio
    (refine_ratio >= 1), its ids, -1 slots included, go through
    refine(dataset, queries, ids, k, index.metric), and the call returns the
    EXACT distances to the original rows. With dataset=None refine_ratio is
    ignored and nothing changes.

    filter, probes, the coarse step and the query chunking (candidate buffer
    within half of res.workspace_budget(), results bitwise identical for any
    chunking) are those of ivf_flat_search. Squared L2 is the fp32 sum over
    subspaces of the unexpanded sums of ((q - c) - codebook entry)^2.
    """
    from raft_amd.core.resources import get_resources
    k = int(k)
    if k <= 0:
        raise ValueError(f"k must be positive, got {k}")
    if dataset is not None:
        from .refine import refine
        refine_ratio = int(refine_ratio)
        if refine_ratio < 1:
            raise ValueError(f"refine_ratio must be at least 1, got {refine_ratio}")
        out = ivf_pq_search(index, queries, k * refine_ratio, n_probes, filter=filter,
                            return_probes=True, probes=probes, res=res)
        dists, ids = refine(dataset, queries, out[1], k, index.metric)
        return (dists, ids, out[2]) if return_probes else (dists, ids)
    if queries.dim() != 2 or queries.shape[1] != index.dim:
        raise ValueError(f"queries must be [q, {index.dim}], got {tuple(queries.shape)}")
    if queries.device != index.device:
        raise ValueError("queries must be on the device of the index")
    dev = index.device
    if dev.type == "cuda":
        require_ext()
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

    use_kernel = index.kernels_serve
    if use_kernel and fdense is not None:
        fwords = Bitset.from_dense(fdense).words.contiguous()
    elif not use_kernel and fwords is not None:
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
                scan = _scan_kernel if index.pq_bits == 8 else _scan_kernel4
                scan(index, q32[s0:s1], pc, pair_off, cand, fwords, fbits)
            else:
                _scan_torch(index, q32[s0:s1], pc, pair_off, cand, fdense, bad)
            vals, pos = _select(cand, row_off, k, select_min, bad)
            dists[s0:s1], ids[s0:s1] = _finish(index, vals, pos, pc, row_off, pair_off,
                                               select_min, bad)
    finally:
        ws.free()
    return (dists, ids, probes) if return_probes else (dists, ids)


def ivf_pq_save(index: IvfPqIndex, path: str) -> None:
    """Write the index to one file (reference ivf_pq::serialize): a header
    (magic, version, metric, dim, n_rows, pq_dim, n_lists, fp32_mode), then
    centroids, codebooks, list_offsets, list_sizes, codes and indices as .npy
    records. An 8-bit index is version 1, a 4-bit index version 2; the book
    size is the codebooks' last extent."""
    with open(path, "wb") as f:
        version = _VERSION if index.pq_bits == 8 else _VERSION_PQ4
        f.write(struct.pack(_HEADER, _MAGIC, version, _METRIC_CODES[index.metric],
                            index.dim, index.n_rows, index.pq_dim, index.n_lists,
                            index.fp32_mode.encode("ascii")))
        for t in (index.centroids, index.codebooks, index.list_offsets, index.list_sizes,
                  index.codes, index.indices):
            serialize_mdspan(f, t)


def ivf_pq_load(path: str, device=None) -> IvfPqIndex:
    """Read an index written by ivf_pq_save onto device (default: CPU)."""
    with open(path, "rb") as f:
        raw = f.read(struct.calcsize(_HEADER))
        if len(raw) != struct.calcsize(_HEADER) or raw[:16] != _MAGIC:
            raise ValueError(f"{path} is not an IVF-PQ index file")
        _, version, metric, dim, n_rows, pq_dim, n_lists, mode = struct.unpack(_HEADER, raw)
        if version not in (_VERSION, _VERSION_PQ4):
            raise ValueError(f"{path}: unsupported IVF-PQ file version {version}")
        centroids, codebooks, offsets, sizes, codes, indices = (
            deserialize_mdspan(f, device=device) for _ in range(6))
    metrics = {c: m for m, c in _METRIC_CODES.items()}
    if (metric not in metrics or centroids.shape[0] != n_lists or codebooks.dim() != 3
            or codebooks.shape[0] != pq_dim or codebooks.shape[2] not in _BOOKS.values()
            or (version == _VERSION and codebooks.shape[2] != _BOOKS[8])):
        raise ValueError(f"{path}: corrupt IVF-PQ header")
    return IvfPqIndex(centroids, codebooks, offsets, sizes, codes, indices, metrics[metric],
                      dim, n_rows, mode.rstrip(b"\x00").decode("ascii"))
