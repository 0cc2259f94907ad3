"""Epsilon-neighborhood (fixed-radius neighbors) under squared L2.

Reference parity: the historical raft::neighbors epsilon_neighborhood /
eps_neighbors_l2sq — a boolean adjacency `adj[i, j] = (||x_i - y_j||^2 <=
eps_sq)` plus vertex degrees `vd` (vd[m] holds the total), the primitive under
DBSCAN and radius graphs.

MI355X design — the fp32 distance tile never reaches HBM:
  1. One sweep of the split-bf16 MFMA tile engine (csrc/eps_neighbors.hip)
     decides every pair on the matrix cores and writes a PACKED bitmap
     (1/8 B per pair) with wave ballots; no atomics on the bitmap.
  2. fp32 inputs are VERIFIED: a pair whose emulated distance lies within the
     provable emulation bound of eps_sq is re-decided by the exact fp32
     unexpanded sum (x - y)^2, inside the same kernel. Every other pair is
     farther from eps_sq than the emulation can move it
     (docs/verified_engines.md, "Eps-neighborhood exactness").
  3. Degrees are integer popcounts of the bitmap rows; CSR column ids come
     from a native bitmap-rows -> CSR fill (count -> scan -> fill), never from
     a dense matrix; the bool adjacency is a coalesced expand of the bitmap.

Rows are processed in chunks; the only scratch is the packed bitmap of one
row chunk, taken from the Resources workspace so limits and tracking apply.
Every pair is decided independently of its tile, so results do not depend on
the chunking.
"""
from __future__ import annotations

import math

import torch

from raft_amd._ext import require_ext
from raft_amd.utils import row_chunks
from raft_amd.linalg.split_bf16 import (MODE_NSLICE, SPLIT_BOUND, pad_features,
                                        row_sqnorms, split_bf16_slices)

_FP32_MODES = ("auto", "bf16x1v", "bf16x2v", "native")
#: the verified engine "auto" resolves to (see docs/performance.md,
#: "Eps-neighborhood", for the measurement behind the choice)
_AUTO_MODE = "bf16x2v"

_BIT_VALUES = [1 << k for k in range(31)] + [-(1 << 31)]


def _bit_table(device) -> torch.Tensor:
    return torch.tensor(_BIT_VALUES, dtype=torch.int32, device=device)


def _pack_rows(adj: torch.Tensor) -> torch.Tensor:
    """bool [r, n] -> int32 [r, ceil(n/32)] words (core/bitset.py layout,
    every row on a word boundary, tail bits zero)."""
    r, n = adj.shape
    n_words = (n + 31) // 32
    pad = n_words * 32 - n
    if pad:
        adj = torch.nn.functional.pad(adj, (0, pad))
    bits = adj.reshape(r, n_words, 32).to(torch.int32)
    # distinct bits: the sum is the OR and cannot overflow int32 in any order
    return (bits * _bit_table(adj.device)).sum(dim=2, dtype=torch.int32)


def _unpack_rows(bitmap: torch.Tensor, n: int) -> torch.Tensor:
    """int32 [r, ceil(n/32)] words -> bool [r, n]."""
    r = bitmap.shape[0]
    shifts = torch.arange(32, dtype=torch.int32, device=bitmap.device)
    bits = (bitmap.unsqueeze(2) >> shifts) & 1
    return bits.to(torch.bool).reshape(r, -1)[:, :n]


def _row_degrees(bitmap: torch.Tensor, n: int, out: torch.Tensor) -> None:
    if bitmap.is_cuda:
        require_ext().bitmap_row_degrees(bitmap, out)
    else:
        out.copy_(_unpack_rows(bitmap, n).sum(dim=1))


def _rows_to_csr(bitmap: torch.Tensor, n: int, deg: torch.Tensor):
    """Sorted int32 column ids of one bitmap row block. Returns indices [nnz]."""
    indptr = torch.zeros(bitmap.shape[0] + 1, dtype=torch.int64,
                         device=bitmap.device)
    torch.cumsum(deg, dim=0, out=indptr[1:])
    nnz = int(indptr[-1].item())
    if bitmap.is_cuda:
        indices = torch.empty(nnz, dtype=torch.int32, device=bitmap.device)
        require_ext().bitmap_rows_to_csr(bitmap, indptr, indices)
        return indices
    # oracle path: row-major nonzero of the block is already sorted per row
    return _unpack_rows(bitmap, n).nonzero()[:, 1].to(torch.int32)


def _check_inputs(x, y, eps_sq, fp32_mode):
    if eps_sq is None:
        raise TypeError("eps_sq (the squared radius) is required")
    if fp32_mode not in _FP32_MODES:
        raise ValueError(f"fp32_mode must be one of {_FP32_MODES}, got {fp32_mode!r}")
    self_join = y is None
    if self_join:
        y = x
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError("x and y must be 2-D [rows, features]")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"feature dimension mismatch: x has {x.shape[1]}, "
                         f"y has {y.shape[1]}")
    if x.dtype != y.dtype or x.device != y.device:
        raise ValueError("x and y must share dtype and device")
    if not x.dtype.is_floating_point:
        raise ValueError("x and y must be floating point")
    if y.shape[0] >= 2 ** 31 or x.shape[0] >= 2 ** 31:
        raise ValueError("eps-neighborhood needs m, n < 2^31")
    return y, self_join


def _cpu_filler(x, y, eps):
    """Oracle path: row-chunked sum of squared differences in the input dtype
    (16-bit floats widen to fp32, which is exact, as on the GPU)."""
    if x.dtype in (torch.float16, torch.bfloat16):
        x, y = x.float(), y.float()
    n, d = y.shape
    sub = max(1, (1 << 22) // max(n * d, 1))

    def fill(s0, s1, bm):
        for r0, r1 in row_chunks(s1 - s0, sub):
            diff = x[s0 + r0:s0 + r1].unsqueeze(1) - y.unsqueeze(0)
            d2 = (diff * diff).sum(dim=2)
            bm[r0:r1] = _pack_rows(d2 <= eps)
    return fill


def _native_filler(x, y, eps):
    """Exact tiled fallback: chunked pairwise_distance tiles, compared and
    packed. Used by fp32_mode="native" and by GPU dtypes the MFMA path does
    not take (fp64)."""
    from raft_amd.distance import pairwise_distance, DistanceType
    n = y.shape[0]
    sub = max(1, (1 << 26) // max(n, 1))

    def fill(s0, s1, bm):
        for r0, r1 in row_chunks(s1 - s0, sub):
            d2 = pairwise_distance(x[s0 + r0:s0 + r1], y,
                                   metric=DistanceType.L2Expanded,
                                   fp32_mode="native")
            bm[r0:r1] = _pack_rows(d2 <= eps)
    return fill


def _mfma_filler(x, y, eps, mode, self_join, counter):
    """The MFMA bitmap engine. fp32: verified (band pairs rechecked in exact
    fp32, counted into `counter`); bf16: one slice, exact in its own dtype."""
    ext = require_ext()
    x = x.contiguous()
    y = x if self_join else y.contiguous()
    n = y.shape[0]
    # the slices carry zero-padded features (no distance changes); the norms
    # and the exact recheck read the rows as given
    if x.dtype == torch.bfloat16:
        nsl, xf, yf, cnt = 1, None, None, None
        xs = [pad_features(x).contiguous()]
        ys = xs if self_join else [pad_features(y).contiguous()]
    else:
        nsl, xf, yf, cnt = MODE_NSLICE[mode], x, y, counter
        xs = split_bf16_slices(pad_features(x), nsl)
        ys = xs if self_join else split_bf16_slices(pad_features(y), nsl)
    lead, tail = SPLIT_BOUND[nsl]
    xn = row_sqnorms(x)
    yn = xn if self_join else row_sqnorms(y)

    def fill(s0, s1, bm):
        ext.eps_neighbors_l2sq([t[s0:s1] for t in xs], ys, xn[s0:s1], yn,
                               None if xf is None else xf[s0:s1], yf, bm, cnt,
                               n, eps, lead, tail)
    return fill


def _sweep(x, y, eps_sq, fp32_mode, row_chunk, res, dest, sink):
    """Fill the packed bitmap row chunk by row chunk and hand each chunk to
    sink(s0, s1, bitmap_chunk). dest: optional [m, words] tensor to fill in
    place (no workspace is taken then). Returns the recheck counter value."""
    from raft_amd.core.resources import get_resources
    y, self_join = _check_inputs(x, y, eps_sq, fp32_mode)
    if x.is_cuda and x.dtype == torch.float16:
        # fp16 -> fp32 is exact: ride the verified fp32 engine, as knn does
        x = x.float()
        y = x if self_join else y.float()
    m, n = x.shape[0], y.shape[0]
    n_words = (n + 31) // 32
    if m == 0:
        return 0
    res = get_resources(res if res is not None else x.device)
    dev = x.device

    eps = float(eps_sq)
    if x.dtype != torch.float64:
        # the comparison runs in fp32: round the threshold once, here
        eps = float(torch.tensor(eps, dtype=torch.float32))
    counter = None
    if not (eps >= 0) or n == 0:
        fill = lambda s0, s1, bm: bm.zero_()                  # noqa: E731
    elif math.isinf(eps):
        full_row = _pack_rows(torch.ones((1, n), dtype=torch.bool, device=dev))
        fill = lambda s0, s1, bm: bm.copy_(full_row.expand_as(bm))  # noqa: E731
    elif not x.is_cuda:
        fill = _cpu_filler(x, y, eps)
    elif x.dtype == torch.bfloat16 or (x.dtype == torch.float32
                                       and fp32_mode != "native"):
        mode = _AUTO_MODE if fp32_mode == "auto" else fp32_mode
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        fill = _mfma_filler(x, y, eps, mode, self_join, counter)
    else:
        require_ext()
        fill = _native_filler(x, y, eps)
    set_diag = self_join and eps >= 0 and n > 0

    if row_chunk is None:
        if dest is not None:
            row_chunk = m
        else:
            # same policy as brute_force._tiles_from_budget: the dominant
            # scratch (here the chunk bitmap) stays under half the budget
            row_chunk = (res.workspace_budget() // 2) // max(4 * n_words, 1)
            if row_chunk >= 128:
                row_chunk -= row_chunk % 128
    row_chunk = int(max(1, min(int(row_chunk), m)))

    ws = None
    if dest is None:
        ws = res.get_workspace((row_chunk, n_words), torch.int32)
    try:
        for s0, s1 in row_chunks(m, row_chunk):
            bm = (dest[s0:s1] if dest is not None
                  else ws.view((s1 - s0, n_words), torch.int32))
            fill(s0, s1, bm)
            if set_diag:
                # a point is its own neighbor whatever the expanded form
                # rounds to
                r = torch.arange(s0, s1, device=dev)
                loc = torch.arange(s1 - s0, device=dev)
                bm[loc, r >> 5] |= _bit_table(dev)[r & 31]
            sink(s0, s1, bm)
    finally:
        if ws is not None:
            ws.free()
    return int(counter.item()) if counter is not None else 0


def eps_neighbors_l2sq(x: torch.Tensor, y: torch.Tensor | None = None,
                       eps_sq: float | None = None, *, packed: bool = False,
                       fp32_mode: str = "auto", row_chunk: int | None = None,
                       return_stats: bool = False, res=None):
    """Rows of y [n,d] within squared radius eps_sq of each row of x [m,d].

    Returns (adj, vd) or (adj, vd, stats). adj[i,j] = (||x_i - y_j||^2 <=
    eps_sq), ties included: bool [m,n], or with packed=True int32
    [m, ceil(n/32)] words (core.Bitset bit order, each row on a word boundary,
    tail bits zero). vd is int64 [m+1]: row degrees, vd[m] the total.
    y=None means y = x and always sets the diagonal for eps_sq >= 0.
    eps_sq < 0 gives an empty result, eps_sq = inf a full one.

    fp32_mode (fp32/fp16 GPU inputs): "bf16x1v" / "bf16x2v" run the verified
    MFMA engine with 1 or 2 bf16 slices (pairs inside the emulation bound
    around eps_sq are re-decided in exact fp32), "native" an exact tiled
    fallback, "auto" the faster verified engine. bf16 inputs use one slice,
    exact in their own dtype. Any d is zero-padded to a multiple of 64.
    CPU tensors take a pure-PyTorch path. stats = {"rechecked": pairs that
    took the exact recheck}.
    """
    m = x.shape[0]
    n = (x if y is None else y).shape[0]
    dev = x.device
    vd = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    if packed:
        adj = torch.empty((m, (n + 31) // 32), dtype=torch.int32, device=dev)
    else:
        adj = torch.empty((m, n), dtype=torch.bool, device=dev)

    def sink(s0, s1, bm):
        _row_degrees(bm, n, vd[s0:s1])
        if packed:
            return
        if bm.is_cuda:
            require_ext().bitmap_rows_expand(bm, adj[s0:s1])
        else:
            adj[s0:s1] = _unpack_rows(bm, n)

    rechecked = _sweep(x, y, eps_sq, fp32_mode, row_chunk, res,
                       adj if packed else None, sink)
    vd[m] = vd[:m].sum()
    if return_stats:
        return adj, vd, {"rechecked": rechecked}
    return adj, vd


def eps_neighbors_l2sq_csr(x: torch.Tensor, y: torch.Tensor | None = None,
                           eps_sq: float | None = None, *,
                           fp32_mode: str = "auto", row_chunk: int | None = None,
                           res=None):
    """CSR form of eps_neighbors_l2sq. Returns (indptr int64 [m+1], indices
    int32 [nnz] strictly increasing within each row, vd int64 [m+1]).

    Never allocates m*n bytes: the scratch is the packed bitmap of one row
    chunk (row_chunk defaults to the largest chunk whose bitmap fits half of
    res.workspace_budget()), turned into column ids by a native
    count -> scan -> fill over the bitmap rows.
    """
    m = x.shape[0]
    n = (x if y is None else y).shape[0]
    dev = x.device
    vd = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    parts = []

    def sink(s0, s1, bm):
        _row_degrees(bm, n, vd[s0:s1])
        parts.append(_rows_to_csr(bm, n, vd[s0:s1]))

    _sweep(x, y, eps_sq, fp32_mode, row_chunk, res, None, sink)
    vd[m] = vd[:m].sum()
    indptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    torch.cumsum(vd[:m], dim=0, out=indptr[1:])
    if len(parts) == 1:
        indices = parts[0]
    elif parts:
        indices = torch.cat(parts)
    else:
        indices = torch.empty(0, dtype=torch.int32, device=dev)
    return indptr, indices, vd
