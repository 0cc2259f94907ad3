"""Masked fused L2 nearest neighbor and the cross-component nearest pair.

Reference parity: the historical raft::distance::masked_l2_nn — for every row
of x the nearest row of y among the GROUPS of y a per-row mask allows — and
raft::sparse::neighbors::cross_component_nn / connect_components, which finds
for every connected component of a labelled point set the shortest edge to a
point outside it (the step that turns the spanning forest of a disconnected
kNN graph into a tree: HDBSCAN, single linkage, Euclidean MST).

MI355X design (csrc/masked_l2nn.hip): the 128x128 split-bf16 MFMA tile of the
fused L2-NN with the mask applied to the accumulator in registers — no fp32
distance tile reaches HBM — and a tile the mask excludes entirely skips its
K-loop (for component-sorted data those are the diagonal blocks). fp32 inputs
are VERIFIED: a row whose (best, second-best) margin over the allowed columns
is inside the provable emulation bound rescans its allowed columns with the
exact unexpanded fp32 sum; every other row recomputes its chosen distance
exactly (docs/verified_engines.md, "Masked L2-NN exactness").

The scratch that grows with the column count — the per-column-split partial
triples of one row chunk — comes from the Resources workspace; results do not
depend on the chunking.
"""
from __future__ import annotations

import torch

from raft_amd._ext import require_ext
from raft_amd.utils import row_chunks
from raft_amd.neighbors.epsilon_neighborhood import _pack_rows, _unpack_rows
from raft_amd.linalg.split_bf16 import (MODE_NSLICE, SPLIT_BOUND, pad_features,
                                        row_sqnorms, split_bf16_slices)

_FP32_MODES = ("auto", "bf16x1v", "bf16x2v", "native")
#: the verified engine "auto" resolves to (docs/performance.md, "Masked L2-NN")
_AUTO_MODE = "bf16x2v"
#: blocks one launch aims for (2 resident blocks on each of 256 CUs, twice
#: over) and the most column splits a row tile is cut into
_TARGET_BLOCKS = 1024
_MAX_SPLIT = 64
_INTS = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def _check_inputs(x, y, adj, group_idxs, x_group, fp32_mode):
    """Validate; returns (group_ends int64 CPU tensor [G], adj_is_packed)."""
    if fp32_mode not in _FP32_MODES:
        raise ValueError(f"fp32_mode must be one of {_FP32_MODES}, got {fp32_mode!r}")
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError("x and y must be 2-D [rows, features]")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"feature dimension mismatch: x has {x.shape[1]}, "
                         f"y has {y.shape[1]}")
    if x.dtype != y.dtype or x.device != y.device:
        raise ValueError("x and y must share dtype and device")
    if not x.dtype.is_floating_point:
        raise ValueError("x and y must be floating point")
    m, n = x.shape[0], y.shape[0]
    if m >= 2 ** 31 or n >= 2 ** 31 - 128:
        raise ValueError("masked_l2nn needs m, n < 2^31")
    if adj is None and x_group is None:
        raise ValueError("masked_l2nn needs adj, x_group or both")
    if group_idxs is None:
        raise ValueError("group_idxs (the group END offsets into y) is required")
    if group_idxs.dim() != 1 or group_idxs.dtype not in _INTS:
        raise ValueError("group_idxs must be a 1-D integer tensor")
    ends = group_idxs.detach().to("cpu", torch.int64)
    n_groups = ends.numel()
    if n_groups and (int(ends[0]) < 0 or bool((ends[1:] < ends[:-1]).any())):
        raise ValueError("group_idxs must be non-negative and non-decreasing")
    if (int(ends[-1]) if n_groups else 0) != n:
        raise ValueError(f"group_idxs[-1] must equal the number of y rows ({n})")
    packed = False
    if adj is not None:
        if adj.device != x.device:
            raise ValueError("adj must be on the device of x")
        if adj.dtype == torch.bool:
            want = (m, n_groups)
        elif adj.dtype == torch.int32:
            want, packed = (m, (n_groups + 31) // 32), True
        else:
            raise ValueError("adj must be bool [m, G] or packed int32 [m, ceil(G/32)]")
        if tuple(adj.shape) != want:
            raise ValueError(f"adj must have shape {want}, got {tuple(adj.shape)}")
    if x_group is not None:
        if (x_group.dim() != 1 or x_group.dtype not in _INTS
                or x_group.shape[0] != m or x_group.device != x.device):
            raise ValueError("x_group must be an integer tensor [m] on the device of x")
    return ends, packed


def _pick_min(d2, ok, key):
    """Row minimum of d2 over ok, exact ties to the smallest key (unique per
    column). Rows without an allowed column give (+inf, -1)."""
    d2 = torch.where(ok, d2, torch.full_like(d2, float("inf")))
    dmin = d2.amin(dim=1)
    big = torch.iinfo(torch.int64).max
    cand = torch.where(ok & (d2 == dmin[:, None]), key[None, :],
                       torch.full_like(key, big)[None, :])
    arg = cand.argmin(dim=1)
    none = ~ok.any(dim=1)
    dmin = torch.where(none, torch.full_like(dmin, float("inf")), dmin)
    return dmin, torch.where(none, torch.full_like(arg, -1), arg)


def _dense_path(x, y, yg, adj_bool, xg, y_rank, native):
    """Row-chunked distances + mask + min. native: exact GPU fallback over
    pairwise_distance tiles; otherwise the oracle path (unexpanded sum in the
    input dtype)."""
    m, n, d = x.shape[0], y.shape[0], x.shape[1]
    key = (y_rank if y_rank is not None
           else torch.arange(n, device=x.device)).to(torch.int64)
    dmin = torch.empty(m, dtype=x.dtype, device=x.device)
    amin = torch.empty(m, dtype=torch.int64, device=x.device)
    if native:
        from raft_amd.distance import pairwise_distance, DistanceType
        require_ext()
        sub = max(1, (1 << 24) // max(n, 1))
    else:
        sub = max(1, (1 << 22) // max(n * d, 1))
    for s0, s1 in row_chunks(m, sub):
        if native:
            d2 = pairwise_distance(x[s0:s1], y, metric=DistanceType.L2Expanded,
                                   fp32_mode="native")
        else:
            diff = x[s0:s1].unsqueeze(1) - y.unsqueeze(0)
            d2 = (diff * diff).sum(dim=2)
        ok = torch.ones((s1 - s0, n), dtype=torch.bool, device=x.device)
        if adj_bool is not None:
            ok &= adj_bool[s0:s1].index_select(1, yg)
        if xg is not None:
            ok &= yg[None, :] != xg[s0:s1, None]
        dmin[s0:s1], amin[s0:s1] = _pick_min(d2, ok, key)
    return dmin, amin


def _mfma_path(x, y, yg, ends, adj, packed, xg, y_rank, mode, res):
    """The masked MFMA tile engine + (fp32) the exact verify / repair pass."""
    from raft_amd.core.resources import get_resources
    ext = require_ext()
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    m, n, d = x.shape[0], y.shape[0], x.shape[1]
    n_groups = ends.numel()
    # the slices carry zero-padded features (no distance changes); the norms
    # and the exact verify pass read the rows as given
    verify = x.dtype != torch.bfloat16
    if verify:
        nsl = MODE_NSLICE[mode]
        xs = split_bf16_slices(pad_features(x), nsl)
        ys = split_bf16_slices(pad_features(y), nsl)
        lead, tail = SPLIT_BOUND[nsl]
    else:
        xs, ys = [pad_features(x).contiguous()], [pad_features(y).contiguous()]
    xn, yn = row_sqnorms(x), row_sqnorms(y)
    yg32 = yg.to(torch.int32)
    adj_w = None
    if adj is not None:
        adj_w = (adj if packed else _pack_rows(adj)).contiguous()
    xg32 = None if xg is None else xg.to(torch.int32).contiguous()
    rank32 = None if y_rank is None else y_rank.to(torch.int32).contiguous()
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    rescanned = torch.zeros(1, dtype=torch.int64, device=dev)
    yn_max = yn.max().reshape(1)   # device scalar: no host sync

    col_tiles = (n + 127) // 128
    row_tiles = (m + 127) // 128
    n_split = max(1, min(col_tiles, _MAX_SPLIT, -(-_TARGET_BLOCKS // row_tiles)))
    # same policy as epsilon_neighborhood._sweep: the scratch of one row chunk
    # (three 4-byte partials per row and split) stays under half the budget
    res = get_resources(res if res is not None else dev)
    row_chunk = (res.workspace_budget() // 2) // (12 * n_split)
    if row_chunk >= 128:
        row_chunk -= row_chunk % 128
    row_chunk = int(max(1, min(row_chunk, m)))

    dmin = torch.empty(m, dtype=torch.float32, device=dev)
    amin = torch.empty(m, dtype=torch.int32, device=dev)
    ws = res.get_workspace((3, n_split, row_chunk), torch.float32)
    try:
        for s0, s1 in row_chunks(m, row_chunk):
            scratch = ws.view((3, n_split, s1 - s0), torch.float32)
            a_c = None if adj_w is None else adj_w[s0:s1]
            g_c = None if xg32 is None else xg32[s0:s1]
            d1, a1, d2 = ext.masked_l2nn([t[s0:s1] for t in xs], ys, xn[s0:s1], yn,
                                         yg32, n_groups, a_c, g_c, scratch, counters)
            if verify:
                ext.masked_l2nn_verify_repair(x[s0:s1], y, xn[s0:s1], yg32, n_groups,
                                              a_c, g_c, rank32, d1, a1, d2, yn_max,
                                              rescanned, lead=lead, tail=tail)
            dmin[s0:s1] = d1
            amin[s0:s1] = a1
    finally:
        ws.free()
    return dmin, amin.to(torch.int64), counters, rescanned


def _masked_l2nn(x, y, adj, group_idxs, x_group, y_rank, sqrt, fp32_mode,
                 return_stats, res):
    """masked_l2nn plus y_rank: an optional integer [n] permutation that
    replaces the column index in the exact-tie rule (cross_component_nn ranks
    columns by their ORIGINAL row index)."""
    ends, packed = _check_inputs(x, y, adj, group_idxs, x_group, fp32_mode)
    if x.dtype == torch.float16 or (x.dtype == torch.bfloat16 and not x.is_cuda):
        # exact widening: fp16 rides the fp32 engines, the oracle runs in fp32
        x, y = x.float(), y.float()
    m, n = x.shape[0], y.shape[0]
    n_groups = ends.numel()
    dev = x.device
    out_dtype = torch.float32 if x.dtype == torch.bfloat16 else x.dtype
    stats = {"rescanned": 0, "tiles": 0, "tiles_skipped": 0}

    if m == 0 or n == 0 or n_groups == 0:
        dmin = torch.full((m,), float("inf"), dtype=out_dtype, device=dev)
        amin = torch.full((m,), -1, dtype=torch.int64, device=dev)
        return (dmin, amin, stats) if return_stats else (dmin, amin)

    sizes = torch.diff(ends, prepend=ends.new_zeros(1))
    yg = torch.repeat_interleave(torch.arange(n_groups), sizes).to(dev)
    if x.is_cuda and (x.dtype == torch.bfloat16 or
                      (x.dtype == torch.float32 and fp32_mode != "native")):
        mode = _AUTO_MODE if fp32_mode == "auto" else fp32_mode
        dmin, amin, counters, rescanned = _mfma_path(
            x, y, yg, ends, adj, packed, x_group, y_rank, mode, res)
        if return_stats:
            visited, skipped = counters.tolist()
            stats = {"rescanned": int(rescanned.item()),
                     "tiles": visited + skipped, "tiles_skipped": skipped}
    else:
        adj_bool = adj
        if adj is not None and packed:
            adj_bool = _unpack_rows(adj, n_groups)
        dmin, amin = _dense_path(x, y, yg, adj_bool, x_group, y_rank,
                                 native=x.is_cuda)
    if sqrt:
        dmin = dmin.clamp_min(0).sqrt()
    return (dmin, amin, stats) if return_stats else (dmin, amin)


def masked_l2nn(x: torch.Tensor, y: torch.Tensor, adj: torch.Tensor | None = None,
                group_idxs: torch.Tensor | None = None, *,
                x_group: torch.Tensor | None = None, sqrt: bool = False,
                fp32_mode: str = "auto", return_stats: bool = False, res=None):
    """Masked fused L2-NN (reference raft::distance::masked_l2_nn).

    For each row of x [m,d]: the nearest row of y [n,d] among the groups of
    y its mask allows. Returns (min_dists [m], argmins [m] int64[, stats]).

    group_idxs: integer [G] group END offsets into y (the reference
    convention): group g is rows [group_idxs[g-1], group_idxs[g]), group 0
    starts at 0, empty groups are allowed, group_idxs[-1] == n.
    adj: bool [m, G] or packed int32 [m, ceil(G/32)] (core.Bitset bit order,
    bits >= G ignored): row i may match group g iff bit g is set.
    x_group: integer [m]: group x_group[i] is excluded for row i (-1 excludes
    nothing). At least one of adj and x_group is required; with both a column
    is allowed iff its adj bit is set and its group differs from x_group[i].

    Distances are squared L2 unless sqrt=True; exact ties go to the smallest
    index; rows with no allowed column return (+inf, -1).

    fp32_mode (fp32/fp16 GPU inputs): "bf16x1v" / "bf16x2v" run the verified
    MFMA engine with 1 or 2 bf16 slices, "native" an exact row-chunked
    fallback over pairwise_distance, "auto" the default verified engine. bf16
    inputs use one slice and no verify pass; fp64 takes the fallback; CPU
    tensors a pure-PyTorch path. Any d is zero-padded to a multiple of 64.
    stats = {"rescanned": rows that took the exact rescan, "tiles": 128x128
    tiles visited + skipped, "tiles_skipped": tiles whose K-loop the mask
    ruled out}; paths without tiles report 0 tiles.
    """
    return _masked_l2nn(x, y, adj, group_idxs, x_group, None, sqrt, fp32_mode,
                        return_stats, res)


def cross_component_nn(x: torch.Tensor, labels: torch.Tensor, *,
                       fp32_mode: str = "auto", res=None):
    """Nearest cross-component pairs (reference cross_component_nn / connect_components).

    For every component (distinct label) of x [m,d] with at least one point
    outside it: the pair (src in the component, dst outside it) of smallest
    squared L2 distance. Returns (src int64 [c], dst int64 [c], dist [c],
    comp int64 [c]) ordered by label; exact ties go to the smallest src, then
    the smallest dst (original row indices). A single component gives an
    empty result.

    Memory stays O(m): points are sorted by label, the sorted densified labels
    serve as both the y groups and the excluded x group, and no [m, G] mask is
    built. 16-bit inputs are widened to fp32 (exact).
    """
    if x.dim() != 2:
        raise ValueError("x must be 2-D [rows, features]")
    m = x.shape[0]
    if (labels.dim() != 1 or labels.shape[0] != m or labels.dtype not in _INTS
            or labels.device != x.device):
        raise ValueError("labels must be an integer tensor [m] on the device of x")
    if x.dtype in (torch.float16, torch.bfloat16):
        x = x.float()
    dev = x.device
    perm = torch.argsort(labels, stable=True)
    comp, dense, counts = torch.unique_consecutive(
        labels[perm], return_inverse=True, return_counts=True)
    c = comp.numel()
    if c <= 1:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone(), torch.empty(0, dtype=x.dtype, device=dev), e.clone()
    xs = x[perm].contiguous()
    dist, arg = _masked_l2nn(xs, xs, None, counts.cumsum(0), dense, perm, False,
                             fp32_mode, False, res)
    # segmented min per component, then the smallest original src among the
    # rows that reach it
    cmin = torch.full((c,), float("inf"), dtype=dist.dtype, device=dev)
    cmin = cmin.scatter_reduce(0, dense, dist, "amin")
    cand = torch.where(dist == cmin[dense], perm, torch.full_like(perm, m))
    src = torch.full((c,), m, dtype=torch.int64, device=dev)
    src = src.scatter_reduce(0, dense, cand, "amin")
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(m, device=dev)
    dst = perm[arg[inv[src]]]
    return src, dst, cmin, comp.to(torch.int64)
