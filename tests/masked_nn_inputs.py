"""Shared inputs and fp64 ground truth for the masked L2-NN tests
(tests/test_masked_nn.py on the CPU, tests/test_gpu_masked_nn.py on the GPU).
Everything here runs on the CPU; references are computed once per process and
never modified."""
import functools
from types import SimpleNamespace

import torch

from eps_inputs import BAND, d2_fp64

#: (m, n, d, G): single element; d-pad + one partial tile; two row tiles +
#: ragged column tile + groups straddling tile edges; five column tiles +
#: multi-K + adj wider than one word; every y row its own group; a second
#: super-tile group on each axis
SHAPES = [(1, 1, 1, 1), (65, 63, 33, 5), (130, 200, 100, 7), (129, 513, 257, 40),
          (257, 300, 64, 300), (1030, 40, 64, 3), (40, 1030, 64, 33)]
CPU_SHAPES = [(1, 1, 1, 1), (65, 63, 33, 5), (130, 200, 100, 7), (257, 300, 64, 300)]
VARIANTS = ("adj", "xg", "both")


def mismatch_cap(m):
    """Rows whose index may differ from the fp64 argmin."""
    return max(2, int(1e-3 * m))


def group_ends(n, n_groups, gen):
    """Random non-decreasing END offsets, last == n; empty groups happen."""
    if n_groups == n:
        return torch.arange(1, n + 1)
    cuts = torch.randint(0, n + 1, (n_groups - 1,), generator=gen).sort().values
    return torch.cat([cuts, torch.tensor([n])])


def groups_of(ends):
    """y_group [n] from the END offsets."""
    sizes = torch.diff(ends, prepend=ends.new_zeros(1))
    return torch.repeat_interleave(torch.arange(ends.numel()), sizes)


def pack(adj, dirty_tail=False):
    """bool [m, G] -> int32 [m, ceil(G/32)] (core/bitset.py layout). With
    dirty_tail the bits at positions >= G are SET: they must be ignored."""
    m, g = adj.shape
    words = (g + 31) // 32
    bits = torch.zeros(m, words * 32, dtype=torch.bool)
    bits[:, :g] = adj
    if dirty_tail:
        bits[:, g:] = True
    w = torch.tensor([1 << k for k in range(31)] + [-(1 << 31)], dtype=torch.int64)
    return (bits.reshape(m, words, 32).to(torch.int64) * w).sum(2).to(torch.int32)


def truth(x, y, ends, adj=None, xg=None):
    """fp64 unexpanded distances with the mask applied: per row the minimum,
    the smallest-index argmin (-1: no allowed column) and the gap from the
    best to the second-best allowed candidate."""
    d2 = d2_fp64(x, y)
    m, n = d2.shape
    yg = groups_of(ends)
    ok = torch.ones(m, n, dtype=torch.bool)
    if adj is not None:
        ok &= adj[:, yg]
    if xg is not None:
        ok &= yg[None, :] != xg[:, None]
    inf = float("inf")
    srt = torch.where(ok, d2, torch.full_like(d2, inf)).sort(dim=1, stable=True)
    none = ~ok.any(dim=1)
    dmin = srt.values[:, 0]
    amin = torch.where(none, torch.full_like(srt.indices[:, 0], -1), srt.indices[:, 0])
    if n > 1:
        gap = srt.values[:, 1] - srt.values[:, 0]
        gap = torch.where(torch.isnan(gap), torch.full_like(gap, inf), gap)
    else:
        gap = torch.full((m,), inf, dtype=torch.float64)
    xn = x.double().pow(2).sum(1)
    yn = y.double().pow(2).sum(1)
    slack = BAND * (xn + (yn.max() if n else 0.0))
    return SimpleNamespace(d2=d2, ok=ok, none=none, dmin=dmin, amin=amin, gap=gap,
                           xn=xn, yn=yn, slack=slack)


def assert_separated(t):
    """The inputs themselves must keep the fp64 gap above the slack in all
    but mismatch_cap rows: the reference alone stays inside the cap."""
    close = int(((t.gap <= t.slack) & ~t.none).sum())
    assert close <= mismatch_cap(t.d2.shape[0]), (close, t.d2.shape)


def check(dmin, amin, t, exact=False):
    """The acceptance rule. exact: index and distance EQUAL the truth."""
    dmin, amin = dmin.detach().cpu().double(), amin.detach().cpu()
    m = t.d2.shape[0]
    assert amin.dtype == torch.int64 and tuple(amin.shape) == (m,)
    assert tuple(dmin.shape) == (m,)
    # rows with no allowed column: exactly (inf, -1)
    assert bool((amin[t.none] == -1).all()) and bool(torch.isinf(dmin[t.none]).all())
    assert bool((dmin[t.none] > 0).all())
    live = (~t.none).nonzero().flatten()
    a = amin[live]
    assert bool(((a >= 0) & (a < t.d2.shape[1])).all()), "index out of range"
    assert bool(t.ok[live, a].all()), "a returned column is not allowed"
    d_at = t.d2[live, a]
    if exact:
        assert torch.equal(a, t.amin[live]), "index differs from the exact truth"
        assert torch.equal(dmin[live], t.dmin[live]), "distance differs from the truth"
        return
    excess = d_at - t.dmin[live]
    err = (dmin[live] - d_at).abs()
    tol = BAND * (t.xn[live] + t.yn[a])
    differ = int((a != t.amin[live]).sum())
    print(f"rows={m} live={live.numel()} differ={differ} "
          f"max_excess/slack={float((excess / t.slack[live]).max()) if live.numel() else 0:.3g} "
          f"max_err/tol={float((err / tol).max()) if live.numel() else 0:.3g}")
    assert bool((excess <= t.slack[live]).all()), "a returned column is not a minimiser"
    assert bool((err <= tol).all()), "returned distance off"
    assert differ <= mismatch_cap(m), (differ, mismatch_cap(m))


@functools.lru_cache(maxsize=None)
def randn_case(m, n, d, n_groups):
    """randn inputs, random group offsets, a ~50% mask with a few empty rows
    and a random x_group. Returns a namespace with the truth per variant."""
    g = torch.Generator().manual_seed(2000 + 7 * m + 3 * n + d + 11 * n_groups)
    x = torch.randn(m, d, generator=g)
    y = torch.randn(n, d, generator=g)
    ends = group_ends(n, n_groups, g)
    adj = torch.rand(m, n_groups, generator=g) < 0.5
    if m >= 8:
        adj[[3, m // 2, m - 1]] = False
    xg = torch.randint(-1, n_groups, (m,), generator=g)
    t = {"adj": truth(x, y, ends, adj=adj), "xg": truth(x, y, ends, xg=xg),
         "both": truth(x, y, ends, adj=adj, xg=xg)}
    for v in t.values():
        assert_separated(v)
    return SimpleNamespace(x=x, y=y, ends=ends, adj=adj, xg=xg, truth=t)


def variant_args(case, variant, device="cpu", packed=False):
    """(adj, x_group) arguments of one variant on a device."""
    adj = xg = None
    if variant in ("adj", "both"):
        adj = (pack(case.adj, dirty_tail=True) if packed else case.adj).to(device)
    if variant in ("xg", "both"):
        xg = case.xg.to(device)
    return adj, xg


@functools.lru_cache(maxsize=None)
def tie_case():
    """Small integers: every product and sum is exact in bf16 and fp32 and
    exact ties are everywhere, so index and distance must equal the truth."""
    g = torch.Generator().manual_seed(5)
    m, n, d, n_groups = 130, 200, 70, 7
    x = torch.randint(-3, 4, (m, d), generator=g).float()
    y = torch.randint(-3, 4, (n, d), generator=g).float()
    y[150:160] = y[20:30]          # duplicated candidates in other groups
    y[5] = x[7]
    y[190] = x[7]
    x[100:] = 0                    # zero-norm rows ...
    y[60:64] = 0                   # ... and columns: bound 0, margin 0
    ends = torch.tensor([0, 31, 64, 64, 129, 170, 200])
    adj = torch.rand(m, n_groups, generator=g) < 0.6
    adj[[3, 65, 129]] = False
    xg = torch.randint(-1, n_groups, (m,), generator=g)
    t = {"adj": truth(x, y, ends, adj=adj), "xg": truth(x, y, ends, xg=xg),
         "both": truth(x, y, ends, adj=adj, xg=xg)}
    assert int((t["both"].gap == 0).sum()) > 0, "the case must hold exact ties"
    return SimpleNamespace(x=x, y=y, ends=ends, adj=adj, xg=xg, truth=t)


@functools.lru_cache(maxsize=None)
def offset_cloud_case():
    """The input that needs the repair: norms ~1090, gaps ~0.15, one-slice
    emulation error of order 1. Every x row has three near-duplicates at
    squared radii {0.30, 0.45, 0.60} (shuffled) in three different groups,
    plus 61 far rows; the mask forbids the nearest one for every third row."""
    g = torch.Generator().manual_seed(13)
    m, d = 192, 64
    x = 4 + torch.randn(m, d, generator=g)
    r2 = torch.tensor([0.30, 0.45, 0.60])
    order = torch.stack([torch.randperm(3, generator=g) for _ in range(m)])  # [m,3]
    parts = []
    for k in range(3):
        u = torch.randn(m, d, generator=g)
        u = u / u.norm(dim=1, keepdim=True)
        parts.append(x + u * r2[order[:, k]].sqrt()[:, None])
    y = torch.cat(parts + [4 + torch.randn(61, d, generator=g)])
    ends = torch.tensor([m, 2 * m, 3 * m, 3 * m + 61])
    adj = torch.ones(m, 4, dtype=torch.bool)
    rows = torch.arange(0, m, 3)
    adj[rows, order[rows].argmin(dim=1)] = False   # the group of radius 0.30
    t = truth(x, y, ends, adj=adj)
    assert_separated(t)
    return SimpleNamespace(x=x, y=y, ends=ends, adj=adj, truth=t)


def cross_component_truth(x, labels):
    """fp64 brute force: per distinct label with a point outside it, the pair
    (src inside, dst outside) of smallest squared distance; ties to the
    smallest src, then the smallest dst. Returns (src, dst, dist, comp)."""
    d2 = d2_fp64(x, x)
    comps = labels.unique(sorted=True)
    src, dst, dist, comp = [], [], [], []
    for c in comps.tolist():
        inside = labels == c
        if bool(inside.all()):
            continue
        sub = d2[inside][:, ~inside]
        best = sub.min()
        r, col = (sub == best).nonzero()[0].tolist()   # row-major: src, then dst
        src.append(int(inside.nonzero().flatten()[r]))
        dst.append(int((~inside).nonzero().flatten()[col]))
        dist.append(float(best))
        comp.append(c)
    return (torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64),
            torch.tensor(dist, dtype=torch.float64), torch.tensor(comp, dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def blobs_case():
    """Three separated blobs on a 1/4 grid (every distance exact in bf16, fp32
    and fp64) with interleaved labels, two singleton labels and duplicated
    points across components, so the tie-break decides several entries."""
    g = torch.Generator().manual_seed(17)
    d = 8
    centers = torch.tensor([[0.] * d, [16.] * d, [-16.] + [16.] * (d - 1)])
    pts = [c + torch.randint(-8, 9, (50, d), generator=g) / 4 for c in centers]
    x = torch.cat(pts + [torch.full((1, d), 40.), torch.full((1, d), -40.)])
    labels = torch.cat([torch.full((50,), 7), torch.full((50,), 2),
                        torch.full((50,), 5), torch.tensor([9, 0])])
    # duplicates across components: rows 10 (blob 0) and 60 (blob 1) both sit
    # on blob 2's point 120, rows 20 and 130 on blob 1's point 70
    x[10] = x[120]
    x[60] = x[120]
    x[20] = x[70]
    x[130] = x[70]
    p = torch.randperm(x.shape[0], generator=g)    # interleave the components
    x, labels = x[p].contiguous(), labels[p].contiguous()
    return SimpleNamespace(x=x, labels=labels, truth=cross_component_truth(x, labels))


@functools.lru_cache(maxsize=None)
def emst_points():
    g = torch.Generator().manual_seed(19)
    return torch.randn(300, 5, generator=g)


def boruvka_emst(x, cross_component_nn, **kw):
    """Test-local Boruvka loop: one cross_component_nn call per round. Returns
    the edge list [(u, v)] of the Euclidean MST."""
    m = x.shape[0]
    parent = list(range(m))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    edges = []
    labels = torch.arange(m)
    for _ in range(32):
        src, dst, _, _ = cross_component_nn(x, labels.to(x.device), **kw)
        if src.numel() == 0:
            break
        for u, v in zip(src.tolist(), dst.tolist()):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[ru] = rv
                edges.append((u, v))
        labels = torch.tensor([find(i) for i in range(m)])
    return edges
