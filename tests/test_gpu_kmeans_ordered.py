"""ext.kmeans_order_rows and ext.kmeans_update_verify_ordered
(csrc/kmeans_ordered.hip), called directly and through kmeans_iterate.

Row ordering: the order words' low 31 bits must be torch.sort(stable=True)'s
indices and the offsets the exclusive scan of bincount, exactly. Bit 31 must be
the rescan decision margin < 2 * (lead * sqrt(xn * cn_max) + tail * (xn +
cn_max)). So that the expected bit does not hang on whether the compiler fuses
a multiply into an add, xn and cn_max are powers of 4 and lead, tail powers of
2: the square root, both products and the sum are then exact in fp32 (checked
against fp64 below), fused or not. dmin is that bound and dmin2 sits at twice
it and one ulp either side, so margin is the bound, one ulp below, two above
(Sterbenz: the subtraction is exact), beside rows with margin 0 and 1e6.

Ordered update: as tests/test_gpu_kmeans_update_verify.py, x and the centroids
are small integers, so every distance, sum, count and the inertia is an integer
below 2^24 that fp32 holds exactly whatever the order of adds and atomics:
every output compares with torch.equal, against int64 truth and against
ext.kmeans_update_verify on the stable sort. x is a centroid plus noise in
{-1, 0, 1} on at most 64 columns, which keeps the inertia below 2^24 at 40000
rows (asserted). Every tenth row gets margin 0 and rescans; every second one of
those carries a wrong label and must move to its true cluster; centroid 1 is
centroid 0 with one coordinate moved by 1, so real near-ties sit beside them.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LEAD, TAIL = 2.0 ** -7, 2.0 ** -12      # the bf16x1v bound


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


def _order_rows(ext, amin, dmin, dmin2, xn, cn_max, k):
    n, dev = amin.numel(), amin.device
    offsets = torch.full((k + 1,), -7, dtype=torch.int32, device=dev)
    order = torch.full((n,), -7, dtype=torch.int32, device=dev)
    table = torch.empty(ext.kmeans_order_rows_workspace(n, k), dtype=torch.int32, device=dev)
    ext.kmeans_order_rows(amin, dmin, dmin2, xn, cn_max, LEAD, TAIL, k, offsets, order, table)
    return offsets, order


def _labels(pattern, n, k, g):
    if pattern == "one":                       # all rows one key
        return torch.full((n,), k // 2, dtype=torch.int32)
    if pattern == "each":                      # every key as evenly as n allows
        return (torch.randperm(n, generator=g) % k).int()
    # "gaps": no rows in the first and last keys and in a band in the middle
    live = [j for j in range(k) if 0 < j < k - 1 and not k // 3 <= j < k // 2] or [0]
    live = torch.tensor(live, dtype=torch.int32)
    return live[torch.randint(0, len(live), (n,), generator=g)]


@pytest.mark.parametrize("pattern", ["one", "gaps", "each"])
@pytest.mark.parametrize("k", [1, 5, 130, 1024])
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 70001])
def test_order_rows(dev, ext, n, k, pattern):
    g = torch.Generator().manual_seed(1000 * n + k)
    amin = _labels(pattern, n, k, g)
    cn_max = torch.tensor([16.0])
    xn = 4.0 ** torch.randint(0, 4, (n,), generator=g).float()
    bound = 2 * (LEAD * (xn * cn_max).sqrt() + TAIL * (xn + cn_max))
    bound64 = 2 * (LEAD * (xn.double() * 16).sqrt() + TAIL * (xn.double() + 16))
    assert bound.dtype == torch.float32 and torch.equal(bound.double(), bound64)
    two = 2 * bound
    kind = torch.randint(0, 5, (n,), generator=g)
    dmin = torch.where(kind == 4, torch.zeros(n), bound)
    dmin2 = torch.stack([two, torch.nextafter(two, torch.zeros(n)),
                         torch.nextafter(two, torch.full((n,), 1e9)), bound,
                         torch.full((n,), 1e6)])[kind, torch.arange(n)]
    near = (dmin2 - dmin) < bound              # fp32, the kernel's operations
    if n >= 64:
        assert {int(kk) for kk in kind[near]} == {1, 3}      # below the bound, zero

    offsets, order = _order_rows(ext, amin.to(dev), dmin.to(dev), dmin2.to(dev),
                                 xn.to(dev), cn_max.to(dev), k)
    perm = torch.sort(amin.to(dev), stable=True).indices
    counts = torch.bincount(amin.to(dev), minlength=k)
    want_offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
    assert torch.equal(offsets, want_offsets)
    assert torch.equal((order & 0x7FFFFFFF).long(), perm)
    assert torch.equal(order < 0, near.to(dev)[perm])


def test_order_rows_binding_refuses(dev, ext):
    """Shapes the counting sort does not serve fail in the binding, before any
    launch; so does a workspace of the wrong size."""
    assert not ext.kmeans_order_rows_serves(2 ** 31, 8)
    assert not ext.kmeans_order_rows_serves(100, 4097)
    assert ext.kmeans_order_rows_serves(2 ** 31 - 1, 4096)
    f = torch.zeros(8, device=dev)
    i = torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="not served"):
        ext.kmeans_order_rows(i, f, f, f, f[:1], LEAD, TAIL, 5000,
                              torch.zeros(5001, dtype=torch.int32, device=dev), i.clone(), i)
    with pytest.raises(RuntimeError, match="workspace"):
        ext.kmeans_order_rows(i, f, f, f, f[:1], LEAD, TAIL, 3,
                              torch.zeros(4, dtype=torch.int32, device=dev), i.clone(), i)


def _update_case(n, d, k):
    """Inputs, int64 truth and the sorted-label kernel's outputs."""
    from raft_amd._ext import require_ext
    ext = require_ext()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(977 * n + 31 * d + k)
    c = torch.randint(-3, 4, (k, d), generator=g, device=dev)
    c[1] = c[0]
    c[1, d // 2] += 1
    x = c[torch.randint(0, k, (n,), generator=g, device=dev)].clone()
    x[:, :64] += torch.randint(-1, 2, (n, min(d, 64)), generator=g, device=dev)
    D = ((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :]
         - 2 * (x.double() @ c.double().T).long())           # int64 [n, k]
    true = (D * k + torch.arange(k, device=dev)).argmin(1)   # ties: smallest
    rows = torch.arange(n, device=dev)
    rescans = rows % 10 == 3
    wrong = rescans & (rows % 20 == 13)
    given = torch.where(wrong, (true + 1) % k, true).int()
    # a row that does not rescan is refined against the label it was given
    final = true
    dmin = D[rows, final]
    assert int(dmin.sum()) < 2 ** 24 and int(D.max()) < 2 ** 24
    t = dict(x=x.float(), c=c.float(), xn=(x * x).sum(1).float(),
             cn_max=(c * c).sum(1).max().float().reshape(1), given=given,
             dmin_in=torch.zeros(n, device=dev),
             dmin2_in=torch.where(rescans, 0.0, 1.0e6).float(),
             sums=torch.zeros(k, d, dtype=torch.long, device=dev).index_add_(0, final, x).float(),
             counts=torch.bincount(final, minlength=k).float(), dmin=dmin.float(),
             amin=final.int(), inertia=dmin.sum().float().reshape(1),
             n_wrong=int(wrong.sum()))
    # the sorted-label kernel on the stable sort of the same labels
    keys_sorted, perm = torch.sort(given, stable=True)
    old = dict(dmin=t["dmin_in"].clone(), amin=given.clone(),
               sums=torch.zeros(k, d, device=dev), counts=torch.zeros(k, device=dev),
               inertia=torch.zeros(1, device=dev))
    ext.kmeans_update_verify(t["x"], perm.to(torch.int32), keys_sorted, t["c"], t["xn"],
                             old["dmin"], old["amin"], t["dmin2_in"], t["cn_max"],
                             old["sums"], old["counts"], old["inertia"],
                             lead=LEAD, tail=TAIL)
    t["old"] = old
    return t


# d: 64, 100 the scalar column map at 4 registers per row, 256 VEC4 at 4; 260,
# 512, 1024 VEC4 at 16 registers per row, 260 with a ragged last quad.
# n: 7 is less than one wave's chunk of 8 rows, 1000 is 125 waves, 40000 is
# many blocks of waves (and ten blocks of the counting sort).
@pytest.mark.parametrize("k", [3, 130])
@pytest.mark.parametrize("n", [7, 1000, 40000])
@pytest.mark.parametrize("d", [64, 100, 256, 260, 512, 1024])
def test_update_verify_ordered(dev, ext, d, n, k):
    t = _update_case(n, d, k)
    assert t["n_wrong"] == len(range(13, n, 20))
    offsets, order = _order_rows(ext, t["given"], t["dmin_in"], t["dmin2_in"], t["xn"],
                                 t["cn_max"], k)

    def run(write_back):
        out = dict(dmin=t["dmin_in"].clone(), amin=t["given"].clone(),
                   sums=torch.zeros(k, d, device=dev), counts=torch.zeros(k, device=dev),
                   inertia=torch.zeros(1, device=dev))
        ext.kmeans_update_verify_ordered(t["x"], order, offsets, t["c"], out["dmin"],
                                         out["amin"], out["sums"], out["counts"],
                                         out["inertia"], write_back=write_back)
        return out

    on, off, old = run(True), run(False), t["old"]
    # against the sorted-label kernel
    assert torch.equal(on["dmin"], old["dmin"])
    assert torch.equal(on["amin"], old["amin"])
    assert torch.equal(on["counts"], old["counts"])
    # against int64 truth (tests/test_gpu_kmeans_update_verify.py: exact)
    assert torch.equal(on["amin"], t["amin"])
    assert torch.equal(on["dmin"], t["dmin"])
    for out in (on, off):
        assert torch.equal(out["counts"], t["counts"])
        assert torch.equal(out["sums"], t["sums"])
        assert torch.equal(out["inertia"], t["inertia"])
    # write_back off: not a bit of dmin / amin moves
    assert torch.equal(off["dmin"], t["dmin_in"])
    assert torch.equal(off["amin"], t["given"])


ROUTE_M, ROUTE_D, ROUTE_K, ROUTE_ITERS = 20000, 64, 37, 3


@functools.lru_cache(maxsize=None)
def _route_case():
    g = torch.Generator().manual_seed(4242)
    c_true = torch.randint(-8, 9, (ROUTE_K, ROUTE_D), generator=g)
    label = torch.randint(0, ROUTE_K, (ROUTE_M,), generator=g)
    x = c_true[label] + torch.randint(-1, 2, (ROUTE_M, ROUTE_D), generator=g)
    c0 = c_true + torch.randint(-1, 2, (ROUTE_K, ROUTE_D), generator=g)
    return x.float().cuda(), c0.float().cuda()


@pytest.mark.parametrize("mode", ["auto", "bf16x2v"])
def test_route_against_generic_loop(dev, ext, mode, monkeypatch):
    """kmeans_iterate's loop on the ordered pair against the generic loop,
    three iterations. x is integer and the blobs are far apart, so both loops
    assign alike and every centroid sum and count is an exact integer: the
    centroids compare with torch.equal, as tests/test_gpu_kmeans_routes.py
    compares its one step. The inertia after the first step sums distances to
    non-integer centroids: each side rounds a d-term fp32 sum of squares per
    row and this loop folds one fp32 atomic per wave (n / 8 waves here), so
    the two may differ by (n / 8 + 2 d) * 2^-24 of the inertia."""
    import functools as ft
    from raft_amd.cluster import kmeans as km
    from raft_amd.comms import LoopbackComms
    from raft_amd.neighbors.fused_l2nn import fused_l2nn
    x, c0 = _route_case()
    calls = []
    real = ext.kmeans_order_rows
    monkeypatch.setattr(ext, "kmeans_order_rows", lambda *a: (calls.append(1), real(*a))[1])

    c_fast, inertia_fast = km.kmeans_iterate(x, c0, ROUTE_ITERS, fp32_mode=mode)
    assert len(calls) == ROUTE_ITERS
    monkeypatch.setenv("RAFT_AMD_KMEANS_ORDERED", "0")
    c_sort, inertia_sort = km.kmeans_iterate(x, c0, ROUTE_ITERS, fp32_mode=mode)
    assert len(calls) == ROUTE_ITERS

    c_gen, comms = c0, LoopbackComms()
    assign = ft.partial(fused_l2nn, x, fp32_mode=mode)
    for _ in range(ROUTE_ITERS):
        c_gen, _, inertia_gen, _, _ = km._lloyd_step(x, c_gen, assign, comms)
    inertia_gen = float(inertia_gen.item())

    tol = (ROUTE_M / 8 + 2 * ROUTE_D) * 2.0 ** -24
    for c, inertia in ((c_fast, inertia_fast), (c_sort, inertia_sort)):
        assert torch.equal(c, c_gen)
        assert abs(inertia - inertia_gen) <= tol * inertia_gen
