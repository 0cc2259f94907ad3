"""Every fused L2-NN engine, named through ext.fused_l2nn_split(engine=, gt=),
against an exact integer reference.

Inputs are small integers, so every value, product and partial sum is an
integer below 2^24: the bf16 slices hold x and y exactly (later slices are
zero, but all 3 or 6 slice products still run) and the fp32 MFMA accumulation
is exact in any K order. No tolerance: every engine must return the int64
result bit for bit. y[256:320] duplicates y[0:64], so exact ties cross lanes,
waves, column tiles and column groups; they resolve to the smallest index and
make the second-best equal the best.
"""
import functools

import pytest
import torch

import masked_nn_inputs as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


def _dot(x, y):
    """x @ y.T in int64 (no integer matmul on the device: fp64 is exact here)."""
    return (x.double() @ y.double().T).long()


@functools.lru_cache(maxsize=None)
def _case(m, n, d):
    """Device inputs and the int64 truth (dmin, amin, dmin2) of one shape."""
    g = torch.Generator().manual_seed(1234 + n + d)
    x = torch.randint(-3, 4, (m, d), generator=g).float()
    y = torch.randint(-3, 4, (n, d), generator=g).float()
    y[256:320] = y[0:64]
    x, y = x.cuda(), y.cuda()
    xi, yi = x.long(), y.long()
    xn, yn = (xi * xi).sum(1), (yi * yi).sum(1)
    D = xn[:, None] + yn[None, :] - 2 * _dot(x, y)
    amin = (D * n + torch.arange(n, device=D.device)).argmin(1)
    top2 = D.sort(1).values[:, :2]
    return x, y, xn.float(), yn.float(), top2[:, 0].float(), amin.int(), top2[:, 1].float()


def _slices(t, nslice):
    from raft_amd.linalg.split_bf16 import split_bf16_slices
    return [t.to(torch.bfloat16)] if nslice == 1 else split_bf16_slices(t, nslice)


def _run(ext, shape, nslice, engine, gt=0):
    x, y, xn, yn = _case(*shape)[:4]
    return ext.fused_l2nn_split(_slices(x, nslice), _slices(y, nslice), xn, yn,
                                engine=engine, gt=gt)


def _check(out, shape, best_only=False):
    dmin, amin, dmin2 = out
    _, _, _, _, rd, ra, rd2 = _case(*shape)
    assert torch.equal(dmin, rd)
    assert torch.equal(amin, ra)
    if best_only:   # persist tracks no second-best: it reports dmin2 = dmin
        assert torch.equal(dmin2, dmin)
    else:
        assert torch.equal(dmin2, rd2)


# m=300: a partial last row tile for the 128- and the 256-row engines; d=128:
# two K-steps; n=512: the least that gives the w8 and 256 engines two column
# tiles and gt=4 one full group
BASE = (300, 512, 128)
BASE_CASES = (
    [(e, ns, 0) for e in ("v1", "v1_db", "w8", "persist") for ns in (1, 2, 3)]
    + [("v1_phased", 2, 0), ("2d_phased", 2, 2)]
    + [(e, ns, gt) for e in ("2d", "2d_bk32") for gt in (1, 2, 4) for ns in (1, 2)]
    + [(e, ns, 0) for e in ("2d_ad", "256") for ns in (1, 2)]
)


@pytest.mark.parametrize("engine,nslice,gt", BASE_CASES)
def test_engine_exact(dev, ext, engine, nslice, gt):
    _check(_run(ext, BASE, nslice, engine, gt), BASE, best_only=engine == "persist")
    name, got_gt = ext.l2nn_resolve_engine(nslice, *BASE, engine=engine, gt=gt)
    assert name == engine
    if gt or not engine.startswith("2d"):   # gt=0 on a 2d engine: its default
        assert got_gt == gt


WIDE = (300, 1024, 128)


def test_2d_gt8(dev, ext):
    assert ext.l2nn_resolve_engine(1, *WIDE, engine="2d", gt=8) == ("2d", 8)
    _check(_run(ext, WIDE, 1, "2d", 8), WIDE)


@pytest.mark.parametrize("nslice", [1, 2, 3])
def test_auto_is_the_resolved_engine(dev, ext, nslice):
    engine, gt = ext.l2nn_resolve_engine(nslice, *WIDE)
    assert engine != "auto"
    auto = _run(ext, WIDE, nslice, "auto")
    _check(auto, WIDE, best_only=engine == "persist")
    named = _run(ext, WIDE, nslice, engine, gt)
    for a, b in zip(auto, named):
        assert torch.equal(a, b)


ODD = (300, 384, 64)   # 3 column tiles, one K-step


def test_2d_gt_halves_to_divide_the_col_tiles(dev, ext):
    assert ext.l2nn_resolve_engine(1, *ODD, engine="2d", gt=2) == ("2d", 1)
    _check(_run(ext, ODD, 1, "2d", 2), ODD)


def test_v1_odd_col_tiles(dev, ext):
    _check(_run(ext, ODD, 2, "v1"), ODD)


def test_named_engine_never_falls_back(dev, ext):
    with pytest.raises(RuntimeError, match=r"'256'.*multiple of 256"):
        _run(ext, ODD, 1, "256")
    with pytest.raises(RuntimeError, match=r"'2d'.*nslice must be 1 or 2"):
        _run(ext, BASE, 3, "2d")
    with pytest.raises(RuntimeError, match="unknown engine"):
        _run(ext, BASE, 1, "v3")


@pytest.mark.parametrize("variant", ["xg", "adj"])
@pytest.mark.parametrize("nslice", [1, 2])
def test_masked_exact(dev, ext, variant, nslice):
    """The masked engine on the same construction, straight from the kernel
    (no verify / repair pass): two column splits, so the index-guarded merge
    runs in the wave combine and in the combine kernel."""
    m, n, d = BASE
    x, y, xn, yn = _case(*BASE)[:4]
    g = torch.Generator().manual_seed(7)
    n_groups = 9
    ends = M.group_ends(n, n_groups, g)
    yg = M.groups_of(ends).to(dev)
    adj = torch.rand(m, n_groups, generator=g) < 0.5
    adj[[3, 200]] = False          # rows with no allowed column
    xg = torch.randint(-1, n_groups, (m,), generator=g)
    adj_w = xg32 = None
    if variant == "adj":
        ok = adj.to(dev)[:, yg]
        adj_w = M.pack(adj, dirty_tail=True).to(dev)
    else:
        ok = yg[None, :] != xg.to(dev)[:, None]
        xg32 = xg.to(dev, torch.int32)
    D = (xn.long()[:, None] + yn.long()[None, :] - 2 * _dot(x, y)).double()
    D[~ok] = float("inf")
    key = torch.where(ok, D * n + torch.arange(n, device=dev), D)
    ra = torch.where(ok.any(1), key.argmin(1), -1).int()
    top2 = D.sort(1).values[:, :2].float()

    scratch = torch.empty(3, 2, m, dtype=torch.float32, device=dev)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    dmin, amin, dmin2 = ext.masked_l2nn(_slices(x, nslice), _slices(y, nslice), xn, yn,
                                        yg.int(), n_groups, adj_w, xg32, scratch,
                                        counters)
    assert torch.equal(amin, ra)
    assert torch.equal(dmin, top2[:, 0])
    assert torch.equal(dmin2, top2[:, 1])
