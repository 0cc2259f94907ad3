"""The "2d_xring" fused L2-NN engine (csrc/fused_l2nn_xring.hip), named through
ext.fused_l2nn_split(engine="2d_xring", gt=).

Exact-integer method of test_gpu_l2nn_xreg.py: inputs are integers in
[-3, 3], so every product and partial sum is an integer below 2^24, bf16
holds the inputs exactly and the fp32 MFMA accumulation is exact in any
order. Where n allows, y[256:320] duplicates y[0:64], so exact ties cross
lanes, column fragments, column tiles and column groups; they go to the
smallest index and make the second-best equal the best. No tolerance anywhere.

What is new in this engine is a hand-counted ring of four LDS buffers with up
to three chunks in flight (a chunk is 128 columns x 64 of d), so the
shapes walk the stream length N = gt * d / 64 across the ring: shorter than,
equal to and longer than it, with the ring index compile-time (d = 256) and
carried at run time (d = 64, 128, 192).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ENGINE = "2d_xring"


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
    g = torch.Generator().manual_seed(4321 + m + n + d)
    x = torch.randint(-3, 4, (m, d), generator=g).float()
    y = torch.randint(-3, 4, (n, d), generator=g).float()
    if n >= 320:
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


def _run(ext, shape, engine=ENGINE, gt=0, nslice=1):
    x, y, xn, yn = _case(*shape)[:4]
    return ext.fused_l2nn_split(_slices(x, nslice), _slices(y, nslice), xn, yn,
                                engine=engine, gt=gt)


def _check(out, shape):
    dmin, amin, dmin2 = out
    _, _, _, _, rd, ra, rd2 = _case(*shape)
    assert torch.equal(dmin, rd)
    assert torch.equal(amin, ra)
    assert torch.equal(dmin2, rd2)


# N = 1, 2, 3, 4 chunks in one tile, then 2 chunks over two tiles: the
# prologue issues min(N, 3) chunks and waits vmcnt(8), 4 or 0 for the first,
# and the tail waits count down 4 -> 0, so these are the shapes where a count
# can be wrong
@pytest.mark.parametrize("n,d,gt", [(128, 64, 1), (128, 128, 1), (128, 192, 1),
                                    (128, 256, 1), (256, 64, 2)])
def test_stream_no_longer_than_the_ring(dev, ext, n, d, gt):
    shape = (300, n, d)
    assert ext.l2nn_resolve_engine(1, *shape, engine=ENGINE, gt=gt) == (ENGINE, gt)
    _check(_run(ext, shape, gt=gt), shape)


# m = 300: two full row tiles and 44 rows; n = 512: 4 column tiles; d: KT =
# 1..4; gt 1, 2, 4: 4, 2 and 1 column groups (partials + combine, and at 4
# the direct write). N = 1 .. 16
@pytest.mark.parametrize("gt", [1, 2, 4])
@pytest.mark.parametrize("d", [64, 128, 192, 256])
def test_exact(dev, ext, d, gt):
    shape = (300, 512, d)
    assert ext.l2nn_resolve_engine(1, *shape, engine=ENGINE, gt=gt) == (ENGINE, gt)
    _check(_run(ext, shape, gt=gt), shape)


# gt = 8 covers all of n = 1024 (the flagship form, direct write); d = 192
# is 24 chunks of odd KT, where the ring index wraps at run time
@pytest.mark.parametrize("d", [256, 192])
def test_gt8_single_group(dev, ext, d):
    shape = (300, 1024, d)
    assert ext.l2nn_resolve_engine(1, *shape, engine=ENGINE, gt=8) == (ENGINE, 8)
    _check(_run(ext, shape, gt=8), shape)


# m = 1: every fragment row of every wave is clamped to row 0; m = 129: a
# second block with one live row
@pytest.mark.parametrize("m", [1, 129])
def test_rows(dev, ext, m):
    shape = (m, 1024, 256)
    _check(_run(ext, shape, gt=8), shape)
    shape = (m, 512, 192)
    _check(_run(ext, shape, gt=2), shape)


def test_gt_halves_to_divide_the_col_tiles(dev, ext):
    shape = (300, 384, 128)   # 3 column tiles
    assert ext.l2nn_resolve_engine(1, *shape, engine=ENGINE, gt=8) == (ENGINE, 1)
    _check(_run(ext, shape, gt=8), shape)
    shape = (300, 512, 128)
    assert ext.l2nn_resolve_engine(1, *shape, engine=ENGINE, gt=8) == (ENGINE, 4)
    _check(_run(ext, shape, gt=8), shape)


def test_bitwise_equal_to_2d_and_2d_xreg_on_real_data(dev, ext):
    """All three engines apply the same MFMA sequence in the same K order to
    every output element and the same top-2 rules: seeded normal data, bit
    for bit."""
    m, n, d = 1000, 1024, 256
    g = torch.Generator().manual_seed(99)
    x = torch.randn(m, d, generator=g).to(dev)
    y = torch.randn(n, d, generator=g).to(dev)
    xb, yb = x.to(torch.bfloat16), y.to(torch.bfloat16)
    xn, yn = (x * x).sum(1), (y * y).sum(1)
    for ref_engine in ("2d", "2d_xreg"):
        ref = ext.fused_l2nn_split([xb], [yb], xn, yn, engine=ref_engine, gt=0)
        for gt in (8, 2):
            out = ext.fused_l2nn_split([xb], [yb], xn, yn, engine=ENGINE, gt=gt)
            for a, b in zip(out, ref):
                assert torch.equal(a, b)


def test_repeatable(dev, ext):
    """The flagship form ten times in a row: a read that races its DMA shows
    as a run that differs."""
    shape = (300, 1024, 256)
    first = _run(ext, shape, gt=8)
    _check(first, shape)
    for _ in range(9):
        for a, b in zip(_run(ext, shape, gt=8), first):
            assert torch.equal(a, b)


def test_named_engine_never_falls_back(dev, ext):
    with pytest.raises(RuntimeError, match=r"'2d_xring'.*nslice must be 1"):
        _run(ext, (300, 512, 128), nslice=2)
    with pytest.raises(RuntimeError, match=r"'2d_xring'.*d must be at most 256"):
        _run(ext, (300, 512, 320))
    x, _, xn, _ = _case(300, 512, 128)[:4]     # n = 192: one and a half tiles
    y = torch.ones(192, 128, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ext.fused_l2nn_split(_slices(x, 1), _slices(y, 1), xn, (y * y).sum(1),
                             engine=ENGINE, gt=0)
