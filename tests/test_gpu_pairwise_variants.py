"""Every pairwise L2 kernel, named through ext.pairwise_l2_mfma(variant=) and
ext.pairwise_l2_filter(variant=), against an exact integer reference.

Inputs are small integers, so every value, product and partial sum is an
integer below 2^24: the bf16 slices hold x and y exactly (later slices are
zero, but all 3 or 6 slice products still run) and the fp32 MFMA accumulation
is exact in any K order. No tolerance on squared distances: every variant must
return the int64 result bit for bit. x[5] = y[7] = y[263], so a zero distance
occurs in two column tiles.
"""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_VARS = ("RAFT_AMD_PW256", "RAFT_AMD_PW_BK32", "RAFT_AMD_PW_RM", "RAFT_AMD_PW_NT",
            "RAFT_AMD_FILTER256", "RAFT_AMD_KNN_PX")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


def _inputs(m, n, d):
    """CPU float x, y: seeded small integers with the planted duplicates."""
    g = torch.Generator().manual_seed(4321 + n + d)
    x = torch.randint(-3, 4, (m, d), generator=g).float()
    y = torch.randint(-3, 4, (n, d), generator=g).float()
    y[263] = y[7]
    x[5] = y[7]
    return x, y


def _exact(x, y):
    """int64 squared distances (no integer matmul on the device: fp64 is exact
    here) and the int64 squared norms."""
    xi, yi = x.long(), y.long()
    xn, yn = (xi * xi).sum(1), (yi * yi).sum(1)
    return xn[:, None] + yn[None, :] - 2 * (x.double() @ y.double().T).long(), xn, yn


@functools.lru_cache(maxsize=None)
def _case(m, n, d):
    """Device inputs, fp32 norms and the exact distances as fp32 of one shape."""
    x, y = (t.cuda() for t in _inputs(m, n, d))
    D, xn, yn = _exact(x, y)
    return x, y, xn.float(), yn.float(), D.float()


def _slices(t, nslice):
    from raft_amd.linalg.split_bf16 import split_bf16_slices
    return [t.to(torch.bfloat16)] if nslice == 1 else split_bf16_slices(t, nslice)


def _tile(ext, shape, nslice, variant, **kw):
    x, y, xn, yn, _ = _case(*shape)
    return ext.pairwise_l2_mfma(_slices(x, nslice), _slices(y, nslice), xn, yn,
                                variant=variant, **kw)


# m=300: a partial last row tile for both geometries. n=520 (row stride a
# multiple of 4: interior tiles take the LDS-staged write): 128^2 interior and
# ragged tiles in both directions, 256^2 one interior and one ragged tile row,
# two interior column tiles and an 8-wide one; d=128: two K-steps.
STAGED = (300, 520, 128)
# row stride 390 is no multiple of 4: every tile takes the scalar write; d=64:
# one K-step, which the BK=32 loop runs as two phases
SCALAR = (300, 390, 64)
TILE_CASES = ([("128", ns) for ns in (1, 2, 3)]
              + [(v, ns) for v in ("128_bk32", "256") for ns in (1, 2)])


@pytest.mark.parametrize("shape", [STAGED, SCALAR])
@pytest.mark.parametrize("variant,nslice", TILE_CASES)
def test_tile_exact(dev, ext, variant, nslice, shape):
    assert torch.equal(_tile(ext, shape, nslice, variant), _case(*shape)[4])


def test_tile_preallocated_out_keeps_rows_past_m(dev, ext):
    m, n, _ = STAGED
    out = torch.full((320, n), -5.0, device=dev)
    got = _tile(ext, STAGED, 1, "128", out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out[:m], _case(*STAGED)[4])
    assert torch.equal(out[m:], torch.full((320 - m, n), -5.0, device=dev))


@pytest.mark.parametrize("variant", ["128", "256"])
def test_tile_sqrt(dev, ext, variant):
    # each side is within one ulp of the true root: at most two apart
    torch.testing.assert_close(_tile(ext, STAGED, 1, variant, sqrt_out=True),
                               torch.sqrt(_case(*STAGED)[4]), rtol=2.0 ** -22, atol=0)


@pytest.mark.skipif(any(v in os.environ for v in ENV_VARS),
                    reason="a pairwise tuning variable is set: auto is not '128'")
def test_auto_is_128(dev, ext):
    for nslice in (1, 2, 3):
        assert torch.equal(_tile(ext, STAGED, nslice, "auto"),
                           _tile(ext, STAGED, nslice, "128"))


CAP, COL_OFFSET = 64, 1000
OVERFLOW_ROWS = (10, 11)


def _thresholds(D):
    """Per-row thresholds on exact distances D (any device, int64 or fp32)."""
    thr = D.float().kthvalue(8, dim=1).values   # an integer: ties admitted alike
    thr[list(OVERFLOW_ROWS)] = float(D.max()) + 1   # every column, count > cap
    thr[[5, 6]] = -1.0   # clamps to 0: row 5 its zero distances, row 6 nothing
    return thr


def _filter(ext, shape, nslice, variant):
    m = shape[0]
    x, y, xn, yn, D = _case(*shape)
    out_d = torch.full((m, CAP), -5.0, device=x.device)
    out_i = torch.full((m, CAP), -7, dtype=torch.int32, device=x.device)
    cnt = torch.zeros(m, dtype=torch.int32, device=x.device)
    ext.pairwise_l2_filter(_slices(x, nslice), _slices(y, nslice), xn, yn,
                           _thresholds(D), out_d, out_i, cnt, COL_OFFSET, variant=variant)
    return out_d.cpu(), out_i.cpu(), cnt.cpu()


def _check_filter(out, shape):
    out_d, out_i, cnt = out
    D = _case(*shape)[4]
    admitted = (D <= _thresholds(D).clamp(min=0)[:, None]).cpu()
    D = D.cpu()
    assert torch.equal(cnt.long(), admitted.sum(1))
    assert cnt[5] >= 2 and cnt[6] == 0
    for row in range(shape[0]):
        c = int(cnt[row])
        if row in OVERFLOW_ROWS:
            assert c > CAP
            cols = out_i[row].long() - COL_OFFSET
            assert cols.unique().numel() == CAP
            assert bool(((cols >= 0) & (cols < shape[1])).all())
            assert bool(admitted[row, cols].all())
            assert torch.equal(out_d[row], D[row, cols])
            continue
        assert c <= CAP
        order = out_i[row, :c].argsort()
        ref = admitted[row].nonzero().flatten()
        assert torch.equal(out_i[row, :c][order].long(), ref + COL_OFFSET)
        assert torch.equal(out_d[row, :c][order], D[row, ref])
        assert bool((out_i[row, c:] == -7).all()) and bool((out_d[row, c:] == -5.0).all())


@pytest.mark.parametrize("variant,nslice",
                         [("128", 1), ("128", 2), ("128", 3), ("256", 1), ("256", 2)])
def test_filter_exact(dev, ext, variant, nslice):
    _check_filter(_filter(ext, STAGED, nslice, variant), STAGED)


# n=1100: one full 8-tile column group plus a one-tile group; two K chunks, one
@pytest.mark.parametrize("shape", [(300, 1100, 128), (300, 1100, 64)])
def test_filter_px_exact(dev, ext, shape):
    _check_filter(_filter(ext, shape, 1, "px"), shape)


def test_named_variant_never_falls_back(dev, ext):
    with pytest.raises(RuntimeError, match=r"'256'.*nslice must be 1 or 2"):
        _tile(ext, STAGED, 3, "256")
    with pytest.raises(RuntimeError, match=r"'256'.*nslice must be 1 or 2"):
        _filter(ext, STAGED, 3, "256")
    with pytest.raises(RuntimeError, match=r"'128_bk32'.*nslice must be 1 or 2"):
        _tile(ext, STAGED, 3, "128_bk32")
    with pytest.raises(RuntimeError, match=r"'px'.*d must be 64 or 128"):
        _filter(ext, (300, 1100, 192), 1, "px")
    with pytest.raises(RuntimeError, match=r"'px'.*n must be at least 1024"):
        _filter(ext, STAGED, 1, "px")
    with pytest.raises(RuntimeError, match="unknown variant"):
        _tile(ext, STAGED, 1, "512")
    with pytest.raises(RuntimeError, match="unknown variant"):
        _filter(ext, STAGED, 1, "128_bk32")
