"""The checked split-bf16 operands of the four MFMA bindings that take slice
lists: fused_l2nn_split, pairwise_l2_mfma, pairwise_l2_filter and
eps_neighbors_l2sq reject the same malformed operands with an error that names
the binding, before anything is launched, and accept well-formed ones.

Every malformed operand is at least as large as the well-formed one it
replaces."""
import pytest
import torch

from raft_amd.linalg.split_bf16 import SPLIT_BOUND, split_bf16_slices

pytestmark = pytest.mark.gpu

M = N = 128
D = 64
CAP, COL_OFFSET = 128, 1000
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


@pytest.fixture(scope="module")
def good(dev):
    """Well-formed 2-slice operands and the fp64 squared distances. Every x
    row is a y row plus noise: the nearest neighbor is unambiguous."""
    g = torch.Generator().manual_seed(77)
    y = torch.randn(N, D, generator=g)
    x = y[torch.randperm(N, generator=g)] + 0.5 * torch.randn(M, D, generator=g)
    x, y = x.to(dev), y.to(dev)
    ref = torch.cdist(x.double(), y.double()) ** 2
    return {"x": x, "y": y, "xs": split_bf16_slices(x, 2), "ys": split_bf16_slices(y, 2),
            "xn": (x * x).sum(1), "yn": (y * y).sum(1), "ref": ref}


def _bad_operands(ops):
    """(name, operands) with one operand of `ops` replaced by a malformed one."""
    dev = ops["x"].device

    def z(*shape, dtype=BF16):
        return torch.zeros(shape, dtype=dtype, device=dev)

    xs0, ys0 = ops["xs"][0], ops["ys"][0]
    return [
        ("second x slice has 256 rows", {**ops, "xs": [xs0, z(2 * M, D)]}),
        ("y has d = 128, x has 64", {**ops, "ys": [z(N, 2 * D), z(N, 2 * D)]}),
        ("a slice is fp16", {**ops, "xs": [xs0, z(M, D, dtype=torch.float16)]}),
        ("a slice is a transposed view", {**ops, "ys": [ys0, z(D, N).t()]}),
        ("a slice is 3-D", {**ops, "xs": [xs0, z(M, D, 1)]}),
        ("xn has m + 1 elements", {**ops, "xn": z(M + 1, dtype=torch.float32)}),
        ("yn is fp64", {**ops, "yn": z(N, dtype=torch.float64)}),
        ("unequal slice counts", {**ops, "ys": [ys0, z(N, D), z(N, D)]}),
    ]


def _fused(ext, o):
    return ext.fused_l2nn_split(o["xs"], o["ys"], o["xn"], o["yn"])


def _tile(ext, o):
    return ext.pairwise_l2_mfma(o["xs"], o["ys"], o["xn"], o["yn"])


def _filter(ext, o):
    dev = o["x"].device
    out_d = torch.full((M, CAP), -5.0, device=dev)
    out_i = torch.full((M, CAP), -7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(M, dtype=torch.int32, device=dev)
    thr = torch.full((M,), 1e30, device=dev)         # admits every column
    ext.pairwise_l2_filter(o["xs"], o["ys"], o["xn"], o["yn"], thr, out_d, out_i,
                           cnt, COL_OFFSET)
    return out_d, out_i, cnt


def _eps(ext, o, eps_sq=1.0):
    dev = o["x"].device
    bitmap = torch.zeros((M, (N + 31) // 32), dtype=torch.int32, device=dev)
    rechecked = torch.zeros(1, dtype=torch.int64, device=dev)
    lead, tail = SPLIT_BOUND[2]
    ext.eps_neighbors_l2sq(o["xs"], o["ys"], o["xn"], o["yn"], o["x"], o["y"], bitmap,
                           rechecked, N, eps_sq, lead, tail)
    return bitmap


BINDINGS = {"fused_l2nn_split": _fused, "pairwise_l2_mfma": _tile,
            "pairwise_l2_filter": _filter, "eps_neighbors_l2sq": _eps}


@pytest.mark.parametrize("who", list(BINDINGS))
def test_malformed_operands_are_rejected(dev, ext, good, who):
    cases = _bad_operands(good)
    assert len(cases) == 8
    for name, ops in cases:
        with pytest.raises(RuntimeError, match=who):
            BINDINGS[who](ext, ops)
            pytest.fail(f"{who} accepted: {name}")


def _envelope(good):
    """|d2 error| <= 2 |dot error| of the 2-slice emulation, per pair."""
    lead, tail = SPLIT_BOUND[2]
    xn, yn = good["xn"].double()[:, None], good["yn"].double()[None, :]
    return 2.0 * (lead * (xn * yn).sqrt() + tail * (xn + yn))


def test_fused_l2nn_split_accepts(dev, ext, good):
    dmin, amin, dmin2 = _fused(ext, good)
    rd, ra = good["ref"].min(dim=1)
    # the bounds of test_gpu_kernels.py TestFusedL2NNMfma for bf16x2
    assert (amin.long() == ra).float().mean() > 0.999
    rel = ((dmin.double() - rd).abs() / rd.clamp_min(1e-2)).median()
    assert float(rel) < 2e-3
    assert bool((dmin2 >= dmin).all())


def test_pairwise_l2_mfma_accepts(dev, ext, good):
    out = _tile(ext, good)
    assert out.shape == (M, N) and out.dtype == torch.float32
    assert bool(((out.double() - good["ref"]).abs() <= _envelope(good)).all())


def test_pairwise_l2_filter_accepts(dev, ext, good):
    out_d, out_i, cnt = _filter(ext, good)
    assert bool((cnt == N).all())
    cols, order = (out_i.long() - COL_OFFSET).sort(dim=1)
    assert torch.equal(cols, torch.arange(N, device=dev).expand(M, N))
    d2 = out_d.gather(1, order).double()
    assert bool(((d2 - good["ref"]).abs() <= _envelope(good)).all())


def test_eps_neighbors_l2sq_accepts(dev, ext, good):
    ref = good["ref"]
    eps_sq = float(ref.median())
    bitmap = _eps(ext, good, eps_sq)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    adj = ((bitmap.unsqueeze(2) >> shifts) & 1).bool().reshape(M, -1)[:, :N]
    # verified engine: the decision is the exact fp32 one; only a pair within
    # fp32 rounding of the threshold (d terms, 2^-24 each) may differ from fp64
    decided = (ref - eps_sq).abs() > (D + 2) * 2.0 ** -24 * eps_sq
    assert int(decided.sum()) >= M * N - 4
    assert torch.equal(adj[decided], (ref <= eps_sq)[decided])


def test_presplit_verifies_with_the_envelope_of_its_slice_count(dev, ext):
    """fused_l2nn_presplit defaults to SPLIT_BOUND[number of slices]. Rows are
    structureless, so many best/second-best gaps lie inside the 1-slice
    envelope: verified against the 2^6-tighter 2-slice one, those rows would
    keep a column that one bf16 slice ranked first wrongly. The verified
    result is the exact fp32 argmin: the chosen column's fp64 distance is the
    minimum up to the rounding of two fp32 distance evaluations (d + 2
    roundings of 2^-24 each, relative to the norms xn + yn)."""
    from raft_amd.neighbors.fused_l2nn import fused_l2nn_presplit
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2000, D, generator=g).to(dev)
    y = torch.randn(16, D, generator=g).to(dev)
    dmin, amin = fused_l2nn_presplit(split_bf16_slices(x, 1), (x * x).sum(1), y,
                                     verify_x=x)
    ref = torch.cdist(x.double(), y.double()) ** 2
    chosen = ref.gather(1, amin[:, None])[:, 0]
    scale = (x.double() ** 2).sum(1) + (y.double() ** 2).sum(1).max()
    tol = 2 * (D + 2) * 2.0 ** -24 * scale
    assert bool((chosen <= ref.min(dim=1).values + tol).all())
    assert bool(((dmin.double() - chosen).abs() <= tol).all())
