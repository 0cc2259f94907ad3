"""Epsilon-neighborhood on the GPU: the verified MFMA bitmap engine, the
bitmap -> degrees / CSR / bool kernels, and the chunked driver, against fp64
ground truth computed on the CPU (tests/eps_inputs.py)."""
import pytest
import torch

import eps_inputs as E
from raft_amd.neighbors import eps_neighbors_l2sq, eps_neighbors_l2sq_csr

pytestmark = pytest.mark.gpu

MODES = ["auto", "bf16x1v", "bf16x2v", "native"]
DEV = "cuda"


def _all_forms(x, y, eps, **kw):
    """bool, packed and CSR outputs of one query, checked against each other
    and against the output contract (dtypes, devices, tail bits, sorting)."""
    adj, vd = eps_neighbors_l2sq(x, y, eps, **kw)
    words, vd_w = eps_neighbors_l2sq(x, y, eps, packed=True, **kw)
    csr = eps_neighbors_l2sq_csr(x, y, eps, **kw)
    assert torch.equal(vd, vd_w)
    m = x.shape[0]
    n = (x if y is None else y).shape[0]
    E.check_contract(adj, words, csr, vd, m, n, "cuda")
    return adj, vd, csr


@pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_randn_vs_fp64(shape, mode):
    x, y, d2, band, eps_list = E.randn_case(*shape)
    xg, yg = x.to(DEV), y.to(DEV)
    for eps in eps_list:
        adj, _, _ = _all_forms(xg, yg, eps, fp32_mode=mode)
        E.compare_outside_band(adj, d2, band, eps)


@pytest.mark.parametrize("dtype,mode", [(torch.float32, m) for m in MODES]
                         + [(torch.bfloat16, "auto"), (torch.float16, "auto")],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_exact_ties_no_exclusions(dtype, mode):
    """Integer inputs: every product and sum is exact, 130 pairs sit exactly
    on eps_sq = 519 and must be included; adjacency, vd and CSR equal the
    oracle bit for bit."""
    x, y, d2 = E.tie_case()
    truth = d2 <= E.TIE_EPS
    assert int((d2 == E.TIE_EPS).sum()) == 130
    adj, vd, (indptr, indices, _) = _all_forms(x.to(DEV, dtype), y.to(DEV, dtype),
                                               E.TIE_EPS, fp32_mode=mode)
    assert torch.equal(adj.cpu(), truth)
    assert torch.equal(vd[:-1].cpu(), truth.sum(1))
    assert int(vd[-1]) == int(truth.sum())
    assert torch.equal(indices.cpu().long(), truth.nonzero()[:, 1])

    x, y, d2 = E.duplicate_case()
    adj, vd, (indptr, indices, _) = _all_forms(x.to(DEV, dtype), y.to(DEV, dtype),
                                               0.0, fp32_mode=mode)
    assert torch.equal(adj.cpu(), d2 == 0)
    assert torch.equal(indices.cpu().long(), (d2 == 0).nonzero()[:, 1])


@pytest.mark.parametrize("mode", ["bf16x1v", "bf16x2v", "auto"])
def test_offset_cloud_needs_the_recheck(mode):
    """Norms ~1090 against eps_sq = 0.5: an unverified 1-slice evaluation gets
    ~250 pairs wrong outside the band, so bf16x1v passes only if the band
    pairs really are re-decided in exact fp32."""
    x, y, d2, band, eps = E.offset_cloud_case()
    assert y.shape[0] == 637 and int((d2 <= eps).sum()) == 291
    xg, yg = x.to(DEV), y.to(DEV)
    adj, vd, stats = eps_neighbors_l2sq(xg, yg, eps, fp32_mode=mode,
                                        return_stats=True)
    print(f"mode={mode} rechecked={stats['rechecked']}")
    n_excl = E.compare_outside_band(adj, d2, band, eps)
    assert n_excl == 25
    assert isinstance(stats["rechecked"], int)
    if mode == "bf16x1v":
        assert stats["rechecked"] > 0
    _all_forms(xg, yg, eps, fp32_mode=mode)


@pytest.mark.parametrize("mode", ["auto", "bf16x1v", "native"])
def test_workspace_limit_chunking_is_invisible(mode):
    from raft_amd.core.resources import Resources
    m, n, d = 257, 300, 64
    x, y, d2, band, eps_list = E.randn_case(m, n, d)
    xg, yg = x.to(DEV), y.to(DEV)
    eps = eps_list[1]
    ref_adj, ref_vd, ref_csr = _all_forms(xg, yg, eps, fp32_mode=mode)
    res = Resources(torch.device(DEV))
    res.set_workspace_limit(8000)   # 40 B per bitmap row -> 100-row chunks
    assert (res.workspace_budget() // 2) // 40 <= m // 2   # >= 3 chunks
    adj, vd, csr = _all_forms(xg, yg, eps, fp32_mode=mode, res=res)
    assert torch.equal(adj, ref_adj) and torch.equal(vd, ref_vd)
    for a, b in zip(csr, ref_csr):
        assert torch.equal(a, b)
    assert res.get_workspace_resource().outstanding_bytes() == 0
    # explicit row_chunk values, tile-aligned or not
    for rc in (1, 129):
        got, got_vd = eps_neighbors_l2sq(xg, yg, eps, fp32_mode=mode, row_chunk=rc)
        assert torch.equal(got, ref_adj) and torch.equal(got_vd, ref_vd)


@pytest.mark.parametrize("mode,offset", [("auto", 100.0), ("bf16x1v", 100.0),
                                         ("bf16x2v", 100.0), ("native", 0.0)])
def test_self_join_diagonal_and_symmetry(mode, offset):
    # the offset puts every pair inside the verified engines' band (norms
    # ~3e5 against distances ~66): the whole matrix takes the exact recheck.
    # The native fallback has no recheck; its expanded fp32 form is only
    # asked to be symmetric where it is well conditioned.
    g = torch.Generator().manual_seed(5)
    x = (offset + torch.randn(200, 33, generator=g)).to(DEV)
    for eps in (0.0, 60.0):
        adj, vd, _ = _all_forms(x, None, eps, fp32_mode=mode)
        assert bool(adj.diagonal().all())
        assert torch.equal(adj, adj.t())
    adj, vd = eps_neighbors_l2sq(x, None, 0.0, fp32_mode=mode)
    assert int(vd[-1]) == 200


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_empty_and_full(dtype):
    x, y, _ = E.tie_case()
    xg, yg = x.to(DEV, dtype), y.to(DEV, dtype)
    adj, vd, (indptr, indices, _) = _all_forms(xg, yg, -1.0)
    assert not bool(adj.any()) and int(vd.sum()) == 0 and indices.numel() == 0
    assert torch.equal(indptr.cpu(), torch.zeros(131, dtype=torch.int64))
    adj, vd, _ = _all_forms(xg, yg, float("inf"))
    assert bool(adj.all()) and int(vd[-1]) == 130 * 200


def test_fp64_takes_the_exact_fallback():
    x, y, d2, band, eps_list = E.randn_case(130, 200, 100)
    adj, _, _ = _all_forms(x.double().to(DEV), y.double().to(DEV), eps_list[0])
    E.compare_outside_band(adj, d2, band, eps_list[0])


def test_dimension_mismatch_raises():
    with pytest.raises(ValueError):
        eps_neighbors_l2sq(torch.zeros(4, 8, device=DEV),
                           torch.zeros(4, 9, device=DEV), 1.0)
