"""masked_l2nn / cross_component_nn on the GPU: the masked MFMA tile engine
with its exact verify / repair pass, the tile skip, the workspace chunking and
the exact fallback, against the fp64 truth of tests/masked_nn_inputs.py."""
import pytest
import torch

import masked_nn_inputs as M
from raft_amd.neighbors import cross_component_nn, masked_l2nn

pytestmark = pytest.mark.gpu

MODES = ["bf16x1v", "bf16x2v", "native"]
DEV = "cuda"
IDS = dict(ids=lambda s: "x".join(map(str, s)))


def _run(case, variant, packed=False, **kw):
    adj, xg = M.variant_args(case, variant, DEV, packed=packed)
    return masked_l2nn(case.x.to(DEV), case.y.to(DEV), adj, case.ends.to(DEV),
                       x_group=xg, **kw)


@pytest.mark.parametrize("shape", M.SHAPES, **IDS)
@pytest.mark.parametrize("mode", MODES)
def test_randn_vs_fp64(shape, mode):
    case = M.randn_case(*shape)
    for variant in M.VARIANTS:
        dmin, amin = _run(case, variant, fp32_mode=mode)
        assert dmin.dtype == torch.float32 and dmin.is_cuda and amin.is_cuda
        M.check(dmin, amin, case.truth[variant])
        if variant != "xg":
            # packed adj (with set bits past G) gives identical outputs
            dmin_p, amin_p = _run(case, variant, packed=True, fp32_mode=mode)
            assert torch.equal(dmin_p, dmin) and torch.equal(amin_p, amin)


def test_auto_is_a_verified_engine():
    case = M.randn_case(130, 200, 100, 7)
    ref = _run(case, "both", fp32_mode="bf16x2v")
    got = _run(case, "both")
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16],
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("mode", MODES)
def test_integer_ties_equal_the_truth(dtype, mode):
    """Everything is exact in bf16 and fp32: index and distance equal the
    truth bit for bit (smallest-index tie rule, `<=` in the margin test with
    zero norms, duplicated candidates in different groups)."""
    case = M.tie_case()
    x, y = case.x.to(DEV, dtype), case.y.to(DEV, dtype)
    for variant in M.VARIANTS:
        adj, xg = M.variant_args(case, variant, DEV)
        dmin, amin, stats = masked_l2nn(x, y, adj, case.ends.to(DEV), x_group=xg,
                                        fp32_mode=mode, return_stats=True)
        M.check(dmin, amin, case.truth[variant], exact=True)
        if dtype != torch.bfloat16 and mode != "native":
            # every exact tie has margin 0 and must take the rescan
            ties = int(((case.truth[variant].gap == 0) & ~case.truth[variant].none).sum())
            assert stats["rescanned"] >= ties > 0


@pytest.mark.parametrize("mode", MODES)
def test_offset_cloud_needs_the_repair(mode):
    case = M.offset_cloud_case()
    dmin, amin, stats = masked_l2nn(case.x.to(DEV), case.y.to(DEV), case.adj.to(DEV),
                                    case.ends.to(DEV), fp32_mode=mode,
                                    return_stats=True)
    print(mode, stats)
    M.check(dmin, amin, case.truth)
    if mode == "bf16x1v":
        assert stats["rescanned"] > 0
    d_sqrt, a_sqrt = masked_l2nn(case.x.to(DEV), case.y.to(DEV), case.adj.to(DEV),
                                 case.ends.to(DEV), fp32_mode=mode, sqrt=True)
    assert torch.equal(a_sqrt, amin) and torch.equal(d_sqrt, dmin.clamp_min(0).sqrt())


@pytest.mark.parametrize("mode", ["bf16x1v", "bf16x2v"])
def test_tile_skipping(mode):
    g = torch.Generator().manual_seed(23)
    m = n = 512
    x = torch.randn(m, 64, generator=g)
    y = torch.randn(n, 64, generator=g)
    ends = torch.tensor([128, 256, 384, 512])
    eye = torch.eye(4, dtype=torch.bool).repeat_interleave(128, 0)    # [m, 4]
    xd, yd, ed = x.to(DEV), y.to(DEV), ends.to(DEV)

    # the count a CPU walk over the 128x128 tiles of the mask gives
    ok = eye[:, M.groups_of(ends)]
    dead = sum(1 for r in range(0, m, 128) for c in range(0, n, 128)
               if not bool(ok[r:r + 128, c:c + 128].any()))
    assert dead == 12
    dmin, amin, stats = masked_l2nn(xd, yd, eye.to(DEV), ed, fp32_mode=mode,
                                    return_stats=True)
    assert stats["tiles"] == 16 and stats["tiles_skipped"] == dead
    M.check(dmin, amin, M.truth(x, y, ends, adj=eye))
    # the complement mask, once as adj and once as x_group: only the four
    # diagonal tiles are dead, and the two spellings give the same outputs
    xg = torch.arange(4).repeat_interleave(128)
    d2_, a2_, s2_ = masked_l2nn(xd, yd, (~eye).to(DEV), ed, fp32_mode=mode,
                                return_stats=True)
    d3_, a3_, s3_ = masked_l2nn(xd, yd, None, ed, x_group=xg.to(DEV),
                                fp32_mode=mode, return_stats=True)
    assert s2_["tiles_skipped"] == s3_["tiles_skipped"] == 4
    assert torch.equal(d2_, d3_) and torch.equal(a2_, a3_)
    M.check(d2_, a2_, M.truth(x, y, ends, xg=xg))
    # the identity-mask result equals an unmasked run restricted to each
    # diagonal block: same pairs, same engine
    for b in range(4):
        sl = slice(128 * b, 128 * (b + 1))
        db, ab = masked_l2nn(xd[sl], yd[sl], torch.ones(128, 1, dtype=torch.bool,
                                                        device=DEV),
                             torch.tensor([128], device=DEV), fp32_mode=mode)
        assert torch.equal(db, dmin[sl]) and torch.equal(ab + 128 * b, amin[sl])

    # all-false adj: every tile is skipped, every row returns (inf, -1)
    dmin, amin, stats = masked_l2nn(xd, yd, torch.zeros_like(eye).to(DEV), ed,
                                    fp32_mode=mode, return_stats=True)
    assert stats["tiles"] == 16 and stats["tiles_skipped"] == 16
    assert stats["rescanned"] == 0
    assert bool(torch.isinf(dmin).all()) and bool((dmin > 0).all())
    assert bool((amin == -1).all())


@pytest.mark.parametrize("mode", ["auto", "bf16x1v", "native"])
def test_workspace_limit_chunking_is_invisible(mode):
    from raft_amd.core.resources import Resources
    case = M.randn_case(257, 300, 64, 300)
    ref = _run(case, "both", fp32_mode=mode)
    res = Resources(torch.device(DEV))
    res.set_workspace_limit(8000)   # 3 splits x 12 B per row -> 111-row chunks
    assert (res.workspace_budget() // 2) // 36 <= 257 // 2   # >= 3 chunks
    got = _run(case, "both", fp32_mode=mode, res=res)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert res.get_workspace_resource().outstanding_bytes() == 0


@pytest.mark.parametrize("mode", MODES)
def test_cross_component_nn_blobs_and_ties(mode):
    case = M.blobs_case()
    out = cross_component_nn(case.x.to(DEV), case.labels.to(DEV), fp32_mode=mode)
    src, dst, dist, comp = (o.cpu() for o in out)
    t_src, t_dst, t_dist, t_comp = case.truth
    assert torch.equal(comp, t_comp)
    assert torch.equal(src, t_src) and torch.equal(dst, t_dst)
    assert torch.equal(dist.double(), t_dist)
    out = cross_component_nn(case.x.to(DEV), torch.zeros_like(case.labels).to(DEV),
                             fp32_mode=mode)
    assert all(o.numel() == 0 and o.is_cuda for o in out)


@pytest.mark.parametrize("mode", ["bf16x1v", "bf16x2v"])
def test_boruvka_emst_matches_scipy(mode):
    from scipy.sparse.csgraph import minimum_spanning_tree
    x = M.emst_points()
    edges = M.boruvka_emst(x.to(DEV), cross_component_nn, fp32_mode=mode)
    assert len(edges) == x.shape[0] - 1
    d = M.d2_fp64(x, x).sqrt()
    total = sum(float(d[u, v]) for u, v in edges)
    ref = float(minimum_spanning_tree(d.numpy()).sum())
    assert abs(total - ref) <= 1e-6 * ref, (total, ref)


def test_fp64_takes_the_exact_fallback():
    case = M.randn_case(130, 200, 100, 7)
    adj, xg = M.variant_args(case, "both", DEV)
    dmin, amin, stats = masked_l2nn(case.x.double().to(DEV), case.y.double().to(DEV),
                                    adj, case.ends.to(DEV), x_group=xg,
                                    return_stats=True)
    assert dmin.dtype == torch.float64
    assert stats == {"rescanned": 0, "tiles": 0, "tiles_skipped": 0}
    M.check(dmin, amin, case.truth["both"])
    case = M.tie_case()
    adj, xg = M.variant_args(case, "both", DEV)
    dmin, amin = masked_l2nn(case.x.double().to(DEV), case.y.double().to(DEV), adj,
                             case.ends.to(DEV), x_group=xg)
    M.check(dmin, amin, case.truth["both"], exact=True)
