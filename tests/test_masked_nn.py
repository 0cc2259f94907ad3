"""masked_l2nn / cross_component_nn on the CPU: the pure-PyTorch oracle path
against the fp64 truth of tests/masked_nn_inputs.py, the argument checks, the
empty cases, and the header <-> kernel-object link of the new launchers."""
import glob
import os
import subprocess

import pytest
import torch

import masked_nn_inputs as M
from raft_amd.neighbors import cross_component_nn, masked_l2nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = dict(ids=lambda s: "x".join(map(str, s)))


@pytest.mark.parametrize("shape", M.CPU_SHAPES, **IDS)
@pytest.mark.parametrize("variant", M.VARIANTS)
def test_randn_vs_fp64(shape, variant):
    case = M.randn_case(*shape)
    adj, xg = M.variant_args(case, variant)
    dmin, amin = masked_l2nn(case.x, case.y, adj, case.ends, x_group=xg)
    assert dmin.dtype == torch.float32
    M.check(dmin, amin, case.truth[variant])
    if adj is not None:
        words, _ = M.variant_args(case, variant, packed=True)
        dmin_p, amin_p = masked_l2nn(case.x, case.y, words, case.ends, x_group=xg)
        assert torch.equal(dmin_p, dmin) and torch.equal(amin_p, amin)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16,
                                   torch.float64],
                         ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("variant", M.VARIANTS)
def test_integer_ties_equal_the_truth(dtype, variant):
    case = M.tie_case()
    adj, xg = M.variant_args(case, variant)
    dmin, amin, stats = masked_l2nn(case.x.to(dtype), case.y.to(dtype), adj, case.ends,
                                    x_group=xg, return_stats=True)
    assert dmin.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    M.check(dmin, amin, case.truth[variant], exact=True)
    assert stats == {"rescanned": 0, "tiles": 0, "tiles_skipped": 0}


def test_sqrt_and_fp32_modes_on_cpu():
    case = M.randn_case(65, 63, 33, 5)
    adj, xg = M.variant_args(case, "both")
    ref, ref_i = masked_l2nn(case.x, case.y, adj, case.ends, x_group=xg)
    for mode in ("auto", "bf16x1v", "bf16x2v", "native"):
        d, i = masked_l2nn(case.x, case.y, adj, case.ends, x_group=xg, sqrt=True,
                           fp32_mode=mode)
        assert torch.equal(i, ref_i)
        assert torch.equal(d, ref.clamp_min(0).sqrt())
    assert bool(torch.isinf(d[case.truth["both"].none]).all())


def test_empty_inputs():
    x = torch.randn(5, 3)
    y = torch.randn(4, 3)
    ends = torch.tensor([2, 4])
    adj = torch.ones(5, 2, dtype=torch.bool)
    # m = 0
    d, i = masked_l2nn(x[:0], y, adj[:0], ends)
    assert tuple(d.shape) == (0,) and tuple(i.shape) == (0,) and i.dtype == torch.int64
    # n = 0 with empty groups, and G = 0
    for e, a in ((torch.tensor([0, 0]), adj), (torch.tensor([], dtype=torch.int64),
                                               adj[:, :0])):
        d, i, stats = masked_l2nn(x, y[:0], a, e, return_stats=True)
        assert bool(torch.isinf(d).all()) and bool((d > 0).all())
        assert torch.equal(i, torch.full((5,), -1, dtype=torch.int64))
        assert stats == {"rescanned": 0, "tiles": 0, "tiles_skipped": 0}
    # a mask with no bit set
    d, i = masked_l2nn(x, y, torch.zeros(5, 2, dtype=torch.bool), ends)
    assert bool(torch.isinf(d).all()) and bool((i == -1).all())
    # x_group = -1 excludes nothing
    d, i = masked_l2nn(x, y, None, ends, x_group=torch.full((5,), -1))
    d2 = M.d2_fp64(x, y)
    assert torch.equal(i, d2.argmin(1))


def test_argument_errors():
    x = torch.randn(5, 3)
    y = torch.randn(4, 3)
    ends = torch.tensor([2, 4])
    adj = torch.ones(5, 2, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"group_idxs\[-1\]"):
        masked_l2nn(x, y, adj, torch.tensor([2, 3]))
    with pytest.raises(ValueError, match="non-decreasing"):
        masked_l2nn(x, y, torch.ones(5, 3, dtype=torch.bool), torch.tensor([3, 2, 4]))
    with pytest.raises(ValueError, match="shape"):
        masked_l2nn(x, y, torch.ones(5, 3, dtype=torch.bool), ends)
    with pytest.raises(ValueError, match="shape"):
        masked_l2nn(x, y, torch.ones(5, 2, dtype=torch.int32), ends)
    with pytest.raises(ValueError, match="bool"):
        masked_l2nn(x, y, torch.ones(5, 2, dtype=torch.int64), ends)
    with pytest.raises(ValueError, match="adj, x_group or both"):
        masked_l2nn(x, y, None, ends)
    with pytest.raises(ValueError, match="group_idxs"):
        masked_l2nn(x, y, adj)
    with pytest.raises(ValueError, match="feature dimension"):
        masked_l2nn(x, torch.randn(4, 2), adj, ends)
    with pytest.raises(ValueError, match="dtype and device"):
        masked_l2nn(x, y.double(), adj, ends)
    with pytest.raises(ValueError, match="dtype and device"):
        masked_l2nn(x, y.to("meta"), adj, ends)
    with pytest.raises(ValueError, match="x_group"):
        masked_l2nn(x, y, adj, ends, x_group=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="x_group"):
        masked_l2nn(x, y, adj, ends, x_group=torch.zeros(5))
    with pytest.raises(ValueError, match="fp32_mode"):
        masked_l2nn(x, y, adj, ends, fp32_mode="bf16x3")
    with pytest.raises(ValueError, match="labels"):
        cross_component_nn(x, torch.zeros(4, dtype=torch.int64))


def test_cross_component_nn_blobs_and_ties():
    case = M.blobs_case()
    src, dst, dist, comp = cross_component_nn(case.x, case.labels)
    t_src, t_dst, t_dist, t_comp = case.truth
    assert comp.dtype == src.dtype == dst.dtype == torch.int64
    assert torch.equal(comp, t_comp) and comp.numel() == 5
    assert torch.equal(src, t_src) and torch.equal(dst, t_dst)
    assert torch.equal(dist.double(), t_dist)
    # the tie-break decides: several components reach distance 0 over duplicates
    assert int((t_dist == 0).sum()) >= 3
    # a single component (and no point at all) gives an empty result
    for xx, ll in ((case.x, torch.zeros_like(case.labels)),
                   (case.x[:0], case.labels[:0])):
        out = cross_component_nn(xx, ll)
        assert all(o.numel() == 0 for o in out)
        assert out[0].dtype == out[1].dtype == out[3].dtype == torch.int64


def test_boruvka_emst_matches_scipy():
    from scipy.sparse.csgraph import minimum_spanning_tree
    x = M.emst_points()
    edges = M.boruvka_emst(x, cross_component_nn)
    assert len(edges) == x.shape[0] - 1
    d = M.d2_fp64(x, x).sqrt()
    total = sum(float(d[u, v]) for u, v in edges)
    ref = float(minimum_spanning_tree(d.numpy()).sum())
    assert abs(total - ref) <= 1e-6 * ref, (total, ref)


def test_emst_example_matches_scipy():
    """examples/emst_example.py: the vectorised Boruvka loop (pointer-jumping
    merge of sparse/solver/mst.py) gives the scipy tree weight."""
    import importlib.util
    from scipy.sparse.csgraph import minimum_spanning_tree
    spec = importlib.util.spec_from_file_location(
        "emst_example", os.path.join(ROOT, "examples", "emst_example.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x = M.emst_points()
    u, v, w, rounds = mod.emst(x)
    assert u.numel() == x.shape[0] - 1 and 1 <= rounds <= 9
    d = M.d2_fp64(x, x).sqrt()
    total = float(d[u, v].sum())
    ref = float(minimum_spanning_tree(d.numpy()).sum())
    assert abs(total - ref) <= 1e-6 * ref, (total, ref)


def test_masked_launchers_link(tmp_path):
    """The two launchers declared in include/raft_amd/neighbors.hpp must match
    the symbols of the kernel objects (compile + link, no GPU)."""
    objs = sorted(glob.glob(os.path.join(ROOT, "build", "ext", "*.o")))
    objs = [o for o in objs if not o.endswith("bindings.o")]
    if len(objs) < 5:
        pytest.skip("build/ext objects not present (run build_ext.py)")
    src = tmp_path / "consumer.cpp"
    src.write_text(
        "#include <raft_amd/raft_amd.hpp>\n"
        "int main() {\n"
        "  void* fns[] = {\n"
        "    (void*)&raft_amd::launch_masked_l2nn,\n"
        "    (void*)&raft_amd::launch_masked_l2nn_verify_repair,\n"
        "  };\n"
        "  for (void* f : fns) if (!f) return 1;\n"
        "  return 0;\n"
        "}\n")
    obj = str(tmp_path / "consumer.o")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
                        "-c", str(src), f"-I{os.path.join(ROOT, 'include')}",
                        "-o", obj], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run(["hipcc", obj, *objs, "-L/opt/rocm/lib", "-lrocblas",
                        "-lhipblaslt", "-o", str(tmp_path / "consumer")],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
