"""Epsilon-neighborhood: CPU oracle path, API contract, header link check."""
import glob
import os
import subprocess

import pytest
import torch

import eps_inputs as E
from raft_amd.neighbors import eps_neighbors_l2sq, eps_neighbors_l2sq_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_forms(x, y, eps, **kw):
    adj, vd = eps_neighbors_l2sq(x, y, eps, **kw)
    words, vd_w = eps_neighbors_l2sq(x, y, eps, packed=True, **kw)
    csr = eps_neighbors_l2sq_csr(x, y, eps, **kw)
    assert torch.equal(vd, vd_w)
    m = x.shape[0]
    n = (x if y is None else y).shape[0]
    E.check_contract(adj, words, csr, vd, m, n, x.device.type)
    return adj, vd, csr


class TestCpuOracle:
    def test_truth_matches_cdist(self):
        x, y, d2, _, _ = E.randn_case(65, 63, 33)
        ref = torch.cdist(x.double(), y.double(),
                          compute_mode="donot_use_mm_for_euclid_dist") ** 2
        assert torch.allclose(d2, ref, rtol=1e-12, atol=1e-12)

    @pytest.mark.parametrize("shape", E.SHAPES, ids=lambda s: "x".join(map(str, s)))
    def test_randn_vs_fp64(self, shape):
        x, y, d2, band, eps_list = E.randn_case(*shape)
        for eps in eps_list:
            adj, _, _ = _all_forms(x, y, eps)
            E.compare_outside_band(adj, d2, band, eps)

    def test_fp64_input_is_exact(self):
        x, y, d2, _, eps_list = E.randn_case(65, 63, 33)
        adj, _ = eps_neighbors_l2sq(x.double(), y.double(), eps_list[1])
        assert torch.equal(adj, d2 <= eps_list[1])

    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
    def test_exact_ties_included(self, dtype):
        x, y, d2 = E.tie_case()
        on_boundary = int((d2 == E.TIE_EPS).sum())
        assert on_boundary == 130
        adj, vd, _ = _all_forms(x.to(dtype), y.to(dtype), E.TIE_EPS)
        assert torch.equal(adj, d2 <= E.TIE_EPS)
        assert int(vd[-1]) == int((d2 <= E.TIE_EPS).sum())

    def test_duplicates_at_zero_radius(self):
        x, y, d2 = E.duplicate_case()
        adj, vd, _ = _all_forms(x, y, 0.0)
        assert torch.equal(adj, d2 == 0)
        assert int(vd[-1]) >= 4

    def test_offset_cloud(self):
        x, y, d2, band, eps = E.offset_cloud_case()
        assert y.shape[0] == 637
        adj, _, _ = _all_forms(x, y, eps)
        E.compare_outside_band(adj, d2, band, eps)


class TestContract:
    def test_self_join_sets_diagonal(self):
        g = torch.Generator().manual_seed(5)
        x = 100 + torch.randn(70, 33, generator=g)
        for eps in (0.0, 1e-3, 60.0):
            adj, vd, _ = _all_forms(x, None, eps)
            assert bool(adj.diagonal().all())
            assert torch.equal(adj, adj.t())
        adj, vd = eps_neighbors_l2sq(x, None, 0.0)
        assert int(vd[-1]) == 70

    def test_negative_radius_is_empty(self):
        x, y, _ = E.tie_case()
        for yy in (y, None):
            adj, vd, (indptr, indices, _) = _all_forms(x, yy, -1.0)
            assert not bool(adj.any())
            assert int(vd.sum()) == 0
            assert indices.numel() == 0
            assert torch.equal(indptr, torch.zeros(x.shape[0] + 1, dtype=torch.int64))

    def test_trailing_empty_rows_keep_indptr_length(self):
        x, y, d2 = E.duplicate_case()
        # rows after the last duplicate holder (x row 129) do not exist, rows
        # 78..128 are empty: indptr still has m + 1 entries and stays flat
        indptr, indices, vd = eps_neighbors_l2sq_csr(x[:129], y, 0.0)
        assert indptr.shape[0] == 130
        assert int(indptr[-1]) == indices.numel() == int((d2[:129] == 0).sum())
        assert torch.equal(indptr[79:], indptr[78].expand(51))

    def test_infinite_radius_is_full(self):
        x, y, _ = E.tie_case()
        adj, vd, _ = _all_forms(x, y, float("inf"))
        assert bool(adj.all())
        assert int(vd[-1]) == x.shape[0] * y.shape[0]
        assert torch.equal(vd[:-1], torch.full((130,), 200, dtype=torch.int64))

    def test_chunking_does_not_change_results(self):
        x, y, _, _, eps_list = E.randn_case(257, 300, 64)
        ref = _all_forms(x, y, eps_list[1])
        for rc in (1, 100, 128, 256):
            got = _all_forms(x, y, eps_list[1], row_chunk=rc)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
            assert torch.equal(got[2][1], ref[2][1])

    def test_workspace_limit_drives_chunking(self):
        from raft_amd.core.resources import Resources
        x, y, _, _, eps_list = E.randn_case(257, 300, 64)
        ref = eps_neighbors_l2sq_csr(x, y, eps_list[0])
        res = Resources(torch.device("cpu"))
        res.set_workspace_limit(8000)       # bitmap row = 40 B -> 100-row chunks
        got = eps_neighbors_l2sq_csr(x, y, eps_list[0], res=res)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
        assert res.get_workspace_resource().outstanding_bytes() == 0

    def test_stats(self):
        x, y, _ = E.tie_case()
        adj, vd, stats = eps_neighbors_l2sq(x, y, E.TIE_EPS, return_stats=True)
        assert stats == {"rechecked": 0}

    def test_bad_arguments_raise(self):
        x = torch.zeros(4, 8)
        with pytest.raises(ValueError):
            eps_neighbors_l2sq(x, torch.zeros(5, 7), 1.0)
        with pytest.raises(ValueError):
            eps_neighbors_l2sq_csr(x, torch.zeros(5, 7), 1.0)
        with pytest.raises(ValueError):
            eps_neighbors_l2sq(x, x, 1.0, fp32_mode="bf16x9")
        with pytest.raises(TypeError):
            eps_neighbors_l2sq(x, x)

    def test_empty_inputs(self):
        x = torch.zeros(0, 8)
        y = torch.zeros(5, 8)
        adj, vd = eps_neighbors_l2sq(x, y, 1.0)
        assert tuple(adj.shape) == (0, 5) and vd.tolist() == [0]
        adj, vd = eps_neighbors_l2sq(y, x, 1.0)
        assert tuple(adj.shape) == (5, 0) and vd.tolist() == [0] * 6
        indptr, indices, _ = eps_neighbors_l2sq_csr(y, x, 1.0)
        assert indptr.tolist() == [0] * 6 and indices.numel() == 0


def test_new_launchers_link(tmp_path):
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
        "    (void*)&raft_amd::launch_eps_neighbors_l2sq,\n"
        "    (void*)&raft_amd::launch_bitmap_rows_to_csr,\n"
        "    (void*)&raft_amd::launch_bitmap_row_degrees,\n"
        "    (void*)&raft_amd::launch_bitmap_rows_expand,\n"
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
