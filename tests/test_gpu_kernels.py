"""GPU numerics tests: every native HIP kernel vs a plain PyTorch fp32/fp64
reference (the pattern the reference uses in cpp/tests with naive kernels).
All tests here REQUIRE the native extension — no silent fallback.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


class TestReductions:
    @pytest.mark.parametrize("shape", [(8, 3), (100, 64), (33, 257), (5, 100000), (3000, 512)])
    @pytest.mark.parametrize("op", [0, 1, 2, 3, 4])
    def test_reduce_rows(self, dev, ext, shape, op):
        torch.manual_seed(0)
        x = torch.randn(shape, device=dev)
        out = ext.reduce_rows(x, op)
        xr = x.double()
        ref = {0: xr.sum(1), 1: (xr * xr).sum(1), 2: xr.abs().sum(1),
               3: xr.max(1).values, 4: xr.min(1).values}[op]
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-4)

    def test_reduce_rows_kahan_long(self, dev, ext):
        """D = 2^17: Kahan-compensated fp32 sum must track fp64."""
        torch.manual_seed(1)
        x = torch.randn(4, 1 << 17, device=dev)
        out = ext.reduce_rows(x, 0)
        ref = x.double().sum(1)
        torch.testing.assert_close(out.double(), ref, rtol=1e-6, atol=1e-3)

    @pytest.mark.parametrize("shape", [(64, 100), (1000, 513), (100000, 17)])
    @pytest.mark.parametrize("op", [0, 1])
    def test_reduce_cols(self, dev, ext, shape, op):
        torch.manual_seed(2)
        x = torch.randn(shape, device=dev)
        out = ext.reduce_cols(x, op)
        xr = x.double()
        ref = {0: xr.sum(0), 1: (xr * xr).sum(0)}[op]
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-4)

    @pytest.mark.parametrize("op", [0, 3, 4])
    def test_reduce_cols_tall_skinny_atomic_path(self, dev, ext, op):
        """d << 256 forces the multi-row-tile grid (atomic combine across
        tiles incl. the CAS min/max path)."""
        torch.manual_seed(3)
        x = torch.randn(1_000_000, 8, device=dev)
        out = ext.reduce_cols(x, op)
        xr = x.double()
        ref = {0: xr.sum(0), 3: xr.max(0).values, 4: xr.min(0).values}[op]
        torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-3)

    def test_row_argmin(self, dev, ext):
        torch.manual_seed(3)
        x = torch.randn(5000, 777, device=dev)
        out = ext.row_argmin(x)
        assert torch.equal(out.long(), x.argmin(dim=1))

    def test_row_normalize(self, dev, ext):
        torch.manual_seed(4)
        x = torch.randn(300, 1000, device=dev)
        out = ext.row_normalize_l2(x, 1e-12)
        torch.testing.assert_close(out.norm(dim=1), torch.ones(300, device=dev),
                                   rtol=1e-5, atol=1e-5)

    def test_python_dispatch_uses_ext(self, dev):
        from raft_amd import linalg
        x = torch.randn(64, 128, device=dev)
        out = linalg.row_norm(x)
        torch.testing.assert_close(out, x.norm(dim=1), rtol=1e-5, atol=1e-5)


class TestPairwiseGpu:
    def test_l2_epilogue_and_pairwise(self, dev):
        from raft_amd.distance import pairwise_distance, DistanceType
        torch.manual_seed(0)
        x = torch.randn(500, 77, device=dev)
        y = torch.randn(300, 77, device=dev)
        d = pairwise_distance(x, y, DistanceType.L2Expanded)
        ref = torch.cdist(x.double(), y.double()) ** 2
        torch.testing.assert_close(d.double(), ref, rtol=1e-3, atol=1e-3)

    def test_pairwise_bf16x3_engine(self, dev):
        from raft_amd.distance import pairwise_distance, DistanceType
        torch.manual_seed(1)
        x = torch.randn(256, 128, device=dev)
        y = torch.randn(128, 128, device=dev)
        d3 = pairwise_distance(x, y, DistanceType.L2Expanded, fp32_mode="bf16x3")
        ref = torch.cdist(x.double(), y.double()) ** 2
        # fp32-class accuracy from the split-bf16 MFMA engine
        torch.testing.assert_close(d3.double(), ref, rtol=5e-3, atol=5e-3)

    @pytest.mark.parametrize("code,metric", [(0, "l1"), (1, "linf")])
    def test_unexpanded(self, dev, code, metric):
        from raft_amd.distance import pairwise_distance
        torch.manual_seed(2)
        x = torch.randn(200, 50, device=dev)
        y = torch.randn(150, 50, device=dev)
        d = pairwise_distance(x, y, metric)
        ref = torch.cdist(x.double(), y.double(), p=1 if metric == "l1" else float("inf"))
        torch.testing.assert_close(d.double(), ref, rtol=1e-4, atol=1e-4)

    def test_l2nn_epilogue_fused(self, dev):
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        torch.manual_seed(3)
        x = torch.randn(10000, 64, device=dev)
        y = torch.randn(1024, 64, device=dev)
        dmin, amin = fused_l2nn(x, y, fp32_mode="native")
        ref = torch.cdist(x.double(), y.double()) ** 2
        rd, ra = ref.min(dim=1)
        assert (amin == ra).float().mean() > 0.999  # ties may differ
        torch.testing.assert_close(dmin.double(), rd, rtol=1e-3, atol=1e-3)

    def test_l2nn_bf16x3_assignment_agreement(self, dev):
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        torch.manual_seed(4)
        x = torch.randn(20000, 256, device=dev)
        y = torch.randn(1024, 256, device=dev)
        _, a3 = fused_l2nn(x, y, fp32_mode="bf16x3")
        _, an = fused_l2nn(x, y, fp32_mode="native")
        assert (a3 == an).float().mean() > 0.999


class TestFusedL2NNMfma:
    """The fused split-bf16 MFMA kernel vs torch/cdist references."""

    @pytest.mark.parametrize("mode,min_agree,dtol", [("bf16x2", 0.999, 2e-3),
                                                     ("bf16x3", 0.9999, 2e-4)])
    def test_vs_fp64_reference(self, dev, ext, mode, min_agree, dtol):
        torch.manual_seed(0)
        x = torch.randn(4096, 128, device=dev)
        y = torch.randn(512, 128, device=dev)
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        dmin, amin = fused_l2nn(x, y, fp32_mode=mode)
        ref = torch.cdist(x.double(), y.double()) ** 2
        rd, ra = ref.min(dim=1)
        assert (amin == ra).float().mean() > min_agree
        rel = ((dmin.double() - rd).abs() / rd.clamp_min(1e-2)).median()
        assert float(rel) < dtol

    def test_unaligned_rows_and_padded_cols(self, dev, ext):
        """m not multiple of 128, n not multiple of 128 (padding path)."""
        torch.manual_seed(1)
        x = torch.randn(1111, 64, device=dev)
        y = torch.randn(200, 64, device=dev)
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        dmin, amin = fused_l2nn(x, y, fp32_mode="bf16x3")
        ref = torch.cdist(x.double(), y.double()) ** 2
        rd, ra = ref.min(dim=1)
        assert (amin == ra).float().mean() > 0.999
        assert (amin < 200).all()  # padded columns never win

    def test_unaligned_d_fallback(self, dev, ext):
        """d % 64 != 0 cannot use the MFMA tile staging -> the chunked
        expanded-GEMM fallback must produce the same argmin."""
        torch.manual_seed(8)
        x = torch.randn(3000, 100, device=dev)
        y = torch.randn(300, 100, device=dev)
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        dmin, amin = fused_l2nn(x, y, fp32_mode="bf16x3")
        ref = torch.cdist(x.double(), y.double()) ** 2
        assert (amin == ref.argmin(dim=1)).float().mean() > 0.999

    def test_bf16_input_path(self, dev, ext):
        torch.manual_seed(2)
        x = torch.randn(2048, 128, device=dev).bfloat16()
        y = torch.randn(256, 128, device=dev).bfloat16()
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        dmin, amin = fused_l2nn(x, y)
        ref = torch.cdist(x.double(), y.double()) ** 2
        rd, ra = ref.min(dim=1)
        assert (amin == ra).float().mean() > 0.99

    @pytest.mark.parametrize("vmode", ["bf16x2v", "bf16x1v"])
    def test_verified_mode_exact_on_adversarial_ties(self, dev, ext, vmode):
        """Verified modes must produce the exact fp32 argmin even with
        near-duplicate centroids (margins far inside the split-emulation
        error). bf16x1v's emulation is 2^6 coarser — same guarantee, its
        wider bound just routes more rows through the exact rescan."""
        torch.manual_seed(5)
        x = torch.randn(8192, 128, device=dev) * 10
        y = torch.randn(256, 128, device=dev) * 10
        # make half the centroids near-duplicates of the other half
        y[128:] = y[:128] + torch.randn(128, 128, device=dev) * 1e-4
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        _, av = fused_l2nn(x, y, fp32_mode=vmode)
        # the meaningful guarantee: the chosen centroid's TRUE distance is
        # fp32-indistinguishable from the optimum for every row (near-tie
        # winners may differ between any two fp32 summation orders, including
        # the native engine's own expanded form)
        ref = torch.cdist(x.double(), y.double()) ** 2
        opt = ref.min(dim=1).values
        chosen = ref[torch.arange(8192, device=dev), av]
        assert float((chosen - opt).max()) < 1e-2
        # and on rows with a clear margin the argmin is exactly the optimum
        margin_ok = (torch.topk(ref, 2, dim=1, largest=False).values.diff(dim=1)
                     .squeeze(1) > 1.0)
        assert (av[margin_ok] == ref.argmin(dim=1)[margin_ok]).all()

    @pytest.mark.parametrize("vmode", ["bf16x2v", "bf16x1v"])
    def test_verified_mode_exact_distances(self, dev, ext, vmode):
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        torch.manual_seed(6)
        x = torch.randn(4096, 256, device=dev)
        y = torch.randn(512, 256, device=dev)
        dv, av = fused_l2nn(x, y, fp32_mode=vmode)
        ref = torch.cdist(x.double(), y.double()) ** 2
        rd = ref[torch.arange(4096, device=dev), av]
        # distances are exact-fp32 recomputed: error = fp32 rounding only
        rel = ((dv.double() - rd).abs() / rd.clamp_min(1e-3)).max()
        assert float(rel) < 1e-4, float(rel)

    def test_2d_xcd_engine_at_scale(self, dev, ext):
        """m >= 1M, n >= 512 routes to the 2D XCD-swizzled tile-pair engine
        (fused_l2nn_2d_kernel + partials combine) by default — verify it on
        sampled rows against an exact fp64 reference, including dmin2."""
        torch.manual_seed(7)
        m, n, d = 1_000_100, 512, 128   # odd m exercises the edge row tile
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        x = torch.randn(m, d, device=dev)
        y = torch.randn(n, d, device=dev)
        dmin, amin = fused_l2nn(x, y, fp32_mode="bf16x2v")
        idx = torch.randperm(m, device=dev)[:2000]
        idx = torch.cat([idx, torch.arange(m - 130, m, device=dev)])  # tail rows
        ref = torch.cdist(x[idx].double(), y.double()) ** 2
        rd, ra = ref.min(dim=1)
        chosen = ref[torch.arange(idx.numel(), device=dev), amin[idx]]
        assert float((chosen - rd).max()) < 1e-2          # argmin fp32-exact
        rel = ((dmin[idx].double() - rd).abs() / rd.clamp_min(1e-3)).max()
        assert float(rel) < 1e-4                          # exact distances

    def test_blob_data_agreement_is_exact(self, dev, ext):
        """On clustered data (the bench workload) assignments must match
        native fp32 exactly for both split modes."""
        from raft_amd.random import make_blobs, RngState
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        x, _, centers = make_blobs(100000, 256, n_clusters=1024, cluster_std=1.0,
                                   state=RngState(seed=7), device=dev)
        c = centers + 0.3
        _, an = fused_l2nn(x, c, fp32_mode="native")
        for mode, bar in (("bf16x2", 0.9999), ("bf16x3", 0.9999),
                          ("bf16x2v", 1.0), ("bf16x1v", 1.0)):
            _, am = fused_l2nn(x, c, fp32_mode=mode)
            agree = float((am == an).float().mean())
            assert agree >= bar, (mode, agree)


class TestPairwiseMfma:
    @pytest.mark.parametrize("mode,tol", [("bf16x2", 3e-3), ("bf16x3", 3e-4)])
    def test_fp32_tile_vs_fp64(self, dev, ext, mode, tol):
        from raft_amd.distance import pairwise_distance, DistanceType
        torch.manual_seed(0)
        x = torch.randn(777, 192, device=dev)   # non-multiple of 128 rows/cols
        y = torch.randn(333, 192, device=dev)
        d = pairwise_distance(x, y, DistanceType.L2Expanded, fp32_mode=mode)
        ref = torch.cdist(x.double(), y.double()) ** 2
        err = (d.double() - ref).abs().max() / ref.abs().max()
        assert float(err) < tol, float(err)

    def test_bf16_tile(self, dev, ext):
        from raft_amd.distance import pairwise_distance, DistanceType
        torch.manual_seed(1)
        x = torch.randn(500, 128, device=dev).bfloat16()
        y = torch.randn(300, 128, device=dev).bfloat16()
        d = pairwise_distance(x, y, DistanceType.L2Expanded)
        ref = torch.cdist(x.double(), y.double()) ** 2
        err = (d.double() - ref).abs().max() / ref.abs().max()
        assert float(err) < 2e-2, float(err)

    def test_sqrt_variant(self, dev, ext):
        from raft_amd.distance import pairwise_distance, DistanceType
        x = torch.randn(256, 64, device=dev)
        d = pairwise_distance(x, x, DistanceType.L2SqrtExpanded, fp32_mode="bf16x3")
        assert d.diagonal().abs().max() < 1e-2
        torch.testing.assert_close(d, d.t(), rtol=1e-3, atol=1e-3)


class TestRngGpu:
    def test_uniform_bitwise_matches_cpu(self, dev, ext):
        from raft_amd.random import uniform, RngState
        g = uniform((4096,), state=RngState(seed=123), device=dev)
        c = uniform((4096,), state=RngState(seed=123), device="cpu")
        assert torch.equal(g.cpu(), c)

    def test_normal_bitwise_matches_cpu(self, dev, ext):
        from raft_amd.random import normal, RngState
        g = normal((4096,), state=RngState(seed=7), device=dev)
        c = normal((4096,), state=RngState(seed=7), device="cpu")
        torch.testing.assert_close(g.cpu(), c, rtol=0, atol=1e-6)

    def test_make_blobs_gpu_matches_cpu(self, dev, ext):
        from raft_amd.random import make_blobs, RngState
        xg, yg, cg = make_blobs(2000, 32, n_clusters=7, cluster_std=0.5,
                                state=RngState(seed=5), device=dev)
        xc, yc, cc = make_blobs(2000, 32, n_clusters=7, cluster_std=0.5,
                                state=RngState(seed=5), device="cpu")
        assert torch.equal(yg.cpu(), yc)
        torch.testing.assert_close(xg.cpu(), xc, rtol=1e-5, atol=1e-5)

    def test_moments(self, dev, ext):
        from raft_amd.random import uniform, normal, RngState
        u = uniform((1000000,), state=RngState(seed=1), device=dev)
        assert abs(u.mean().item() - 0.5) < 0.005
        z = normal((1000000,), state=RngState(seed=2), device=dev)
        assert abs(z.mean().item()) < 0.01 and abs(z.std().item() - 1) < 0.01


class TestSelectKGpu:
    @pytest.mark.parametrize("batch,n,k", [(32, 1000, 10), (4, 100000, 64),
                                           (128, 512, 256), (2, 1000000, 100),
                                           (16, 2048, 1024), (20000, 500, 32),
                                           (128, 500, 64), (64, 65, 64)])
    def test_vs_topk(self, dev, ext, batch, n, k):
        from raft_amd.matrix import select_k
        torch.manual_seed(0)
        x = torch.randn(batch, n, device=dev)
        vals, idx = select_k(x, k, select_min=True)
        ref_v, _ = torch.topk(x, k, dim=1, largest=False)
        torch.testing.assert_close(vals, ref_v)
        torch.testing.assert_close(torch.gather(x, 1, idx), vals)

    def test_select_max(self, dev, ext):
        from raft_amd.matrix import select_k
        x = torch.randn(10, 5000, device=dev)
        vals, idx = select_k(x, 32, select_min=False)
        ref_v, _ = torch.topk(x, 32, dim=1, largest=True)
        torch.testing.assert_close(vals, ref_v)

    def test_duplicates_short_row_warpsort(self, dev, ext):
        """short-row path (native warpsort): duplicate minima straddling k."""
        from raft_amd.matrix import select_k
        x = torch.zeros(5, 300, device=dev)
        x[:, :40] = -1.0
        vals, idx = select_k(x, 64, select_min=True)
        assert (vals[:, :40] == -1).all() and (vals[:, 40:] == 0).all()
        for r in range(5):
            assert idx[r].unique().numel() == 64

    def test_duplicates_at_kth(self, dev, ext):
        """k = 100 > 64 at n = 1000 <= 4096 is dispatched to the vendor top-k
        (torch.topk), as are (128, 512, 256) and (16, 2048, 1024) above: no
        native kernel runs here. Ties at the k-th value on the native engines
        are covered in tests/test_gpu_select_k.py."""
        from raft_amd.matrix import select_k
        x = torch.zeros(3, 1000, device=dev)
        x[:, :50] = -1.0  # 50 identical minima, k straddles them
        vals, idx = select_k(x, 100, select_min=True)
        assert (vals[:, :50] == -1).all()
        assert (vals[:, 50:] == 0).all()
        # indices must be valid and unique per row
        for r in range(3):
            assert idx[r].unique().numel() == 100


class TestSparseGpu:
    def test_spmv(self, dev, ext):
        from raft_amd.sparse import CSR, spmv
        torch.manual_seed(0)
        dense = torch.randn(500, 400, device=dev)
        dense[torch.rand_like(dense) > 0.05] = 0
        csr = CSR.from_dense(dense)
        x = torch.randn(400, device=dev)
        y = spmv(csr, x)
        torch.testing.assert_close(y.double(), dense.double() @ x.double(),
                                   rtol=1e-4, atol=1e-4)

    def test_spmv_empty_rows(self, dev, ext):
        from raft_amd.sparse import CSR, spmv
        dense = torch.zeros(100, 50, device=dev)
        dense[0, 0] = 2.0
        csr = CSR.from_dense(dense)
        y = spmv(csr, torch.ones(50, device=dev))
        assert y[0] == 2.0 and y[1:].abs().sum() == 0

    def test_lanczos_gpu(self, dev, ext):
        from raft_amd.sparse import CSR
        from raft_amd.sparse.solver import eigsh
        torch.manual_seed(1)
        a = torch.randn(300, 300, device=dev)
        a = (a + a.t()) / 2
        mask = torch.rand_like(a) > 0.9
        a = a * (mask | mask.t()).float()
        a = a + 10 * torch.eye(300, device=dev)
        csr = CSR.from_dense(a)
        w, v = eigsh(csr, k=4, tol=1e-8)
        ref = torch.linalg.eigvalsh(a.double())[:4]
        torch.testing.assert_close(w.double(), ref, rtol=1e-4, atol=1e-4)


class TestKMeansGpu:
    def test_reduce_rows_by_key(self, dev, ext):
        from raft_amd.linalg import reduce_rows_by_key
        torch.manual_seed(0)
        x = torch.randn(10000, 64, device=dev)
        keys = torch.randint(0, 100, (10000,), device=dev)
        out = reduce_rows_by_key(x, keys, 100)
        ref = torch.zeros(100, 64, device=dev, dtype=torch.float64)
        ref.index_add_(0, keys, x.double())
        torch.testing.assert_close(out.double(), ref, rtol=1e-4, atol=1e-3)

    def test_kmeans_fit_gpu(self, dev, ext):
        from raft_amd.cluster import kmeans_fit, KMeansParams
        from raft_amd.random import make_blobs, RngState
        x, _, centers = make_blobs(50000, 32, n_clusters=16, cluster_std=0.3,
                                   center_box=(-20, 20), state=RngState(seed=2),
                                   device=dev)
        model = kmeans_fit(x, KMeansParams(n_clusters=16, max_iter=30, seed=0,
                                           init="kmeans++", fp32_mode="bf16x3"))
        d = torch.cdist(centers, model.centroids)
        assert d.min(dim=1).values.max() < 1.0

    @pytest.mark.parametrize("vmode", ["bf16x2v", "bf16x1v", "auto"])
    def test_fast_iterate_matches_cpu(self, dev, ext, vmode):
        """the minimal-dispatch fused EM loop (k % 128 == 0) vs CPU oracle —
        both verified engines (2-slice tight bound, 1-slice wide bound) plus
        the adaptive auto engine (starts 1-product, widens on rescan rate)."""
        from raft_amd.cluster.kmeans import kmeans_iterate
        from raft_amd.random import make_blobs, RngState
        x, _, centers = make_blobs(20000, 64, n_clusters=128, cluster_std=0.4,
                                   state=RngState(seed=9), device=dev)
        c0 = centers + 0.2
        cg, ig = kmeans_iterate(x, c0.clone(), 3, fp32_mode=vmode)
        cc, ic = kmeans_iterate(x.cpu(), c0.cpu().clone(), 3)
        torch.testing.assert_close(cg.cpu(), cc, rtol=1e-3, atol=1e-3)
        assert abs(ig - ic) / ic < 1e-3

    def test_fast_path_any_d_padding(self, dev, ext):
        """d % 64 != 0 now pads feature columns with zeros and takes the
        fused engines (distances unchanged) — kmeans and fused_l2nn must
        match the CPU oracle at d=100."""
        from raft_amd.cluster.kmeans import kmeans_iterate
        from raft_amd.neighbors.fused_l2nn import fused_l2nn
        from raft_amd.random import make_blobs, RngState
        x, _, centers = make_blobs(20000, 100, n_clusters=96, cluster_std=0.3,
                                   state=RngState(seed=14), device=dev)
        c0 = centers + 0.2
        cg, ig = kmeans_iterate(x, c0.clone(), 3, fp32_mode="auto")
        assert cg.shape == (96, 100)
        cc, ic = kmeans_iterate(x.cpu(), c0.cpu().clone(), 3)
        torch.testing.assert_close(cg.cpu(), cc, rtol=1e-3, atol=1e-3)
        assert abs(ig - ic) / ic < 1e-3
        d1, a1 = fused_l2nn(x, c0)
        ref = torch.cdist(x.double(), c0.double()) ** 2
        rd, ra = ref.min(dim=1)
        assert (a1 == ra).float().mean() > 0.999
        rel = ((d1.double() - rd).abs() / rd.clamp_min(1e-3)).max()
        assert float(rel) < 1e-4

    @pytest.mark.parametrize("k", [100, 1000])
    def test_fast_iterate_any_k_padding(self, dev, ext, k):
        """ANY k now takes the minimal-dispatch fast path (centroids padded
        to a 128 multiple with +inf-norm zero rows) — results must match the
        CPU oracle exactly like the k%128==0 case."""
        from raft_amd.cluster.kmeans import kmeans_iterate
        from raft_amd.random import make_blobs, RngState
        x, _, centers = make_blobs(20000, 64, n_clusters=k, cluster_std=0.3,
                                   state=RngState(seed=13), device=dev)
        c0 = centers + 0.2
        cg, ig = kmeans_iterate(x, c0.clone(), 3, fp32_mode="auto")
        assert cg.shape == (k, 64)
        cc, ic = kmeans_iterate(x.cpu(), c0.cpu().clone(), 3)
        torch.testing.assert_close(cg.cpu(), cc, rtol=1e-3, atol=1e-3)
        assert abs(ig - ic) / ic < 1e-3

    def test_adaptive_auto_engine_decisions(self, dev, ext):
        """fp32_mode="auto" stays on the 1-product engine on well-separated
        data and widens to the 2-slice engine on near-tie-heavy data; both
        paths stay exact (every verified engine rescans uncertain rows in
        exact fp32, so results agree across engines)."""
        import raft_amd.cluster.kmeans as km
        from raft_amd.random import make_blobs, RngState
        # clear margins -> stays on bf16x1v
        x, _, centers = make_blobs(20000, 64, n_clusters=128, cluster_std=0.3,
                                   state=RngState(seed=12), device=dev)
        km.kmeans_iterate(x, (centers + 0.2).clone(), 2, fp32_mode="auto")
        assert km._LAST_ADAPTIVE_NSLICE == 1
        # near-duplicate centroids -> margins collapse -> widens to 2 slices
        torch.manual_seed(11)
        xd = torch.randn(20000, 64, device=dev) * 5
        c0 = torch.randn(128, 64, device=dev) * 5
        c0[64:] = c0[:64] + 1e-5
        ca, ia = km.kmeans_iterate(xd, c0.clone(), 3, fp32_mode="auto")
        assert km._LAST_ADAPTIVE_NSLICE == 2
        # the widened run matches the always-2-slice verified engine
        cv, iv = km.kmeans_iterate(xd, c0.clone(), 3, fp32_mode="bf16x2v")
        assert abs(ia - iv) / iv < 1e-5
        torch.testing.assert_close(ca, cv, rtol=1e-4, atol=1e-4)

    def test_split_norms_and_update_kernels(self, dev, ext):
        torch.manual_seed(10)
        c = torch.randn(256, 192, device=dev)
        s = [torch.empty_like(c, dtype=torch.bfloat16) for _ in range(2)]
        cn = torch.empty(256, device=dev)
        ext.split_bf16_norms(c, s, cn)
        torch.testing.assert_close(cn.double(), (c.double() ** 2).sum(1),
                                   rtol=1e-5, atol=1e-4)
        recon = s[0].float() + s[1].float()
        assert float((recon - c).abs().max()) < 1e-3
        # update kernel
        sums = torch.randn(256, 192, device=dev)
        counts = torch.randint(0, 3, (256,), device=dev).float()
        c2 = c.clone()
        ext.kmeans_update_centroids(sums.contiguous(), counts.contiguous(), c2)
        ref = torch.where((counts > 0).unsqueeze(1), sums / counts.clamp_min(1e-9).unsqueeze(1), c)
        torch.testing.assert_close(c2, ref, rtol=1e-5, atol=1e-6)

    def test_rrbk_sorted_counts(self, dev, ext):
        torch.manual_seed(11)
        x = torch.randn(30000, 64, device=dev)
        keys = torch.randint(0, 100, (30000,), device=dev, dtype=torch.int32)
        ks, perm = torch.sort(keys)
        sums = torch.zeros(100, 64, device=dev)
        counts = torch.zeros(100, device=dev)
        ext.reduce_rows_by_key_sorted_into(x, perm.to(torch.int32), ks, sums, counts)
        ref_counts = torch.bincount(keys.long(), minlength=100).float()
        torch.testing.assert_close(counts, ref_counts)
        ref = torch.zeros(100, 64, device=dev, dtype=torch.float64)
        ref.index_add_(0, keys.long(), x.double())
        torch.testing.assert_close(sums.double(), ref, rtol=1e-4, atol=1e-3)

    def test_kmeans_iterate_matches_cpu(self, dev, ext):
        from raft_amd.cluster.kmeans import kmeans_iterate
        from raft_amd.random import make_blobs, RngState
        x, _, centers = make_blobs(5000, 16, n_clusters=8, cluster_std=0.5,
                                   state=RngState(seed=3), device=dev)
        c0 = centers + 0.3
        cg, ig = kmeans_iterate(x, c0.clone(), 3, fp32_mode="native")
        cc, ic = kmeans_iterate(x.cpu(), c0.cpu().clone(), 3)
        torch.testing.assert_close(cg.cpu(), cc, rtol=1e-3, atol=1e-3)
        assert abs(ig - ic) / ic < 1e-3


class TestGemmGpu:
    def test_gemm_bf16_f32(self, dev, ext):
        torch.manual_seed(0)
        a = torch.randn(128, 256, device=dev).bfloat16()
        b = torch.randn(256, 64, device=dev).bfloat16()
        c = ext.gemm_bf16_f32(a, b)
        ref = a.double() @ b.double()
        torch.testing.assert_close(c.double(), ref, rtol=1e-2, atol=1e-2)
        assert c.dtype == torch.float32

    def test_gemm_beta_accumulate(self, dev, ext):
        a = torch.randn(32, 64, device=dev).bfloat16()
        b = torch.randn(64, 32, device=dev).bfloat16()
        c = ext.gemm_bf16_f32(a, b)
        c2 = ext.gemm_bf16_f32(a, b, c, 1.0)
        torch.testing.assert_close(c2, (a.float() @ b.float()) * 2, rtol=2e-2, atol=2e-2)

    def test_huge_output_gemm_guard(self, dev, ext):
        """Vendor gemm_ex corrupts >= 2^31-element outputs on this stack
        (32-bit C-element indexing — measured). The raft_amd
        wrappers row-chunk below the boundary: a [256 x 20M] C (5.1e9
        elements) must be exact everywhere, INCLUDING the tail rows where
        the unguarded vendor call returns garbage."""
        torch.manual_seed(0)
        a = torch.randn(256, 128, device=dev).bfloat16()
        b = torch.randn(20_000_000, 128, device=dev).bfloat16()
        out = ext.gemm_bf16_f32_nt(a, b)
        cols = torch.randint(0, 20_000_000, (512,),
                             generator=torch.Generator(dev).manual_seed(1),
                             device=dev)
        for r in (0, 128, 255):
            exact = (a[r].float().double().unsqueeze(0)
                     * b[cols].float().double()).sum(1)
            err = float((out[r, cols].double() - exact).abs().max())
            assert err < 1e-3, (r, err)
        del out

    def test_fp32_emulation_gpu_accuracy(self, dev, ext):
        from raft_amd.linalg import gemm_fp32_emulated
        torch.manual_seed(1)
        a = torch.randn(256, 512, device=dev)
        b = torch.randn(512, 128, device=dev)
        ref = a.double() @ b.double()
        err_native = ((a @ b).double() - ref).abs().max()
        err3 = (gemm_fp32_emulated(a, b, "bf16x3").double() - ref).abs().max()
        assert float(err3) < float(err_native) * 8, (float(err3), float(err_native))


class TestSelectKNaN:
    """NaN semantics (documented in matrix/select_k.py): NaN of ANY sign or
    payload canonicalizes to the max ordinal — ordered after every finite
    value and +/-inf in BOTH selection directions; NaN-padded outputs carry
    real in-range indices (no -1 sentinels)."""

    @pytest.mark.parametrize("algo_name", ["radix", "warpsort"])
    @pytest.mark.parametrize("select_min", [True, False])
    def test_nan_never_selected(self, dev, ext, algo_name, select_min):
        from raft_amd.matrix import select_k, SelectAlgo
        torch.manual_seed(0)
        x = torch.randn(8, 6000 if algo_name == "radix" else 500, device=dev)
        x[:, :4] = float("nan")
        # negative-sign NaN: maps below -inf unless canonicalized
        neg_nan = torch.tensor(float("nan"), device=dev).view(torch.int32) \
            | torch.tensor(-0x80000000, device=dev, dtype=torch.int32)
        x[:, 4:7] = neg_nan.view(torch.float32)
        algo = SelectAlgo.RADIX if algo_name == "radix" else SelectAlgo.WARPSORT
        vals, idx = select_k(x, 16, select_min=select_min, algo=algo)
        assert not torch.isnan(vals).any()
        fill = float("inf") if select_min else float("-inf")
        finite = torch.nan_to_num(x, nan=fill, posinf=float("inf"),
                                  neginf=float("-inf"))
        ref = torch.topk(finite, 16, dim=1, largest=not select_min).values
        torch.testing.assert_close(vals, ref)
        assert (idx >= 0).all() and (idx < x.shape[1]).all()

    @pytest.mark.parametrize("algo_name", ["radix", "warpsort"])
    def test_nan_heavy_rows_valid_indices(self, dev, ext, algo_name):
        # rows with FEWER than k finite values: NaNs fill the tail slots and
        # every index must still be in-range (the old warpsort emitted -1)
        from raft_amd.matrix import select_k, SelectAlgo
        torch.manual_seed(1)
        n = 6000 if algo_name == "radix" else 500
        x = torch.full((4, n), float("nan"), device=dev)
        x[:, :5] = torch.randn(4, 5, device=dev)
        algo = SelectAlgo.RADIX if algo_name == "radix" else SelectAlgo.WARPSORT
        vals, idx = select_k(x, 16, select_min=True, algo=algo)
        assert (idx >= 0).all() and (idx < n).all()
        torch.testing.assert_close(vals[:, :5], torch.sort(x[:, :5], dim=1).values)
        assert torch.isnan(vals[:, 5:]).all()


class TestSolverKernelsGpu:
    def test_cholesky_r1_update_single_kernel(self, dev, ext):
        from raft_amd.linalg.decomp import cholesky_r1_update
        torch.manual_seed(0)
        for n, dt in [(64, torch.float64), (257, torch.float32)]:
            a = torch.randn(n, n, dtype=dt, device=dev)
            a = a @ a.t() + n * torch.eye(n, dtype=dt, device=dev)
            x = torch.randn(n, dtype=dt, device=dev)
            l = torch.linalg.cholesky(a)
            l2 = cholesky_r1_update(l, x)
            ref = torch.linalg.cholesky(a + torch.outer(x, x))
            tol = 1e-10 if dt == torch.float64 else 1e-3
            torch.testing.assert_close(l2, ref, rtol=tol, atol=tol)

    def test_lanczos_gpu_residuals(self, dev, ext):
        # default (eager, sync-free) GPU solver: residual check vs scipy CSR
        from raft_amd.sparse.solver.lanczos import eigsh
        from raft_amd.sparse.types import CSR
        import scipy.sparse as sp
        n = 4000
        m = sp.random(n, n, density=2e-3, random_state=3, format="csr")
        m = (m + m.T) * 0.5 + sp.identity(n) * 0.1
        csr = CSR(torch.as_tensor(m.indptr, dtype=torch.int32, device=dev),
                  torch.as_tensor(m.indices, dtype=torch.int32, device=dev),
                  torch.as_tensor(m.data, dtype=torch.float32, device=dev),
                  n, n)
        w, v = eigsh(csr, k=4, maxiter=40)
        av = torch.as_tensor(m @ v.cpu().double().numpy(), device=dev)
        res = (av - v.double() * w.double().unsqueeze(0)).norm(dim=0)
        assert float(res.max()) < 1e-3


class TestSelectKGeneric:
    """Generic select engine: dtypes, unbounded k, int64 idx, CSR rows
    (reference select test matrix: select_radix len_i + CSR adapter)."""

    @pytest.mark.parametrize("dt", [torch.float64, torch.bfloat16, torch.float16])
    @pytest.mark.parametrize("select_min", [True, False])
    def test_dtypes_vs_topk(self, dev, ext, dt, select_min):
        from raft_amd.matrix import select_k
        torch.manual_seed(0)
        x = (torch.randn(64, 3000, device=dev) * 10).to(dt)
        vals, idx = select_k(x, 16, select_min=select_min)
        ref_v, _ = torch.topk(x.float(), 16, dim=1, largest=not select_min)
        torch.testing.assert_close(vals.float(), ref_v, rtol=0, atol=0)
        g = torch.gather(x, 1, idx)
        torch.testing.assert_close(g.float(), vals.float(), rtol=0, atol=0)

    def test_large_k_fp32(self, dev, ext):
        from raft_amd.matrix import select_k
        torch.manual_seed(1)
        x = torch.randn(8, 100000, device=dev)
        vals, idx = select_k(x, 5000, select_min=True)   # k > 2048
        ref_v, _ = torch.topk(x, 5000, dim=1, largest=False)
        torch.testing.assert_close(vals, ref_v, rtol=0, atol=0)
        assert idx.dtype == torch.int64
        torch.testing.assert_close(torch.gather(x, 1, idx), vals)

    def test_csr_no_densify_power_law(self, dev, ext):
        # ragged rows incl. empty and shorter-than-k; compare vs the CPU
        # densify oracle
        from raft_amd.sparse.types import CSR
        from raft_amd.sparse.select_k import csr_select_k
        torch.manual_seed(2)
        lens = torch.tensor([0, 3, 5000, 17, 1, 900, 64, 2], dtype=torch.int64)
        indptr = torch.cat([torch.zeros(1, dtype=torch.int64),
                            lens.cumsum(0)])
        nnz = int(indptr[-1])
        vals = torch.randn(nnz)
        cols = torch.randint(0, 100000, (nnz,))
        a_gpu = CSR(indptr.to(dev).to(torch.int32), cols.to(dev).to(torch.int32),
                    vals.to(dev), 8, 100000)
        a_cpu = CSR(indptr.to(torch.int32), cols.to(torch.int32), vals,
                    8, 100000)
        k = 8
        gv, gi = csr_select_k(a_gpu, k)
        cv, ci = csr_select_k(a_cpu, k)
        torch.testing.assert_close(gv.cpu(), cv, rtol=0, atol=0)
        # where padded (inf), index must be -1; real slots: same VALUES
        # (column ids may differ on duplicate values)
        pad = torch.isinf(cv)
        assert (gi.cpu()[pad] == -1).all()
        assert (gi.cpu()[~pad] >= 0).all()


class TestHistogramBitsetGpu:
    @pytest.mark.parametrize("n,d,bins", [(100000, 8, 256), (50000, 3, 4096),
                                          (20000, 2, 20000)])
    def test_histogram_strategies(self, dev, ext, n, d, bins):
        # 256 and 4096 bins both take LDS-multi (4 waves x 4096 bins x 4 B is
        # exactly the 64 KiB limit), 20000 bins takes gmem; LDS-single (4097
        # to 16384 bins) runs in tests/test_gpu_primitives.py
        torch.manual_seed(0)
        x = torch.rand(n, d, device=dev) * 10 - 5
        out = ext.histogram_f32(x.contiguous(), bins, -5.0, 5.0)
        # reference with the SAME fp32 binning formula
        scale = bins / 10.0
        b = ((x - (-5.0)) * scale).floor().clamp_(0, bins - 1).to(torch.int64)
        ref = torch.zeros(bins, d, dtype=torch.int64, device=dev)
        for j in range(d):
            ref[:, j] = torch.bincount(b[:, j], minlength=bins)
        assert torch.equal(out, ref)

    def test_histogram_python_api(self, dev):
        from raft_amd.stats import histogram
        x = torch.rand(10000, 4, device=dev)
        h = histogram(x, 64)
        assert h.shape == (64, 4)
        assert int(h.sum()) == 40000

    def test_bitset_set_test_count(self, dev, ext):
        from raft_amd.core import Bitset
        n = 1_000_000
        bs = Bitset(n, device=dev, default=False)
        torch.manual_seed(1)
        idx = torch.randint(0, n, (50000,), device=dev)
        bs.set(idx, True)
        uniq = int(idx.unique().numel())
        assert bs.count() == uniq
        assert bool(bs.test(idx).all())
        # clear half
        half = idx[:25000]
        bs.set(half, False)
        assert not bool(bs.test(half).any())
        expect = int(torch.cat([idx.unique(),
                                half.unique()]).unique().numel()) \
            - int(half.unique().numel())
        # remaining = uniq minus cleared uniq that were set
        remaining = int((~torch.isin(idx.unique(), half.unique())).sum())
        assert bs.count() == remaining


class TestLinewiseGpu:
    @pytest.mark.parametrize("along_rows", [True, False])
    @pytest.mark.parametrize("op", ["add", "sub", "mul", "div"])
    def test_matrix_vector_native(self, dev, ext, along_rows, op):
        from raft_amd.linalg.matrix_vector import matrix_vector_op
        torch.manual_seed(0)
        x = torch.randn(333, 129, device=dev)   # odd d -> scalar tail path
        v = torch.rand((129 if along_rows else 333,), device=dev) + 0.5
        out = matrix_vector_op(x, v, op, along_rows)
        ref = getattr(torch, op if op != "div" else "div")(
            x, v.unsqueeze(0 if along_rows else 1))
        torch.testing.assert_close(out, ref)

    @pytest.mark.parametrize("along_rows", [True, False])
    def test_linewise_fused_standardize(self, dev, ext, along_rows):
        from raft_amd.linalg.matrix_vector import linewise_fused
        torch.manual_seed(1)
        x = torch.randn(1000, 256, device=dev)
        n = 256 if along_rows else 1000
        mu = torch.randn(n, device=dev)
        sig = torch.rand(n, device=dev) + 0.5
        out = linewise_fused(x, mu, "sub", sig, "div", along_rows)
        mu_b = mu.unsqueeze(0 if along_rows else 1)
        sig_b = sig.unsqueeze(0 if along_rows else 1)
        torch.testing.assert_close(out, (x - mu_b) / sig_b)


class TestPhiloxGpu:
    def test_philox_bitwise_cpu_gpu(self, dev, ext):
        from raft_amd.random.rng import RngState, uniform
        sg = RngState(seed=77, gen_type="philox")
        sc = RngState(seed=77, gen_type="philox")
        g = uniform((40000,), state=sg, device=dev)
        c = uniform((40000,), state=sc, device="cpu")
        assert torch.equal(g.cpu(), c.float())

    def test_device_sampling_proportional(self, dev, ext):
        # block_random_sample: empirical pick frequency must track weights
        w = torch.zeros(256, device=dev)
        w[10] = 1.0
        w[20] = 2.0
        w[200] = 4.0
        draws = ext.device_sample_test(w, 70000, 123)
        counts = torch.bincount(draws.long(), minlength=256).float()
        assert counts[[10, 20, 200]].sum() == 70000  # zero-weight never picked
        p = counts / 70000
        assert abs(p[10] - 1 / 7) < 0.02
        assert abs(p[20] - 2 / 7) < 0.02
        assert abs(p[200] - 4 / 7) < 0.02


class TestSddmmGpu:
    @pytest.mark.parametrize("d", [8, 32, 100, 256])
    def test_sddmm_vs_dense(self, dev, ext, d):
        import scipy.sparse as sp
        from raft_amd.sparse.types import CSR
        from raft_amd.sparse.linalg import sddmm
        torch.manual_seed(d)
        m, n = 500, 400
        mask_sp = sp.random(m, n, density=0.02, random_state=d, format="csr")
        mask = CSR(torch.as_tensor(mask_sp.indptr, dtype=torch.int32, device=dev),
                   torch.as_tensor(mask_sp.indices, dtype=torch.int32, device=dev),
                   torch.ones(mask_sp.nnz, device=dev), m, n)
        a = torch.randn(m, d, device=dev)
        b = torch.randn(n, d, device=dev)
        out = sddmm(a, b, mask)
        dense = (a @ b.t())
        rows = torch.repeat_interleave(
            torch.arange(m, device=dev),
            (mask.indptr[1:] - mask.indptr[:-1]).to(torch.int64))
        ref = dense[rows, mask.indices.to(torch.int64)]
        torch.testing.assert_close(out.values, ref, rtol=1e-4, atol=1e-4)
