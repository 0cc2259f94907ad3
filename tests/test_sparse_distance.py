"""Sparse (CSR) pairwise distances and sparse brute-force kNN: the CPU oracle
path, the API contract and the header link check."""
import glob
import os
import subprocess

import pytest
import torch

import sparse_dist_inputs as S
from raft_amd.distance import pairwise_distance
from raft_amd.neighbors.brute_force import knn
from raft_amd.sparse import (CSR, csr_to_dense, sparse_knn, sparse_pairwise_distance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (5, 7, 33), (17, 9, 300)]
TOL = dict(rtol=1e-12, atol=1e-12)


def dense_ref(a, b, metric, p=2.0):
    return pairwise_distance(csr_to_dense(a), csr_to_dense(b), metric, p=p)


@pytest.mark.parametrize("m,n,d", SHAPES)
@pytest.mark.parametrize("metric,p", S.METRICS, ids=S.METRIC_IDS)
def test_matches_dense(metric, p, m, n, d):
    a = S.random_csr(m, d, 0.1, 1, S.kind_for(metric), fill_first=False)
    b = S.random_csr(n, d, 0.1, 2, S.kind_for(metric), fill_first=False)
    got = sparse_pairwise_distance(a, b, metric, p)
    assert got.dtype == torch.float64 and got.shape == (m, n)
    torch.testing.assert_close(got, dense_ref(a, b, metric, p), **TOL)


def test_string_and_enum_metric_agree():
    from raft_amd.distance import DistanceType
    a = S.random_csr(6, 40, 0.2, 3)
    assert torch.equal(sparse_pairwise_distance(a, a, "cosine"),
                       sparse_pairwise_distance(a, a, DistanceType.CosineExpanded))


def test_fp32_input_returns_fp32():
    a = S.random_csr(6, 40, 0.2, 3, dtype=torch.float32)
    got = sparse_pairwise_distance(a, None, "l1")
    assert got.dtype == torch.float32
    torch.testing.assert_close(got.double(), dense_ref(S.cast(a, torch.float64),
                                                       S.cast(a, torch.float64), "l1"),
                               rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("metric", ["sqeuclidean", "l1", "canberra", "jaccard"])
def test_self_join_is_b_equals_a(metric):
    a = S.random_csr(9, 50, 0.2, 4, S.kind_for(metric))
    assert torch.equal(sparse_pairwise_distance(a, None, metric),
                       sparse_pairwise_distance(a, a, metric))


@pytest.mark.parametrize("metric,p", S.METRICS, ids=S.METRIC_IDS)
def test_empty_rows(metric, p):
    a = S.with_empty_rows(S.random_csr(8, 60, 0.2, 5, S.kind_for(metric)), [0, 3, 7])
    b = S.with_empty_rows(S.random_csr(6, 60, 0.2, 6, S.kind_for(metric)), [0, 2, 5])
    assert int(a.row_lengths()[3]) == 0 and int(b.row_lengths()[5]) == 0
    torch.testing.assert_close(sparse_pairwise_distance(a, b, metric, p),
                               dense_ref(a, b, metric, p), **TOL)


@pytest.mark.parametrize("metric,p", S.METRICS, ids=S.METRIC_IDS)
def test_all_empty_matrix(metric, p):
    a = S.empty_csr(4, 30)
    b = S.random_csr(5, 30, 0.2, 7, S.kind_for(metric))
    for x, y in ((a, b), (b, a), (a, a)):
        got = sparse_pairwise_distance(x, y, metric, p)
        ref = pairwise_distance(csr_to_dense(x), csr_to_dense(y), metric, p=p)
        torch.testing.assert_close(got, ref, **TOL)


def test_zero_rows():
    a = S.empty_csr(0, 30)
    b = S.random_csr(5, 30, 0.2, 7)
    assert sparse_pairwise_distance(a, b).shape == (0, 5)
    assert sparse_pairwise_distance(b, a).shape == (5, 0)


@pytest.mark.parametrize("metric", ["canberra", "hamming", "l1", "cosine", "jensenshannon"])
def test_stored_zeros_change_nothing(metric):
    g = torch.Generator().manual_seed(8)
    mask = torch.rand(7, 40, generator=g) < 0.3
    vals = (torch.rand(7, 40, generator=g, dtype=torch.float64) + 0.1) * mask
    plain = S.csr_from_mask(mask, vals)
    # the same matrix with explicit zeros stored at extra positions
    extra = mask | (torch.rand(7, 40, generator=g) < 0.3)
    padded = S.csr_from_mask(extra, vals)
    assert padded.nnz > plain.nnz and int((padded.values == 0).sum()) > 0
    ref = sparse_pairwise_distance(plain, plain, metric)
    torch.testing.assert_close(sparse_pairwise_distance(padded, plain, metric), ref, **TOL)
    torch.testing.assert_close(sparse_pairwise_distance(plain, padded, metric), ref, **TOL)
    torch.testing.assert_close(sparse_pairwise_distance(padded, padded, metric), ref, **TOL)


@pytest.mark.parametrize("metric", ["sqeuclidean", "l1", "hamming"])
def test_unsorted_columns(metric):
    a = S.random_csr(9, 50, 0.3, 9)
    b = S.random_csr(6, 50, 0.3, 10)
    au = S.random_csr(9, 50, 0.3, 9, shuffle_seed=1)
    bu = S.random_csr(6, 50, 0.3, 10, shuffle_seed=2)
    assert not torch.equal(a.indices, au.indices)
    torch.testing.assert_close(sparse_pairwise_distance(au, bu, metric),
                               sparse_pairwise_distance(a, b, metric), **TOL)


@pytest.mark.parametrize("metric", S.UNSUPPORTED)
def test_unsupported_metrics_raise(metric):
    a = S.random_csr(4, 2, 0.5, 11)
    with pytest.raises(ValueError, match=metric):
        sparse_pairwise_distance(a, a, metric)
    with pytest.raises(ValueError, match=metric):
        sparse_knn(a, a, 1, metric)


def test_bad_arguments_raise():
    a = S.random_csr(4, 20, 0.5, 12)
    b = S.random_csr(4, 21, 0.5, 13)
    with pytest.raises(ValueError, match="column"):
        sparse_pairwise_distance(a, b)
    with pytest.raises(ValueError, match="strategy"):
        sparse_pairwise_distance(a, a, strategy="sorted")
    with pytest.raises(ValueError, match="hash_capacity"):
        sparse_pairwise_distance(a, a, strategy="hash", hash_capacity=100)
    with pytest.raises(ValueError, match="hash_capacity"):
        sparse_pairwise_distance(a, a, strategy="hash", hash_capacity=1 << 20)
    with pytest.raises(ValueError, match="dense_window"):
        sparse_pairwise_distance(a, a, strategy="dense", dense_window=100)
    with pytest.raises(ValueError, match="dense_window"):
        sparse_pairwise_distance(a, a, strategy="dense", dense_window=1 << 20)
    with pytest.raises(ValueError, match="unknown metric"):
        sparse_pairwise_distance(a, a, "manhattan_ish")
    with pytest.raises(ValueError, match="column"):
        sparse_knn(a, b, 1)
    with pytest.raises(ValueError, match="k="):
        sparse_knn(a, a, 5)


@pytest.fixture(scope="module")
def knn_case():
    index = S.random_csr(120, 64, 0.15, 14)
    queries = S.random_csr(23, 64, 0.15, 15)
    return index, queries, csr_to_dense(index), csr_to_dense(queries)


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine", "l1"])
def test_knn_matches_dense_knn(knn_case, metric):
    index, queries, xd, qd = knn_case
    d_ref, _ = knn(xd, qd, 7, metric=metric)
    true = pairwise_distance(qd, xd, metric)
    d, i = sparse_knn(index, queries, 7, metric)
    assert d.shape == (23, 7) and i.dtype == torch.int64
    assert bool((d[:, 1:] >= d[:, :-1]).all())  # best first
    S.check_knn(metric, d, i, d_ref, true, 1e-10, 1e-10)


def test_knn_inner_product_selects_largest(knn_case):
    index, queries, xd, qd = knn_case
    true = qd @ xd.t()
    d_ref = true.topk(5, dim=1).values
    d, i = sparse_knn(index, queries, 5, "inner_product")
    assert bool((d[:, 1:] <= d[:, :-1]).all())
    S.check_knn("inner_product", d, i, d_ref, true, 1e-10, 1e-10)


@pytest.mark.parametrize("bi,bq", [(50, 10), (7, 23), (3, 5), (1000, 1000)])
def test_knn_batch_sizes(knn_case, bi, bq):
    """Batches that do not divide q = 23 or n = 120, and index batches smaller
    than k = 7."""
    index, queries, xd, qd = knn_case
    true = pairwise_distance(qd, xd, "sqeuclidean")
    d_ref = true.topk(7, dim=1, largest=False).values
    d, i = sparse_knn(index, queries, 7, batch_size_index=bi, batch_size_query=bq)
    S.check_knn("sqeuclidean", d, i, d_ref, true, 1e-10, 1e-10)
    assert all(len(set(row)) == 7 for row in i.tolist())


def test_knn_workspace_budget_drives_batches():
    from raft_amd.core.resources import Resources
    index = S.random_csr(120, 64, 0.15, 14)
    queries = S.random_csr(23, 64, 0.15, 15)
    res = Resources(torch.device("cpu"))
    res.set_workspace_limit(1 << 16)
    d, i = sparse_knn(index, queries, 4, res=res)
    d0, i0 = sparse_knn(index, queries, 4, batch_size_index=120, batch_size_query=23)
    torch.testing.assert_close(d, d0)


def test_new_launchers_link(tmp_path):
    """A translation unit that takes the addresses of the two launchers through
    include/raft_amd/sparse.hpp compiles for gfx950 and, where the kernel
    objects of an in-tree build are present, links against them."""
    src = tmp_path / "consumer.cpp"
    src.write_text(
        "#include <raft_amd/sparse.hpp>\n"
        "int main() {\n"
        "  void* fns[] = {\n"
        "    (void*)&raft_amd::launch_csr_row_stats,\n"
        "    (void*)&raft_amd::launch_csr_pairwise,\n"
        "  };\n"
        "  for (void* f : fns) if (!f) return 1;\n"
        "  return raft_amd::kSparseDenseWindowMax == 8192 ? 0 : 1;\n"
        "}\n")
    obj = str(tmp_path / "consumer.o")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17",
                        "-c", str(src), f"-I{os.path.join(ROOT, 'include')}",
                        "-o", obj], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    objs = sorted(glob.glob(os.path.join(ROOT, "build", "ext", "*.o")))
    objs = [o for o in objs if not o.endswith("bindings.o")]
    if any(o.endswith("sparse_pairwise.o") for o in objs):
        r = subprocess.run(["hipcc", obj, *objs, "-L/opt/rocm/lib", "-lrocblas",
                            "-lhipblaslt", "-o", str(tmp_path / "consumer")],
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
