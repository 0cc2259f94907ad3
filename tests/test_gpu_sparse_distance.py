"""GPU kernels of csrc/sparse_pairwise.hip against the CPU fp64 path: both LDS
staging strategies, chunked hash tables, windowed slabs, probing chains,
degenerate inputs, dtypes, self-joins and sparse kNN."""
import pytest
import torch

import sparse_dist_inputs as S
from raft_amd.sparse import CSR, sparse_knn, sparse_pairwise_distance

pytestmark = pytest.mark.gpu

R, JT = 4, 64  # A rows per block / B rows per output tile of the kernel
# one stored value; ragged in the row group and in the B tile; n = 1000 is
# split over several blocks along B for the 33 row groups of m = 130
SHAPES = [(1, 1, 1), (R + 1, JT + 1, 33), (130, 1000, 257)]
STRATEGIES = ["dense", "hash"]
EXACT_METRICS = ["inner_product", "sqeuclidean", "l1"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def gpu(a, dev, dtype=torch.float32):
    return S.cast(a, dtype).to(dev)


_cache = {}


def parity_case(kind, m, n, d):
    """(a, b) fp64 CPU CSR inputs, built once per (kind, shape)."""
    key = (kind, m, n, d)
    if key not in _cache:
        _cache[key] = (S.random_csr(m, d, 0.1, 21, kind), S.random_csr(n, d, 0.1, 22, kind))
    return _cache[key]


_ref_cache = {}


def parity_ref(metric, p, m, n, d):
    key = (metric, m, n, d)
    if key not in _ref_cache:
        a, b = parity_case(S.kind_for(metric), m, n, d)
        _ref_cache[key] = sparse_pairwise_distance(a, b, metric, p)
    return _ref_cache[key]


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("m,n,d", SHAPES)
@pytest.mark.parametrize("metric,p", S.METRICS, ids=S.METRIC_IDS)
def test_parity_fp32(dev, metric, p, m, n, d, strategy):
    a, b = parity_case(S.kind_for(metric), m, n, d)
    got = sparse_pairwise_distance(gpu(a, dev), gpu(b, dev), metric, p, strategy=strategy)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (m, n)
    S.check_close(metric, got, parity_ref(metric, p, m, n, d), 1e-4, 1e-4)


def test_auto_strategy_and_int64_indices(dev):
    a, b = parity_case("signed", R + 1, JT + 1, 33)
    a64 = CSR(a.indptr.long(), a.indices.long(), a.values.float(), a.n_rows, a.n_cols).to(dev)
    got = sparse_pairwise_distance(a64, gpu(b, dev), "cosine")
    S.check_close("cosine", got, parity_ref("cosine", 2.0, R + 1, JT + 1, 33), 1e-4, 1e-4)


# ---- exactness: integer values, every sum an integer below 2^24 ------------

@pytest.fixture(scope="module")
def int_case():
    a = S.random_csr(37, 300, 0.2, 31, "int")
    b = S.random_csr(70, 300, 0.2, 32, "int")
    refs = {m: sparse_pairwise_distance(a, b, m).float() for m in EXACT_METRICS}
    return a, b, refs


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("metric", EXACT_METRICS)
def test_exact_on_small_integers(dev, int_case, metric, strategy):
    a, b, refs = int_case
    got = sparse_pairwise_distance(gpu(a, dev), gpu(b, dev), metric, strategy=strategy)
    assert torch.equal(got.cpu(), refs[metric])


def _exact_vs_default_and_cpu(dev, a, b, **kw):
    for metric in EXACT_METRICS:
        ref = sparse_pairwise_distance(a, b, metric).float()
        default = sparse_pairwise_distance(gpu(a, dev), gpu(b, dev), metric)
        got = sparse_pairwise_distance(gpu(a, dev), gpu(b, dev), metric, **kw)
        assert torch.equal(got, default), metric
        assert torch.equal(got.cpu(), ref), metric


def test_hash_chunking(dev):
    """An A row of 200 stored values against 32-entry chunks (capacity 64)."""
    g = torch.Generator().manual_seed(33)
    d = 1000
    mask = torch.rand(6, d, generator=g) < 0.05
    mask[2] = False
    mask[2, torch.randperm(d, generator=g)[:200]] = True
    vals = torch.randint(-3, 4, (6, d), generator=g).double()
    a = S.csr_from_mask(mask, vals)
    assert int(a.row_lengths()[2]) == 200
    b = S.random_csr(70, d, 0.1, 34, "int")
    _exact_vs_default_and_cpu(dev, a, b, strategy="hash", hash_capacity=64)


def test_dense_windowing(dev):
    """d = 300 over windows of 128 columns: two full windows and a ragged one."""
    a = S.random_csr(9, 300, 0.2, 35, "int")
    b = S.random_csr(70, 300, 0.2, 36, "int")
    _exact_vs_default_and_cpu(dev, a, b, strategy="dense", dense_window=128)


def test_hash_probing_single_bucket(dev):
    """Capacity 64 and an A row whose columns are all multiples of 64: every
    key starts in bucket 0 and is found only by walking the chain. B rows hit
    some of those columns and miss others."""
    g = torch.Generator().manual_seed(37)
    d = 64 * 40
    mask = torch.rand(5, d, generator=g) < 0.01
    mask[1] = False
    mask[1, torch.arange(0, d, 64)] = True
    vals = torch.randint(1, 4, (5, d), generator=g).double()
    a = S.csr_from_mask(mask, vals)
    assert int(a.row_lengths()[1]) == 40 and bool((a.indices[a.indptr[1]:a.indptr[2]] % 64 == 0).all())
    bmask = torch.rand(66, d, generator=g) < 0.01
    bmask[:, torch.arange(0, d, 64)] = torch.rand(66, 40, generator=g) < 0.5
    bmask[:, torch.arange(1, d, 64)] = torch.rand(66, 40, generator=g) < 0.5  # near misses
    b = S.csr_from_mask(bmask, torch.randint(1, 4, (66, d), generator=g).double())
    _exact_vs_default_and_cpu(dev, a, b, strategy="hash", hash_capacity=64)


# ---- degenerate inputs ------------------------------------------------------

@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("metric", ["sqeuclidean", "cosine", "l1", "canberra", "jaccard"])
def test_empty_rows(dev, metric, strategy):
    kind = S.kind_for(metric)
    a = S.with_empty_rows(S.random_csr(11, 60, 0.2, 41, kind), [0, 5, 10])
    b = S.with_empty_rows(S.random_csr(67, 60, 0.2, 42, kind), [0, 30, 66])
    got = sparse_pairwise_distance(gpu(a, dev), gpu(b, dev), metric, strategy=strategy)
    S.check_close(metric, got, sparse_pairwise_distance(a, b, metric), 1e-4, 1e-4)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_nnz_zero_and_no_rows(dev, strategy):
    e = S.empty_csr(5, 60)
    b = S.random_csr(7, 60, 0.2, 43)
    for metric in ("sqeuclidean", "cosine", "l1", "hamming"):
        for x, y in ((e, b), (b, e), (e, e)):
            got = sparse_pairwise_distance(gpu(x, dev), gpu(y, dev), metric, strategy=strategy)
            S.check_close(metric, got, sparse_pairwise_distance(x, y, metric), 1e-4, 1e-4)
    z = S.empty_csr(0, 60)
    assert sparse_pairwise_distance(gpu(z, dev), gpu(b, dev), strategy=strategy).shape == (0, 7)
    assert sparse_pairwise_distance(gpu(b, dev), gpu(z, dev), strategy=strategy).shape == (7, 0)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("metric", ["canberra", "hamming", "l1", "jensenshannon"])
def test_stored_zeros(dev, metric, strategy):
    g = torch.Generator().manual_seed(44)
    mask = torch.rand(9, 70, generator=g) < 0.3
    vals = ((torch.rand(9, 70, generator=g) + 0.1) * mask).double()
    plain = S.csr_from_mask(mask, vals)
    padded = S.csr_from_mask(mask | (torch.rand(9, 70, generator=g) < 0.3), vals)
    assert int((padded.values == 0).sum()) > 0
    ref = sparse_pairwise_distance(plain, plain, metric)
    for x, y in ((padded, plain), (plain, padded), (padded, padded)):
        got = sparse_pairwise_distance(gpu(x, dev), gpu(y, dev), metric, strategy=strategy)
        S.check_close(metric, got, ref, 1e-4, 1e-4)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_unsorted_columns(dev, strategy):
    a = S.random_csr(9, 80, 0.3, 45, "int")
    b = S.random_csr(66, 80, 0.3, 46, "int")
    au = S.random_csr(9, 80, 0.3, 45, "int", shuffle_seed=1)
    bu = S.random_csr(66, 80, 0.3, 46, "int", shuffle_seed=2)
    assert not torch.equal(a.indices, au.indices)
    for metric in EXACT_METRICS:
        got = sparse_pairwise_distance(gpu(au, dev), gpu(bu, dev), metric, strategy=strategy)
        assert torch.equal(got.cpu(), sparse_pairwise_distance(a, b, metric).float())


# ---- dtypes, self-join, argument errors -----------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_inputs_widen_exactly(dev, dtype):
    a = S.cast(S.random_csr(9, 80, 0.3, 47), dtype)
    b = S.cast(S.random_csr(66, 80, 0.3, 48), dtype)
    for metric in ("cosine", "l1"):
        got = sparse_pairwise_distance(a.to(dev), b.to(dev), metric)
        wide = sparse_pairwise_distance(gpu(a, dev), gpu(b, dev), metric)
        assert got.dtype == torch.float32
        assert torch.equal(got, wide)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_self_join_diagonal(dev, strategy):
    a = gpu(S.random_csr(70, 120, 0.2, 49), dev)
    for metric in ("l1", "hamming", "canberra"):
        diag = sparse_pairwise_distance(a, None, metric, strategy=strategy).diagonal()
        assert float(diag.abs().max()) == 0.0, metric
    for metric in ("sqeuclidean", "cosine"):
        diag = sparse_pairwise_distance(a, None, metric, strategy=strategy).diagonal()
        assert float(diag.abs().max()) <= 1e-4, metric
    assert torch.equal(sparse_pairwise_distance(a, None, "l1", strategy=strategy),
                       sparse_pairwise_distance(a, a, "l1", strategy=strategy))


def test_argument_errors_on_gpu(dev):
    a = gpu(S.random_csr(4, 20, 0.5, 50), dev)
    with pytest.raises(TypeError, match="fp64"):
        sparse_pairwise_distance(S.cast(a, torch.float64), None)
    for metric in S.UNSUPPORTED:
        with pytest.raises(ValueError, match=metric):
            sparse_pairwise_distance(a, a, metric)
    with pytest.raises(ValueError, match="strategy"):
        sparse_pairwise_distance(a, a, strategy="sorted")
    with pytest.raises(ValueError, match="hash_capacity"):
        sparse_pairwise_distance(a, a, strategy="hash", hash_capacity=96)


# ---- kNN ------------------------------------------------------------------

@pytest.fixture(scope="module")
def knn_case():
    index = S.random_csr(300, 64, 0.15, 51)
    queries = S.random_csr(40, 64, 0.15, 52)
    return index, queries


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("metric", ["sqeuclidean", "cosine", "l1", "inner_product"])
def test_knn(dev, knn_case, metric, k):
    index, queries = knn_case
    d_cpu, _ = sparse_knn(index, queries, k, metric)
    true = sparse_pairwise_distance(queries, index, metric)
    # 300 rows in batches of 128: three index batches
    d_gpu, i_gpu = sparse_knn(gpu(index, dev), gpu(queries, dev), k, metric,
                              batch_size_index=128, batch_size_query=16)
    assert d_gpu.dtype == torch.float32 and i_gpu.dtype == torch.int64
    S.check_knn(metric, d_gpu, i_gpu, d_cpu, true, 1e-4, 1e-4)
