"""neighbors.refine on the CPU (the torch path) against tests/refine_inputs.py.
tests/test_gpu_refine.py runs the same bodies with dev="cuda", engine="kernel"."""
import pytest
import torch

import ivf_pq_inputs as P
import refine_inputs as R
from raft_amd.neighbors import ivf_pq_search, refine

#: (d, n_cand, k, q): d tiers next to ragged n_cand, n_cand edges next to plain d
FP32_CASES = ((1, 5, 8, 3), (3, 100, 100, 3), (4, 1, 1, 3), (4, 4096, 7, 1), (36, 257, 260, 3),
              (128, 64, 1, 1), (128, 100, 103, 3), (260, 100, 10, 3), (260, 257, 257, 1),
              (8192, 5, 5, 3), (8192, 64, 67, 1))
HALF_CASES = ((8, 5, 1, 3), (100, 257, 260, 3), (200, 64, 64, 3), (520, 100, 100, 3),
              (520, 64, 67, 1))
CASES = ([(torch.float32,) + c for c in FP32_CASES]
         + [(t,) + c for t in (torch.bfloat16, torch.float16) for c in HALF_CASES])


def exact_inputs(dtype, d, n_cand, q, n):
    """Integers in [-4, 4]: fp32 sums are exact, ties plentiful. A row with room holds
    -1, ids >= n and a repeated id; the last of three rows is entirely invalid."""
    g = torch.Generator().manual_seed(1000 * d + n_cand)
    x = torch.randint(-4, 5, (n, d), generator=g).to(dtype)
    qs = torch.randint(-4, 5, (q, d), generator=g).to(dtype)
    cand = torch.randint(0, n, (q, n_cand), generator=g)
    if n_cand >= 5:
        cand[:, 1], cand[:, 2], cand[:, 3], cand[:, 4] = -1, n, 2 ** 40 + 3, cand[:, 0]
    if q > 1:
        cand[-1] = torch.tensor([-1, n, -2 ** 33, 2 ** 32 + 1])[torch.arange(n_cand) % 4]
    return x, qs, cand


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("dtype,d,n_cand,k,q", CASES)
def test_exact_on_integer_inputs(dtype, d, n_cand, k, q, metric, dev="cpu", engine="auto", n=0):
    x, qs, cand = exact_inputs(dtype, d, n_cand, q, n or (5000 if n_cand > 1000 else 300))
    got = refine(x.to(dev), qs.to(dev), cand.to(dev), k, metric, engine=engine)
    R.assert_exact(got, R.reference(x, qs, cand, k, metric), metric, d)
    flipped = refine(x.to(dev), qs.to(dev), cand.flip(1).to(dev), k, metric, engine=engine)
    assert torch.equal(flipped[0], got[0]) and torch.equal(flipped[1], got[1])


def real_inputs(dtype, d=260, n_cand=100, q=3, n=400):
    g = torch.Generator().manual_seed(5)
    x, qs = torch.randn(n, d, generator=g).to(dtype), torch.randn(q, d, generator=g).to(dtype)
    cand = torch.stack([torch.randperm(n, generator=g)[:n_cand] for _ in range(q)])
    cand[:, 7] = -1
    return x, qs, cand


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_real_values_within_the_bound(dtype, metric, dev="cpu", engine="auto"):
    x, qs, cand = real_inputs(dtype)
    R.assert_close(refine(x.to(dev), qs.to(dev), cand.to(dev), 10, metric, engine=engine),
                   x, qs, cand, 10, metric)


@pytest.mark.parametrize("view", ["columns", "rows", "misaligned"])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_strided_rows_equal_their_contiguous_copy(dtype, view, dev="cpu", engine="auto"):
    """GPU: fp32 "columns" and all "rows" take the vector path, the rest the element-wise."""
    d = 40
    g = torch.Generator().manual_seed(9)
    big = torch.randn(600, d + 8, generator=g).to(dtype).to(dev)
    x = {"columns": big[:, 4:4 + d], "rows": big[::2, :d], "misaligned": big[:, 1:1 + d]}[view]
    qs = torch.randn(3, d, generator=g).to(dev)
    cand = torch.randint(-2, x.shape[0] + 2, (3, 100), generator=g).to(dev)
    for metric in R.METRICS:
        a = refine(x, qs, cand, 12, metric, engine=engine)
        b = refine(x.contiguous(), qs, cand, 12, metric, engine=engine)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        R.assert_close(a, x.cpu(), qs.cpu(), cand.cpu(), 12, metric)


@pytest.mark.parametrize("metric", R.METRICS)
def test_nan_row_keeps_its_id_and_ranks_before_the_missing(metric, dev="cpu", engine="auto"):
    x, qs, _ = real_inputs(torch.float32, d=36, q=1, n=50)
    x[11, 5] = float("nan")
    cand = torch.tensor([[3, 11, -1, 20, 4]])
    dists, ids = refine(x.to(dev), qs.to(dev), cand.to(dev), 6, metric, engine=engine)
    bad = float("-inf") if metric == "inner_product" else float("inf")
    assert sorted(ids[0, :3].tolist()) == [3, 4, 20] and ids[0, 3:].tolist() == [11, -1, -1]
    assert bool(dists[0, :3].isfinite().all()) and dists[0, 3:].tolist() == [bad] * 3


def test_empty_inputs_and_errors(dev="cpu", engine="auto"):
    x, qs, cand = (t.to(dev) for t in real_inputs(torch.float32, d=8, n_cand=10, q=2, n=20))
    dists, ids = refine(x, qs, cand[:, :0], 3, "inner_product", engine=engine)
    assert bool((dists == float("-inf")).all()) and bool((ids == -1).all())
    assert tuple(refine(x, qs[:0], cand[:0], 3, engine=engine)[1].shape) == (0, 3)
    for args in ((x, qs, cand, 0), (x, qs[:, :7], cand, 3), (x, qs, cand[:1], 3),
                 (x, qs, cand.int(), 3), (x.t(), qs[:, :20], cand, 3), (x, qs, cand, 3, "cosine"),
                 (x.cpu(), qs.cpu(), cand.cpu(), 3, "euclidean", "kernel")):
        with pytest.raises(ValueError):
            refine(*args[:5], engine=args[5] if len(args) > 5 else engine)


@pytest.mark.parametrize("metric", R.METRICS)
def test_ivf_pq_search_with_a_dataset_is_search_then_refine(metric, dev="cpu"):
    f, index = P.forced_index(dev, metric, 24, 24)
    x, qs, k, n_lists = f.x.to(dev), f.q.to(dev), 5, index.n_lists
    plain = ivf_pq_search(index, qs, k, n_lists)
    same = ivf_pq_search(index, qs, k, n_lists, dataset=None, refine_ratio=7)
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    wide = ivf_pq_search(index, qs, 4 * k, n_lists)
    want = refine(x, qs, wide[1], k, metric)
    got = ivf_pq_search(index, qs, k, n_lists, dataset=x, refine_ratio=4, return_probes=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert tuple(got[2].shape) == (qs.shape[0], n_lists)
    R.assert_close(got[:2], f.x, f.q, wide[1].cpu(), k, metric)
