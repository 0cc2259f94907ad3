"""csrc/refine.hip (engine="kernel") on the bodies and cases of tests/test_refine.py."""
import pytest
import torch

import refine_inputs as R
import test_refine as T
from raft_amd.neighbors import refine
from raft_amd.neighbors.refine import kernel_serves

pytestmark = pytest.mark.gpu
GPU = ("cuda", "kernel")


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("dtype,d,n_cand,k,q", T.CASES)
def test_exact_on_integer_inputs(dtype, d, n_cand, k, q, metric):
    assert kernel_serves(d, n_cand, k)
    T.test_exact_on_integer_inputs(dtype, d, n_cand, k, q, metric, *GPU)


def test_exact_at_the_lds_maximum():
    """32 KiB of query and 32 KiB of keys: d = 8192 with n_cand = 4096 = k."""
    T.test_exact_on_integer_inputs(torch.float16, 8192, 4096, 4096, 1, "inner_product", *GPU,
                                   n=700)


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_real_values_within_the_bound(dtype, metric):
    T.test_real_values_within_the_bound(dtype, metric, *GPU)


@pytest.mark.parametrize("view", ["columns", "rows", "misaligned"])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_strided_rows_equal_their_contiguous_copy(dtype, view):
    T.test_strided_rows_equal_their_contiguous_copy(dtype, view, *GPU)


@pytest.mark.parametrize("metric", R.METRICS)
def test_nan_row_keeps_its_id_and_ranks_before_the_missing(metric):
    T.test_nan_row_keeps_its_id_and_ranks_before_the_missing(metric, *GPU)


def test_empty_inputs_and_errors():
    T.test_empty_inputs_and_errors(*GPU)


@pytest.mark.parametrize("d,n_cand", [(4, 4097), (8200, 5)])
def test_beyond_the_kernel_auto_takes_the_torch_path(d, n_cand):
    assert not kernel_serves(d, n_cand, 4)
    T.test_exact_on_integer_inputs(torch.float32, d, n_cand, 4, 3, "sqeuclidean", "cuda", "auto")
    x, qs, cand = (t.cuda() for t in T.exact_inputs(torch.float32, d, n_cand, 3, 300))
    with pytest.raises(ValueError):
        refine(x, qs, cand, 4, engine="kernel")


@pytest.mark.parametrize("metric", R.METRICS)
def test_ivf_pq_search_with_a_dataset_is_search_then_refine(metric):
    T.test_ivf_pq_search_with_a_dataset_is_search_then_refine(metric, "cuda")
