"""IVF-Flat on the CPU: the pure-PyTorch path over unpack_list, the packing,
extend, the serializer and the argument checks, against the fp64 oracle of
tests/ivf_flat_inputs.py."""
import pytest
import torch

import ivf_flat_inputs as I
from raft_amd.distance import DistanceType
from raft_amd.neighbors import (IvfFlatIndex, IvfFlatParams, ivf_flat_build,
                                ivf_flat_extend, ivf_flat_search)

DEV = "cpu"


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
@pytest.mark.parametrize("metric", I.METRICS)
def test_exact_with_all_lists_probed(metric, dtype):
    I.case_exactness(DEV, metric, dtype)


@pytest.mark.parametrize("n_probes", [1, 3])
@pytest.mark.parametrize("metric", I.METRICS)
def test_few_probes_vs_oracle(metric, n_probes):
    I.case_few_probes(DEV, metric, torch.float32, n_probes)


def test_few_probes_bf16():
    I.case_few_probes(DEV, "sqeuclidean", torch.bfloat16, 3)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product"])
def test_forced_list_shapes(metric, dtype):
    I.case_forced_lists(DEV, metric, dtype)


@pytest.mark.parametrize("d,dtype", [(1, torch.float32), (3, torch.float32),
                                     (129, torch.float32), (9, torch.bfloat16)])
def test_feature_widths(d, dtype):
    I.case_width(DEV, d, dtype)


@pytest.mark.parametrize("metric", ["euclidean", "inner_product"])
def test_filter(metric):
    I.case_filter(DEV, metric, torch.float32)


def test_query_chunks_from_the_workspace_limit():
    I.case_chunking(DEV, "sqeuclidean", torch.float32, exact=False)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
def test_extend(dtype):
    I.case_extend(DEV, "sqeuclidean", dtype)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
def test_pack_unpack(dtype):
    I.case_pack_unpack(DEV, dtype)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
def test_save_load(tmp_path, dtype):
    I.case_save_load(DEV, "euclidean", dtype, str(tmp_path / "index.ivf"))


def test_fp16_is_widened_to_fp32():
    w = I.width_data(3)
    index = ivf_flat_build(w.x.half(), IvfFlatParams(n_lists=4))
    assert index.dtype == torch.float32 and isinstance(index, IvfFlatIndex)
    assert index.metric == DistanceType.L2Expanded
    d, i, p = ivf_flat_search(index, w.q.half(), 5, 2, return_probes=True)
    I.check(index, w.q.half().float(), p, d, i, 5)


def test_metric_enum_and_n_probes_clamp():
    w = I.width_data(3)
    index = ivf_flat_build(w.x, IvfFlatParams(n_lists=4,
                                              metric=DistanceType.InnerProduct))
    d, i, p = ivf_flat_search(index, w.q, 5, 100, return_probes=True)
    assert tuple(p.shape) == (w.q.shape[0], 4)
    I.check_full_scan(w.x, "inner_product", w.q, d, i, 5)


def test_argument_errors():
    w = I.width_data(3)
    with pytest.raises(ValueError):
        ivf_flat_build(w.x, IvfFlatParams(n_lists=4, metric="cosine"))
    with pytest.raises(ValueError):
        ivf_flat_build(w.x, IvfFlatParams(n_lists=4, metric=DistanceType.L1))
    index = ivf_flat_build(w.x, IvfFlatParams(n_lists=4))
    with pytest.raises(ValueError):
        ivf_flat_search(index, w.q, 0)
    with pytest.raises(ValueError):
        ivf_flat_search(index, torch.zeros(2, 4), 1)
    with pytest.raises(ValueError):
        ivf_flat_extend(index, torch.zeros(2, 4))
    with pytest.raises(ValueError):
        ivf_flat_extend(index, torch.zeros(2, 3, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ivf_flat_extend(index, torch.zeros(2, 3), torch.arange(3))
    with pytest.raises(ValueError):
        ivf_flat_search(index, w.q, 1, filter=torch.ones(600))
