"""IVF-Flat on the GPU: the list-scan kernel (csrc/ivf_flat_scan.hip) with its
query-group tiers, pair-group boundaries and row split, the filter, the
workspace chunking and the torch fallback, against the fp64 oracle of
tests/ivf_flat_inputs.py."""
import pytest
import torch

import ivf_flat_inputs as I
from raft_amd.neighbors import IvfFlatParams, ivf_flat_build, ivf_flat_search

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


@pytest.mark.parametrize("d", [1024, 2048, 4096])
@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
def test_wide_rows_cover_the_query_group_tiers(d, dtype):
    """Asking for 16 queries per block gives QG = 16 at d = 1024, 8 at 2048 and
    4 at 4096 (64 KiB of staged queries); the default covers 8, 8 and 4."""
    from raft_amd._ext import require_ext
    assert require_ext().ivf_flat_scan_max_qg(d) == {1024: 16, 2048: 8, 4096: 4}[d]
    I.case_width(DEV, d, dtype, n=640, n_lists=4, given_centroids=True, qg=16)
    I.case_width(DEV, d, dtype, n=640, n_lists=4, given_centroids=True)


def test_wider_than_the_kernel_takes_the_torch_path():
    index = I.case_width(DEV, 4100, torch.float32, n=640, n_lists=4,
                         given_centroids=True)
    assert index.d_pad > 4096


def test_native_mode_takes_the_torch_path_with_the_same_results():
    b = I.base_data()
    index = I.base_index("sqeuclidean", torch.float32, DEV)
    d0, i0, p = ivf_flat_search(index, b.q.to(DEV), b.k, 3, return_probes=True)
    native = index.to(DEV)
    native.fp32_mode = "native"
    d1, i1 = ivf_flat_search(native, b.q.to(DEV), b.k, probes=p)
    cpu = index.to("cpu")
    I.check(cpu, b.q, p, d1, i1, b.k)
    I.sets_match_up_to_ties(cpu, b.q, p, i0, i1, b.k)


@pytest.mark.parametrize("qg", [4, 8, 16, 32])
@pytest.mark.parametrize("q", [1, 16, 17, 33])
def test_query_group_boundaries(q, qg):
    """All queries probe one list: full and short pair groups, and the row
    split of a small batch."""
    o = I.one_list_data()
    index = ivf_flat_build(o.x.to(DEV), IvfFlatParams(), centroids=o.centroids.to(DEV))
    assert index.list_sizes.tolist() == [o.x.shape[0], 0]
    queries = o.q[:q]
    d, i, p = ivf_flat_search(index, queries.to(DEV), 7, 1, return_probes=True, qg=qg)
    assert bool((p == 0).all())
    I.check(index.to("cpu"), queries, p, d, i, 7)
    I.check_full_scan(o.x, "sqeuclidean", queries, d, i, 7)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
@pytest.mark.parametrize("metric", ["euclidean", "inner_product"])
def test_filter(metric, dtype):
    I.case_filter(DEV, metric, dtype)


def test_query_chunks_are_bitwise_identical():
    I.case_chunking(DEV, "sqeuclidean", torch.float32, exact=True)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
def test_extend(dtype):
    I.case_extend(DEV, "sqeuclidean", dtype)


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
def test_pack_unpack(dtype):
    I.case_pack_unpack(DEV, dtype)


def test_save_load(tmp_path):
    I.case_save_load(DEV, "euclidean", torch.bfloat16, str(tmp_path / "index.ivf"))


@pytest.mark.parametrize("dtype", I.DTYPES, **I.DTYPE_IDS)
@pytest.mark.parametrize("metric", I.METRICS)
def test_gpu_against_cpu(metric, dtype):
    """The index built on the CPU and moved, with the CPU's probes."""
    b = I.base_data()
    cpu = I.base_index(metric, dtype, "cpu")
    d0, i0, p = ivf_flat_search(cpu, b.q, b.k, 3, return_probes=True)
    d1, i1 = ivf_flat_search(cpu.to(DEV), b.q.to(DEV), b.k, probes=p.to(DEV))
    I.check(cpu, b.q, p, d1, i1, b.k)
    I.sets_match_up_to_ties(cpu, b.q, p, i0, i1, b.k)


def test_argument_errors():
    w = I.width_data(3)
    index = ivf_flat_build(w.x.to(DEV), IvfFlatParams(n_lists=4))
    with pytest.raises(ValueError):
        ivf_flat_search(index, w.q.to(DEV), 0)
    with pytest.raises(ValueError):
        ivf_flat_search(index, w.q, 1)            # queries on another device
    with pytest.raises(ValueError):
        ivf_flat_search(index, w.q.to(DEV), 1, qg=5)
