"""csrc/cagra.hip (engine="kernel") against the torch paths of neighbors.cagra.

Search tests build the index on the CPU and move it, so both sides walk one graph."""
import pytest
import torch

import cagra_inputs as C
import test_cagra as T
from refine_inputs import U
from test_cagra import recall_data  # noqa: F401  (a fixture)
from raft_amd.neighbors import (CagraIndex, CagraParams, cagra_build, cagra_optimize, cagra_search,
                                optimize_kernel_serves, search_kernel_serves)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,kd,g,tails", [(130, 8, 4, False), (1000, 32, 16, False),
                                          (300, 96, 33, False), (600, 128, 64, False),
                                          (400, 256, 128, False), (20, 32, 16, True)])
def test_prune_kernel_equals_the_torch_path(n, kd, g, tails):
    assert optimize_kernel_serves(kd, g)
    graph = C.knn_graph(n, kd, tails)
    got = cagra_optimize(graph.cuda(), g, engine="kernel")
    assert torch.equal(got.cpu(), cagra_optimize(graph, g, engine="torch"))
    assert torch.equal(cagra_optimize(graph.int().cuda(), g), got)


def check_search(index, qs, k, gpu_index=None, **kw):
    assert search_kernel_serves(index.dim, kw.get("itopk_size", 64), kw.get("search_width", 1),
                                index.graph_degree, k)
    ref = cagra_search(index, qs, k, engine="torch", **kw)
    if "seeds" in kw:
        kw["seeds"] = kw["seeds"].cuda()
    got = cagra_search(gpu_index or index.to("cuda"), qs.cuda(), k, engine="kernel", **kw)
    assert (got[0].dtype, got[1].dtype) == (torch.float32, torch.int64)
    assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[0].cpu(), ref[0]), (got, ref)
    return ref


@pytest.mark.parametrize("d", [1, 20, 128, 1000, 4096])
@pytest.mark.parametrize("metric", C.METRICS)
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_search_kernel_over_dtype_metric_and_width(dtype, metric, d):
    index, qs = C.cpu_index(300, d, 8, metric, dtype)
    check_search(index, qs[:5], 10, itopk_size=32)


@pytest.mark.parametrize("view", ["rows", "columns", "misaligned"])
@pytest.mark.parametrize("dtype", C.DTYPES)
def test_search_kernel_reads_a_sliced_dataset_in_place(dtype, view):
    big = C.integer_rows(600, 48, 5, dtype)
    cut = {"rows": lambda t: t[::2, :40], "columns": lambda t: t[:300, 4:44],
           "misaligned": lambda t: t[:300, 1:41]}[view]
    index, qs = C.cpu_index(300, 40, 8)
    index = CagraIndex(cut(big).contiguous(), index.graph, index.seeds, index.metric)
    gpu = CagraIndex(cut(big.cuda()), index.graph.cuda(), index.seeds.cuda(), index.metric)
    assert not gpu.dataset.is_contiguous()
    check_search(index, qs[:5].to(dtype), 10, gpu, itopk_size=32)


@pytest.mark.parametrize("L,w,g", [(32, 1, 4), (64, 1, 32), (64, 4, 32), (512, 4, 128)])
@pytest.mark.parametrize("q", [1, 70])
def test_search_kernel_over_list_and_batch_sizes(L, w, g, q):
    index, qs = C.cpu_index(700, 20, g)
    check_search(index, qs[:q], L, itopk_size=L, search_width=w)              # k = L


@pytest.mark.parametrize("kw", [dict(hash_slots=256, max_iterations=40),     # resets
                                dict(max_iterations=3),                       # cut mid-walk
                                dict(seeds=T.caller_seeds(700, 6, True))])
def test_search_kernel_table_resets_cutoff_and_caller_seeds(kw):
    index, qs = C.cpu_index(700, 20, 32)
    check_search(index, qs[:6], 10, itopk_size=64, **kw)


def test_search_kernel_fills_missing_slots():
    index, qs = C.cpu_index(10, 8, 4)
    dists, ids = check_search(index, qs[:3], 16, itopk_size=32)
    assert bool((ids[:, 10:] == -1).all()) and bool(dists[:, 10:].isinf().all())
    assert bool((ids[:, :10] >= 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_real_values_within_the_bound(dtype):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2000 + 20, 96, generator=g).to(dtype)
    index = cagra_build(x[:2000], CagraParams(graph_degree=16, intermediate_graph_degree=32,
                                              build_algo="brute_force"))
    dists, ids = cagra_search(index.to("cuda"), x[2000:].cuda(), 10, engine="kernel")
    dists, ids = dists.cpu().double(), ids.cpu()
    assert all(row.unique().numel() == 10 for row in ids) and bool((ids >= 0).all())
    term = (x[ids].double() - x[2000:].double().unsqueeze(1)) ** 2
    assert bool(((dists - term.sum(dim=2)).abs() <= (96 + 8) * U * term.sum(dim=2)).all())
    assert bool((dists[:, 1:] >= dists[:, :-1]).all())


def test_recall_condition_end_to_end_on_the_gpu(recall_data):  # noqa: F811
    T.test_recall_condition(recall_data, "cuda")


@pytest.mark.parametrize("d,w,g", [(4097, 1, 8), (8, 19, 27)])
def test_beyond_the_kernel_auto_takes_the_torch_path(d, w, g):
    assert not search_kernel_serves(d, 64, w, g, 10)
    gen = torch.Generator().manual_seed(d)
    graph = torch.randint(0, 200, (200, g), generator=gen).int()
    x = C.integer_rows(203, d, 4)
    index = CagraIndex(x[:200], graph, torch.arange(64).int(), "sqeuclidean")
    ref = cagra_search(index, x[200:], 10, search_width=w)
    got = cagra_search(index.to("cuda"), x[200:].cuda(), 10, search_width=w)
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
    with pytest.raises(ValueError):
        cagra_search(index.to("cuda"), x[200:].cuda(), 10, search_width=w, engine="kernel")
    with pytest.raises(ValueError):
        cagra_search(index, x[200:], 10, search_width=w, engine="kernel")
