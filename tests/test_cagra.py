"""neighbors.cagra on the CPU (the torch paths) against the literal references of
tests/cagra_inputs.py. tests/test_gpu_cagra.py checks csrc/cagra.hip against these paths."""
import pytest
import torch

import cagra_inputs as C
from raft_amd.neighbors import CagraParams, cagra_build, cagra_optimize, cagra_search, knn


@pytest.mark.parametrize("n,kd,g,tails", [(40, 8, 4, False), (6, 8, 4, True)])
def test_optimize_equals_the_literal_loops(n, kd, g, tails):
    graph = C.knn_graph(n, kd, tails)
    got = cagra_optimize(graph, g)
    assert got.dtype == torch.int32
    assert torch.equal(got, C.optimize_reference(graph, g))
    assert torch.equal(cagra_optimize(graph.int(), g), got)


def caller_seeds(n, q, per_query):
    """A repeated seed and seeds out of range among valid ones."""
    g = torch.Generator().manual_seed(3)
    seeds = torch.randint(0, n, (q, 12) if per_query else (12,), generator=g)
    seeds[..., 1], seeds[..., 5], seeds[..., 7] = seeds[..., 0], n, -1
    return seeds


@pytest.mark.parametrize("seeds", ["index", "shared", "per_query"])
@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("metric", C.METRICS)
def test_search_equals_the_literal_loop(metric, w, seeds):
    index, qs = C.cpu_index(300, 8, 8, metric)
    qs = qs[:9]
    given = None if seeds == "index" else caller_seeds(300, 9, seeds == "per_query")
    got = cagra_search(index, qs, 10, itopk_size=32, search_width=w, seeds=given)
    ref = C.search_reference(index, qs, 10, 32, w, index.seeds[:32] if given is None else given)
    assert (got[0].dtype, got[1].dtype) == (torch.float32, torch.int64)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0]), (got, ref)


@pytest.fixture(scope="module")
def recall_data():
    """Uniform integer rows, 4096 x 32, 200 queries and the ids of their exact 10 nearest."""
    x = C.integer_rows(4096 + 200, 32, 11)
    x, qs = x[:4096], x[4096:]
    return x, qs, knn(x, qs, 10)[1]


def test_recall_condition(recall_data, dev="cpu"):
    x, qs, exact = recall_data
    index = cagra_build(x.to(dev), CagraParams(graph_degree=32, intermediate_graph_degree=64,
                                               build_algo="brute_force"))
    assert index.graph.shape == (4096, 32) and index.seeds.shape == (512,)
    assert index.seeds.unique().numel() == 512
    ids = cagra_search(index, qs.to(dev), 10, itopk_size=64)[1]
    assert all(row.unique().numel() == 10 for row in ids.cpu())
    # measured on the CPU path: 0.9845 (ties of the integer data count against it)
    assert float((ids.cpu()[:, :, None] == exact[:, None, :]).any(dim=2).float().mean()) >= 0.95


def test_errors_and_edges():
    index, qs = C.cpu_index(300, 8, 8)
    with pytest.raises(ValueError):
        cagra_search(index, qs, 10, engine="kernel")              # CPU tensors
    with pytest.raises(ValueError):
        cagra_search(index, qs, 65)                                # k > itopk_size
    with pytest.raises(ValueError):
        cagra_search(index, qs, 10, hash_slots=100)                # not a power of two
    with pytest.raises(ValueError):
        cagra_optimize(index.graph, 9)                             # graph_degree > kd
    with pytest.raises(ValueError):
        cagra_build(qs, CagraParams(build_algo="nn_descent"))
    d, i = cagra_search(index, qs[:0], 3)
    assert d.shape == (0, 3) and i.shape == (0, 3)
    moved = index.to("cpu")
    assert (moved.n_rows, moved.dim, moved.graph_degree) == (300, 8, 8)
