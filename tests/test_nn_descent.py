"""neighbors.nn_descent on the CPU (the torch paths) against the literal references of
tests/nn_descent_inputs.py. tests/test_gpu_nn_descent.py checks csrc/nn_descent.hip
against these paths."""
import pytest
import torch

import cagra_inputs as C
import nn_descent_inputs as N
from test_cagra import recall_data  # noqa: F401  (a fixture)
from raft_amd.neighbors import CagraParams, cagra_build, cagra_search, nn_descent
from raft_amd.neighbors.nn_descent import merge_candidates


@pytest.mark.parametrize("metric", C.METRICS[::2])
def test_join_and_merge_equal_the_literal_loops(metric):
    x = C.integer_rows(60, 6, 1)
    for rounds in (0, 2):                                   # all new; new and old entries
        lists, new, old, triples = N.torch_rounds(x, 8, 4, rounds, metric)
        assert bool((old >= 0).any()) == (rounds > 0)
        for got, ref in zip(triples, N.join_reference(x, new, old, metric)):
            assert got.dtype == ref.dtype and torch.equal(got, ref), (got, ref)
        *got, updates = merge_candidates(*lists, *triples)
        ref = N.merge_reference(*lists, *triples)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), (got, ref)
        assert updates == int(ref[2].sum()) - int(lists[2].sum()) and updates > 0


def test_invariants_and_recall():
    x = C.integer_rows(4096, 32, 11)
    dists, ids = nn_descent(x, 32)
    N.check_invariants(dists, ids, 32)
    assert torch.equal(dists, ((x[ids] - x.unsqueeze(1)) ** 2).sum(dim=2))
    # measured on the CPU path: 0.9146 (ties of the integer data count against it)
    assert N.recall(ids, x, 32) >= 0.90


def test_cagra_build_takes_the_graph(recall_data):  # noqa: F811
    x, qs, exact = recall_data
    index = cagra_build(x, CagraParams(graph_degree=32), knn_graph=nn_descent(x, 64)[1])
    assert index.graph.shape == (4096, 32)
    ids = cagra_search(index, qs, 10, itopk_size=64)[1]
    assert all(row.unique().numel() == 10 for row in ids)
    # measured on the CPU path: 0.9840
    assert float((ids[:, :, None] == exact[:, None, :]).any(dim=2).float().mean()) >= 0.95


def test_errors():
    x = C.integer_rows(50, 8, 2)
    with pytest.raises(ValueError):
        nn_descent(x.double(), 4)                                   # dtype
    with pytest.raises(ValueError):
        nn_descent(x, 0)                                            # k < 1
    with pytest.raises(ValueError):
        nn_descent(x, 4, n_samples=33, engine="kernel")
    with pytest.raises(ValueError):
        nn_descent(x, 4, engine="kernel")                           # CPU tensors
    with pytest.raises(ValueError):
        cagra_build(x, CagraParams(graph_degree=8), knn_graph=nn_descent(x, 4)[1])
    dists, ids = nn_descent(x[:3], 4, metric="inner_product")       # n - 1 < k
    assert bool((ids[:, 2:] == -1).all()) and bool((dists[:, 2:] == float("-inf")).all())
    assert bool((ids[:, :2] >= 0).all())
