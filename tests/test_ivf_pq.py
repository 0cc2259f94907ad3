"""IVF-PQ on the CPU (the plain-torch path) against tests/ivf_pq_inputs.py."""
import pytest
import torch

import ivf_pq_inputs as I
from raft_amd.neighbors import (IvfPqParams, ivf_pq_build, ivf_pq_extend, ivf_pq_load,
                                ivf_pq_search)

@pytest.mark.parametrize("d,pq_dim", I.SHAPES)
@pytest.mark.parametrize("metric", I.METRICS)
def test_search_vs_oracle(metric, d, pq_dim):
    I.case_search("cpu", metric, d, pq_dim)


@pytest.mark.parametrize("metric", I.METRICS)
def test_one_query_one_long_list(metric):
    I.case_long_list("cpu", metric)


@pytest.mark.parametrize("metric", ["euclidean", "inner_product"])
def test_filter(metric):
    I.case_filter("cpu", metric)


def test_query_chunks_are_bitwise_identical():
    I.case_chunking("cpu", "sqeuclidean")


@pytest.mark.parametrize("pq_len", [1, 3, 8, 32])
def test_encode(pq_len):
    I.case_encode("cpu", pq_len)


def test_end_to_end_with_training(tmp_path):
    I.case_end_to_end("cpu", str(tmp_path / "index.ivfpq"))


def test_argument_errors(tmp_path):
    f, index = I.forced_index("cpu", "sqeuclidean", 10, 4)
    for bad in (dict(x=f.x[0]), dict(x=f.x, params=IvfPqParams(metric="cosine")),
                dict(x=f.x, params=IvfPqParams(pq_dim=11), centroids=f.centroids),
                dict(x=f.x, params=IvfPqParams(pq_dim=-1), centroids=f.centroids),
                dict(x=f.x[:200], params=IvfPqParams(pq_dim=2), centroids=f.centroids),
                dict(x=f.x, centroids=f.centroids[:, :9], codebooks=f.books),
                dict(x=f.x, centroids=f.centroids, codebooks=f.books[:, :2]),
                dict(x=f.x, params=IvfPqParams(n_lists=0))):
        with pytest.raises(ValueError):
            ivf_pq_build(**bad)
    for call in (lambda: ivf_pq_search(index, f.q, 0),
                 lambda: ivf_pq_search(index, f.q[:, :9], 1),
                 lambda: ivf_pq_search(index, f.q, 1, filter=torch.ones(400)),
                 lambda: ivf_pq_search(index, f.q, 1, probes=torch.zeros(2, 1)),
                 lambda: ivf_pq_extend(index, f.x[:, :9]),
                 lambda: ivf_pq_extend(index, f.x[:2], torch.arange(3))):
        with pytest.raises(ValueError):
            call()
    empty = ivf_pq_build(f.x.half(), IvfPqParams(add_data_on_build=False), centroids=f.centroids)
    assert (empty.pq_dim, empty.n_rows) == (10, 0)           # default 16, capped at d
    assert bool((ivf_pq_search(empty, f.q, 3, 2)[1] == -1).all())
    assert ivf_pq_extend(empty, f.x[:5].bfloat16()).list_sizes.sum() == 5
    path = tmp_path / "not_an_index"
    path.write_bytes(b"RAFTAMD_IVFFLAT\x00" + bytes(80))
    with pytest.raises(ValueError):
        ivf_pq_load(str(path))
