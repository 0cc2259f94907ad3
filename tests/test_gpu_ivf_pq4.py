"""IVF-PQ with 4-bit codes on the GPU (csrc/ivf_pq4.hip) against
tests/ivf_pq4_inputs.py."""
import pytest
import torch

import ivf_pq4_inputs as C
import ivf_pq_inputs as I
from raft_amd.neighbors import ivf_pq_search

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,pq_dim", C.SHAPES)
@pytest.mark.parametrize("metric", I.METRICS)
def test_search_vs_oracle(metric, d, pq_dim):
    C.case_search("cuda", metric, d, pq_dim)


@pytest.mark.parametrize("metric", I.METRICS)
def test_one_query_one_long_list(metric):
    C.case_long_list("cuda", metric)


@pytest.mark.parametrize("metric", ["euclidean", "inner_product"])
def test_filter(metric):
    C.case_filter("cuda", metric)


def test_query_chunks_are_bitwise_identical():
    C.case_chunking("cuda", "sqeuclidean")


@pytest.mark.parametrize("pq_len", [1, 3, 8, 32])
def test_encode_and_equal_codes_on_cpu_and_gpu(pq_len):
    """Both obey the encode rule, so codes can differ only at near ties."""
    assert torch.equal(C.case_encode("cuda", pq_len)[100:], C.case_encode("cpu", pq_len)[100:])


def test_bytes_at_the_documented_addresses():
    C.case_layout("cuda")


@pytest.mark.parametrize("metric", I.METRICS)
def test_cpu_index_moved_with_the_cpu_probes(metric):
    f, cpu = C.forced_index("cpu", metric, 33, 33)
    _, _, p = ivf_pq_search(cpu, f.q, 9, 3, return_probes=True)
    d1, i1 = ivf_pq_search(cpu.to("cuda"), f.q.to("cuda"), 9, probes=p.to("cuda"))
    I.check(cpu, f.q, p, d1, i1, 9)


def test_end_to_end_with_training(tmp_path):
    C.case_end_to_end("cuda", str(tmp_path / "index.ivfpq"))


def test_wider_than_the_kernels_takes_the_torch_path():
    f, index = C.forced_index("cuda", "sqeuclidean", 257, 257)
    assert not index.kernels_serve
    d, i, p = ivf_pq_search(index, f.q.to("cuda"), 9, 3, return_probes=True)
    I.check(index, f.q, p, d, i, 9)
