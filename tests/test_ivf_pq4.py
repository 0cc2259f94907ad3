"""IVF-PQ with 4-bit codes on the CPU (the plain-torch path, which defines the
results) against tests/ivf_pq4_inputs.py."""
import pytest

import ivf_pq4_inputs as C
import ivf_pq_inputs as I


@pytest.mark.parametrize("d,pq_dim", C.SHAPES)
@pytest.mark.parametrize("metric", I.METRICS)
def test_search_vs_oracle(metric, d, pq_dim):
    C.case_search("cpu", metric, d, pq_dim)


@pytest.mark.parametrize("metric", I.METRICS)
def test_one_query_one_long_list(metric):
    C.case_long_list("cpu", metric)


@pytest.mark.parametrize("metric", ["euclidean", "inner_product"])
def test_filter(metric):
    C.case_filter("cpu", metric)


def test_query_chunks_are_bitwise_identical():
    C.case_chunking("cpu", "sqeuclidean")


@pytest.mark.parametrize("pq_len", [1, 3, 8, 32])
def test_encode(pq_len):
    C.case_encode("cpu", pq_len)


def test_bytes_at_the_documented_addresses():
    C.case_layout("cpu")


def test_end_to_end_with_training(tmp_path):
    C.case_end_to_end("cpu", str(tmp_path / "index.ivfpq"))
