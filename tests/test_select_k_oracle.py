"""The select_k oracle and checker (tests/select_k_inputs.py) tested on their
own, on the CPU: the oracle against torch.topk where NaN plays no part, and
the checker against hand-made wrong outputs. This is the evidence that the
GPU tests in tests/test_gpu_select_k.py can fail."""
import pytest
import torch

import select_k_inputs as S

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]


@pytest.mark.parametrize("select_min", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_oracle_matches_topk_without_nan(dtype, select_min):
    n = 100
    for name in S.NAN_FREE_FAMILIES:
        if not S.representable(name, n, dtype):
            continue
        x = S.family(name, 4, n, dtype)
        for k in (1, 17, n):
            ref = torch.topk(x.double(), k, dim=1, largest=not select_min).values
            assert torch.equal(S.oracle_topk(x, k, select_min), ref), (name, k)
            assert torch.equal(S.oracle_topk(x[0], k, select_min), ref[0])


@pytest.mark.parametrize("select_min", [True, False])
def test_oracle_puts_nan_last_and_after_inf(select_min):
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([nan, 2.0, -inf, -0.0, inf, -nan, 0.0, -3.0])
    out = S.oracle_topk(x, 8, select_min)
    want = [-inf, -3.0, 0.0, 0.0, 2.0, inf] if select_min else \
        [inf, 2.0, 0.0, 0.0, -3.0, -inf]
    assert out[:6].tolist() == want
    assert bool(torch.isnan(out[6:]).all())
    # NaN is chosen only once the row runs out of other values
    assert not bool(torch.isnan(S.oracle_topk(x, 6, select_min)).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_families_are_what_they_claim(dtype):
    n = 128 if dtype == torch.bfloat16 else 1000
    for name in S.families_for(n, dtype):
        x = S.family(name, 3, n, dtype)
        assert x is S.family(name, 3, n, dtype)          # cached, shared
        assert x.dtype == dtype and tuple(x.shape) == (3, n)
        d = x.double()
        if name == "ulp_ladder":
            ulp = 2.0 ** -S.MANT[dtype]
            want = 1 + torch.arange(n, dtype=torch.float64) * ulp
            assert torch.equal(d.sort(dim=1).values, want.expand(3, n))
        if name == "same_exponent":
            assert bool(((d >= 1) & (d < 2)).all())
        if name == "nan_mix":
            share = float(torch.isnan(d).float().mean())
            assert 0.2 < share < 0.4
            words = x.view(torch.int16 if x.element_size() == 2 else
                           torch.int32 if x.element_size() == 4 else torch.int64)
            nan_words = words[torch.isnan(x)]
            assert bool((nan_words < 0).any()) and bool((nan_words > 0).any())
            assert nan_words.unique().numel() > 10
        if name == "nan_tail":
            assert not bool(torch.isnan(d[:, :3]).any())
            assert bool(torch.isnan(d[:, 3:]).all())
        if name == "inf_heavy":
            assert float((d == float("inf")).float().mean()) > 0.8
            assert bool((d == float("-inf")).any())
        if name == "zeros_denormals":
            assert bool((d == 0).any()) and bool(torch.signbit(x[d == 0]).any())
            assert bool(((d != 0) & (d.abs() < 1.1e-38)).any())
    assert S.representable("zeros_denormals", n, dtype) == (x.element_size() >= 4)


@pytest.mark.parametrize("select_min", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_slab_order_follows_the_oracle(dtype, select_min):
    """The Python ordering of the generic engine's unsorted [batch, k] slab
    (plain torch, so it runs here too): numbers, then NaN, then pads."""
    from raft_amd.matrix.select_k import slab_order
    for name in ("randn", "inf_heavy", "nan_mix", "nan_tail", "few_values"):
        x = S.family(name, 4, 64, dtype)
        got = torch.gather(x, 1, slab_order(x, select_min)).double()
        assert bool(S._same(got, S.oracle_topk(x, 64, select_min)).all()), name
        # the last 9 slots flagged as pads: they go last, the rest keep the rule
        pad = torch.zeros(4, 64, dtype=torch.bool)
        pad[:, 55:] = True
        order = slab_order(x, select_min, pad=pad)
        assert bool((order[:, 55:] >= 55).all()), name
        got = torch.gather(x, 1, order[:, :55]).double()
        want = S.oracle_topk(x[:, :55], 55, select_min)
        assert bool(S._same(got, want).all()), name


# --------------------------------------------------------------------------
# the checker accepts a right answer and rejects each kind of wrong one
# --------------------------------------------------------------------------

def _right_answer(x, k, select_min):
    """A correct sorted (vals, idx) built from the oracle's own order."""
    _, order = S._oracle_order(x, select_min)
    idx = order[:, :k].contiguous()
    iv = S._INT_VIEW[x.dtype]          # integer gather: payloads survive
    return torch.gather(x.view(iv), 1, idx).view(x.dtype), idx


@pytest.fixture(params=[True, False], ids=["min", "max"])
def select_min(request):
    return request.param


def test_checker_accepts_right_answers(select_min):
    for name in S.FAMILIES:
        x = S.family(name, 3, 50)
        vals, idx = _right_answer(x, 8, select_min)
        S.check_select(x, vals, idx, 8, select_min, True)
        perm = torch.randperm(8, generator=torch.Generator().manual_seed(1))
        S.check_select(x, vals[:, perm], idx[:, perm], 8, select_min, False)
    # equal values may come back with any of their indices
    x = S.family("few_values", 3, 50)
    vals, idx = _right_answer(x, 8, select_min)
    tied = (x[0] == vals[0, 7]).nonzero().flatten()
    idx[0, 7] = tied[-1]
    S.check_select(x, vals, idx, 8, select_min, True)


def test_checker_rejects_int32_indices(select_min):
    x = S.family("randn", 3, 50)
    vals, idx = _right_answer(x, 8, select_min)
    with pytest.raises(AssertionError, match="int64"):
        S.check_select(x, vals, idx.int(), 8, select_min, True)


def test_checker_rejects_duplicated_index(select_min):
    x = S.family("all_equal", 3, 50)
    vals, idx = _right_answer(x, 8, select_min)
    idx[1, 5] = idx[1, 2]                  # values still right: all equal
    with pytest.raises(AssertionError, match="selected twice"):
        S.check_select(x, vals, idx, 8, select_min, True)


def test_checker_rejects_index_equal_to_n(select_min):
    x = S.family("randn", 3, 50)
    vals, idx = _right_answer(x, 8, select_min)
    idx[2, 0] = 50
    with pytest.raises(AssertionError, match="outside"):
        S.check_select(x, vals, idx, 8, select_min, True)
    idx[2, 0] = -1
    with pytest.raises(AssertionError, match="outside"):
        S.check_select(x, vals, idx, 8, select_min, True)


@pytest.mark.parametrize("sorted_", [True, False])
def test_checker_rejects_value_swapped_for_next(select_min, sorted_):
    x = S.family("randn", 3, 50)
    _, order = S._oracle_order(x, select_min)
    vals, idx = _right_answer(x, 8, select_min)
    idx[0, 7] = order[0, 8]                # the (k+1)-th in place of the k-th
    vals[0, 7] = x[0, idx[0, 7]]
    with pytest.raises(AssertionError, match="oracle has"):
        S.check_select(x, vals, idx, 8, select_min, sorted_)


def test_checker_rejects_gathered_value_mismatch(select_min):
    x = S.family("zeros_denormals", 3, 50)
    vals, idx = _right_answer(x, 50, select_min)
    zero = (vals[0] == 0).nonzero().flatten()[0]
    vals[0, zero] = -vals[0, zero]         # equal as a number, other sign bit
    with pytest.raises(AssertionError, match="bitwise"):
        S.check_select(x, vals, idx, 50, select_min, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_checker_counts_nan_payloads(select_min, dtype):
    x = S.family("nan_tail", 3, 50, dtype)
    vals, idx = _right_answer(x, 8, select_min)
    S.check_select(x, vals, idx, 8, select_min, True)
    vals[:, 3:] = float("nan")             # still NaN, another payload
    with pytest.raises(AssertionError, match="bitwise"):
        S.check_select(x, vals, idx, 8, select_min, True)


def test_checker_rejects_fabricated_pad(select_min):
    """A NaN slot replaced by +/-inf with index n-1: what the two-level split
    returned for a row whose last segment is all NaN."""
    n = 50
    x = S.family("nan_tail", 3, n)
    vals, idx = _right_answer(x, 8, select_min)
    assert bool(torch.isnan(vals[:, 3:]).all())
    vals[:, 3:] = float("inf") if select_min else float("-inf")
    idx[:, 3:] = n - 1
    with pytest.raises(AssertionError):
        S.check_select(x, vals, idx, 8, select_min, True)
    # even with distinct in-range indices the values give it away
    idx[:, 3:] = torch.arange(n - 5, n)
    with pytest.raises(AssertionError, match="bitwise"):
        S.check_select(x, vals, idx, 8, select_min, True)


def test_checker_rejects_nan_first(select_min):
    """Selected NaNs ahead of the numbers: what a descending torch sort gives."""
    x = S.family("nan_tail", 3, 50)
    vals, idx = _right_answer(x, 8, select_min)
    vals, idx = vals.roll(5, dims=1), idx.roll(5, dims=1)
    assert bool(torch.isnan(vals[:, 0]).all())
    with pytest.raises(AssertionError, match="oracle has"):
        S.check_select(x, vals, idx, 8, select_min, True)
    S.check_select(x, vals, idx, 8, select_min, False)   # a valid multiset


def _ragged_answer(x, lens, k, select_min):
    pad = float("inf") if select_min else float("-inf")
    vals = torch.full((len(lens), k), pad, dtype=x.dtype)
    idx = torch.full((len(lens), k), -1, dtype=torch.int64)
    for r, ln in enumerate(lens):
        m = min(k, ln)
        v, i = _right_answer(x[r:r + 1, :ln], m, select_min)
        vals[r, :m], idx[r, :m] = v[0], i[0]
    return vals, idx


@pytest.mark.parametrize("name", ["nan_mix", "inf_heavy", "few_values"])
def test_checker_ragged_rows(select_min, name):
    k = 8
    lens = S.ragged_lens(k, 200)
    x = S.family(name, len(lens), 200)
    vals, idx = _ragged_answer(x, lens, k, select_min)
    S.check_select(x, vals, idx, k, select_min, True, pad_lens=lens)

    # a pad ahead of a real entry (row of length k-1: slots 0..6 real)
    v, i = vals.clone(), idx.clone()
    v[2, [6, 7]], i[2, [6, 7]] = v[2, [7, 6]], i[2, [7, 6]]
    with pytest.raises(AssertionError):
        S.check_select(x, v, i, k, select_min, True, pad_lens=lens)
    # a pad that keeps a real index, and a pad of the wrong sign
    i = idx.clone()
    i[1, 3] = 0
    with pytest.raises(AssertionError, match="expected a pad"):
        S.check_select(x, vals, i, k, select_min, True, pad_lens=lens)
    v = vals.clone()
    v[0, 0] = -v[0, 0]
    with pytest.raises(AssertionError, match="expected a pad"):
        S.check_select(x, v, idx, k, select_min, True, pad_lens=lens)
    # an index past the row's own length but inside the matrix
    i = idx.clone()
    i[1, 0] = 1
    with pytest.raises(AssertionError, match="outside"):
        S.check_select(x, vals, i, k, select_min, True, pad_lens=lens)


def test_checker_rejects_real_nan_after_pad():
    """select-min CSR rows sorted with pads as +inf: the row's NaN lands after
    the pads."""
    k = 8
    lens = S.ragged_lens(k, 200)
    x = S.family("nan_tail", len(lens), 200)
    vals, idx = _ragged_answer(x, lens, k, True)
    assert bool(torch.isnan(vals[2, 6]))          # row of length 7: 3 numbers, 4 NaN
    vals[2, [6, 7]], idx[2, [6, 7]] = vals[2, [7, 6]], idx[2, [7, 6]]
    with pytest.raises(AssertionError):
        S.check_select(x, vals, idx, k, True, True, pad_lens=lens)
