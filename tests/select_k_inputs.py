"""Shared oracle, checker and adversarial inputs for the select_k tests
(tests/test_select_k_oracle.py on the CPU, tests/test_gpu_select_k.py on the
GPU). Everything here runs on the CPU in fp64, where bf16, fp16 and fp32 embed
exactly, so every comparison is exact: no tolerance appears anywhere. Inputs
are computed once per process and never modified."""
import functools

import torch

#: every input family, in the order the tests parametrise them
FAMILIES = ["randn", "ulp_ladder", "same_exponent", "few_values", "all_equal",
            "inf_heavy", "zeros_denormals", "nan_mix", "nan_tail", "ascending",
            "descending"]
NAN_FAMILIES = ("nan_mix", "nan_tail")
NAN_FREE_FAMILIES = [f for f in FAMILIES if f not in NAN_FAMILIES]

#: explicit mantissa bits: 1 + i * 2**-MANT[dtype] is exact for i < 2**MANT
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23,
        torch.float64: 52}
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16,
             torch.float32: torch.int32, torch.float64: torch.int64}
_EXP_BITS = {torch.bfloat16: 8, torch.float16: 5, torch.float32: 8,
             torch.float64: 11}


def representable(family, n, dtype):
    """Whether `family` can be built at row length n in dtype."""
    if family == "zeros_denormals":
        return dtype in (torch.float32, torch.float64)
    if family == "ulp_ladder":
        return n <= (1 << MANT[dtype])
    return True


def families_for(n, dtype):
    return [f for f in FAMILIES if representable(f, n, dtype)]


# --------------------------------------------------------------------------
# oracle
# --------------------------------------------------------------------------

def _oracle_order(x, select_min):
    """fp64 copy of a [batch, n] matrix and the column order of the oracle:
    numeric order (reversed for select-max) over finite values and +/-inf,
    then every NaN. -0.0 == +0.0. Two stable sorts: by key, then by is-NaN."""
    d = x.detach().cpu().double()
    nan = torch.isnan(d)
    key = torch.where(nan, torch.zeros_like(d), d if select_min else -d)
    o1 = torch.argsort(key, dim=1, stable=True)
    o2 = torch.argsort(torch.gather(nan, 1, o1).to(torch.uint8), dim=1,
                       stable=True)
    return d, torch.gather(o1, 1, o2)


def oracle_topk(x, k, select_min):
    """Sorted top-k values (fp64) of a row [n] or of each row of [batch, n]."""
    one_row = x.dim() == 1
    d, order = _oracle_order(x.unsqueeze(0) if one_row else x, select_min)
    assert 0 <= k <= d.shape[1], (k, d.shape)
    out = torch.gather(d, 1, order[:, :k])
    return out[0] if one_row else out


# --------------------------------------------------------------------------
# checker
# --------------------------------------------------------------------------

def _same(a, b):
    """fp64 a == b, or both NaN."""
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def _first_bad(ok):
    r, c = (~ok).nonzero()[0].tolist()
    return r, c


def check_select(x, vals, idx, k, select_min, sorted, pad_lens=None):
    """Assert that (vals, idx) is a valid top-k of every row of the CPU matrix
    x [batch, n]. With pad_lens (one length per row) only x[r, :pad_lens[r]]
    is the row; slots past min(k, len) must be +/-inf pads with index -1.

    Distinct in-range indices, gathered values bitwise equal to the output,
    and the output equal to the oracle multiset together prove the top-k."""
    x = x.detach().cpu()
    vals, idx = vals.detach().cpu(), idx.detach().cpu()
    batch, n = x.shape
    assert idx.dtype == torch.int64, f"idx dtype {idx.dtype}, want int64"
    assert vals.dtype == x.dtype, f"vals dtype {vals.dtype}, want {x.dtype}"
    assert tuple(vals.shape) == (batch, k), (tuple(vals.shape), (batch, k))
    assert tuple(idx.shape) == (batch, k), (tuple(idx.shape), (batch, k))
    if pad_lens is None:
        lens = torch.full((batch,), n, dtype=torch.int64)
    else:
        lens = torch.as_tensor(pad_lens, dtype=torch.int64)
        assert lens.shape == (batch,) and int(lens.max()) <= n
    m = lens.clamp(max=k)
    slot = torch.arange(k).unsqueeze(0)
    real = slot < m.unsqueeze(1)                       # [batch, k]

    # pads: exactly +/-inf with index -1, after every real entry
    pad_val = float("inf") if select_min else float("-inf")
    ok = real | ((idx == -1) & (vals.double() == pad_val))
    if not bool(ok.all()):
        r, c = _first_bad(ok)
        raise AssertionError(
            f"row {r} (len {int(lens[r])}) slot {c}: expected a pad "
            f"({pad_val}, -1), got ({vals[r, c].item()}, {int(idx[r, c])})")

    # real slots: index in [0, len)
    ok = ~real | ((idx >= 0) & (idx < lens.unsqueeze(1)))
    if not bool(ok.all()):
        r, c = _first_bad(ok)
        raise AssertionError(f"row {r} slot {c}: index {int(idx[r, c])} "
                             f"outside [0, {int(lens[r])})")

    # pairwise distinct within a row (pads get distinct negative stand-ins)
    uniq = torch.where(real, idx, -1 - slot.expand(batch, k))
    srt = uniq.sort(dim=1).values
    ok = srt[:, 1:] != srt[:, :-1]
    if not bool(ok.all()):
        r, c = _first_bad(ok)
        raise AssertionError(f"row {r}: index {int(srt[r, c])} selected twice")

    # x[row, idx] is bitwise vals (NaN payloads and zero signs count); gather
    # the integer view: a CPU gather of half floats rewrites NaN payloads
    got = torch.gather(x.contiguous().view(_INT_VIEW[x.dtype]), 1,
                       idx.clamp(min=0))
    ok = ~real | (got == vals.contiguous().view(_INT_VIEW[x.dtype]))
    if not bool(ok.all()):
        r, c = _first_bad(ok)
        raise AssertionError(
            f"row {r} slot {c}: vals {vals[r, c].item()} is not bitwise "
            f"x[{r}, {int(idx[r, c])}] = {x[r, int(idx[r, c])].item()}")

    # values equal the oracle, position by position
    v = vals.double()
    if pad_lens is None:
        ref = oracle_topk(x, k, select_min)
        if not sorted:
            v = oracle_topk(v, k, select_min)
        ok = _same(v, ref)
    else:
        ok = torch.ones(batch, k, dtype=torch.bool)
        for r in range(batch):
            mr = int(m[r])
            ref = oracle_topk(x[r, :int(lens[r])], mr, select_min)
            vr = v[r, :mr] if sorted else oracle_topk(v[r, :mr], mr, select_min)
            ok[r, :mr] = _same(vr, ref)
    if not bool(ok.all()):
        r, c = _first_bad(ok)
        want = oracle_topk(x[r, :int(lens[r])], int(m[r]), select_min)
        raise AssertionError(
            f"row {r} slot {c} ({'sorted' if sorted else 'multiset'}): got "
            f"{vals[r, c].item()}, oracle has {want[c].item()}; "
            f"{int((~ok).sum())} slots differ in all")


# --------------------------------------------------------------------------
# input families: cached functions of (batch, n, dtype, seed) -> CPU tensor
# --------------------------------------------------------------------------

def _gen(name, batch, n, seed):
    g = torch.Generator()
    g.manual_seed(1000003 * seed + 7919 * FAMILIES.index(name) + 31 * batch + n)
    return g


def _mantissa_grid(i, dtype):
    """1 + i * ulp(1) as dtype, exact for 0 <= i < 2**MANT[dtype]."""
    out = (1.0 + i.double() * 2.0 ** -MANT[dtype]).to(dtype)
    assert bool((out.double() >= 1).all()) and bool((out.double() < 2).all())
    return out


def _random_nans(shape, dtype, g):
    """NaNs of both signs with assorted payloads (quiet and signalling)."""
    mant, bits = MANT[dtype], MANT[dtype] + _EXP_BITS[dtype] + 1
    payload = torch.randint(1, 1 << mant, shape, generator=g, dtype=torch.int64)
    exp_all_ones = ((1 << _EXP_BITS[dtype]) - 1) << mant
    word = payload | exp_all_ones                      # sign bit still clear
    neg = torch.randint(0, 2, shape, generator=g).bool()
    # set the sign bit in two's complement: word - 2**(bits-1)
    word = torch.where(neg, word + (-(1 << (bits - 1))), word)
    out = word.to(_INT_VIEW[dtype]).view(dtype)
    assert bool(torch.isnan(out).all())
    return out


@functools.lru_cache(maxsize=None)
def family(name, batch, n, dtype=torch.float32, seed=0):
    assert representable(name, n, dtype), (name, n, dtype)
    g = _gen(name, batch, n, seed)
    if name == "randn":
        x = torch.randn(batch, n, generator=g).to(dtype)
    elif name == "ulp_ladder":
        # shuffled 1 + i*ulp: the k-th value is decided by the LAST radix byte
        i = torch.argsort(torch.rand(batch, n, generator=g), dim=1)
        x = _mantissa_grid(i, dtype)
    elif name == "same_exponent":
        # uniform in [1, 2): the whole row shares the top ordinal byte
        i = torch.randint(0, 1 << MANT[dtype], (batch, n), generator=g,
                          dtype=torch.int64)
        x = _mantissa_grid(i, dtype)
    elif name == "few_values":
        x = torch.randint(0, 8, (batch, n), generator=g).to(dtype)
    elif name == "all_equal":
        x = torch.full((batch, n), 1.5, dtype=dtype)
    elif name == "inf_heavy":
        u = torch.rand(batch, n, generator=g)
        x = torch.randn(batch, n, generator=g).to(dtype)
        x[u < 0.90] = float("inf")
        x[(u >= 0.90) & (u < 0.91)] = float("-inf")
    elif name == "zeros_denormals":
        table = torch.tensor([-0.0, 0.0, 1e-40, -1e-40, 1e-38, -1e-38],
                             dtype=dtype)
        x = table[torch.randint(0, 6, (batch, n), generator=g)]
    elif name == "nan_mix":
        x = torch.randn(batch, n, generator=g).to(dtype)
        nans = _random_nans((batch, n), dtype, g)
        x = torch.where(torch.rand(batch, n, generator=g) < 0.30, nans, x)
    elif name == "nan_tail":
        x = _random_nans((batch, n), dtype, g)
        x[:, :3] = torch.randn(batch, min(n, 3), generator=g).to(dtype)
    elif name in ("ascending", "descending"):
        x = torch.randn(batch, n, generator=g).to(dtype)
        x = x.sort(dim=1, descending=(name == "descending")).values
    else:
        raise ValueError(name)
    assert x.dtype == dtype and tuple(x.shape) == (batch, n)
    return x.contiguous()


def ragged_lens(k, longest):
    """Row lengths around k: empty, one, k-1, k, k+1 and a long row."""
    return [0, 1, k - 1, k, k + 1, longest]
