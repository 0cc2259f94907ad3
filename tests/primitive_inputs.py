"""Shared input families, fp64 oracles, checkers and launcher arithmetic for
the primitive-kernel tests (tests/test_primitive_oracle.py on the CPU,
tests/test_gpu_primitives.py on the GPU): row/column reductions, row argmin,
row normalize, bf16 row norms, linewise, histogram, bitset, CSR SpMV, SDDMM.

Everything here runs on the CPU. The main families are integer-valued with
|v| <= 8, so every product and every partial sum is an integer below 2^24 and
therefore exact in fp32 (and bf16 holds the inputs exactly): on them a kernel
must EQUAL the fp64 oracle whatever its summation order. `exact_ok` is that
condition; the oracle test asserts it for every case. Inputs are built from a
seed, cached per process and never modified."""
import functools
import math

import torch

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}  # unit roundoff
INT_LIM = 8
OPS = (0, 1, 2, 3, 4, 5)  # sum x, sum x^2, sum |x|, max x, min x, max |x|
SUM_OPS = (0, 1, 2)
WAVE = 64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------
# launcher arithmetic (mirrors csrc/*.hip; the oracle test checks that the
# shapes below reach the routes their names claim)
# --------------------------------------------------------------------------

def rows_route(n, d):
    """launch_reduce_rows: kernel, logical-warp width, grid, grid-stride passes."""
    if d <= 256:
        lw = 2 if d <= 4 else 8 if d <= 16 else 32 if d <= 64 else 64
        blocks = (n * lw + 255) // 256
        grid = min(blocks, 2048)               # grid_1d cap
        per_pass = grid * (256 // lw)
        return dict(kernel="thin", lw=lw, grid=grid,
                    passes=-(-n // per_pass))
    grid = min(n, 2048)
    return dict(kernel="block", lw=None, grid=grid, passes=-(-n // grid))


def cols_route(n, d):
    """launch_reduce_cols: kernel, gx, gy, rows_per_tile."""
    if d < 32 and n >= 4096:
        gy = min(1024, (n + 4095) // 4096)
        dp2 = 1
        while dp2 < d:
            dp2 <<= 1
        return dict(kernel="skinny", gx=1, gy=gy, rows_per_tile=-(-n // gy),
                    rpt=WAVE // dp2)
    gx = (d + 255) // 256
    gy = max(1, min((512 + gx - 1) // gx, (n + 1023) // 1024))
    return dict(kernel="general", gx=gx, gy=gy, rows_per_tile=-(-n // gy))


def capped_passes(n, cap):
    """Grid-stride passes of a one-block-per-row kernel capped at `cap` blocks."""
    return -(-n // min(n, cap))


def histogram_strategy(n_bins):
    """launch_histogram: NW = 256 / 64 = 4 waves; LDS-MULTI while
    NW * n_bins * 4 B <= 64 KiB, LDS-SINGLE while n_bins * 4 B <= 64 KiB."""
    if 4 * n_bins * 4 <= 65536:
        return "lds_multi"
    if n_bins * 4 <= 65536:
        return "lds_single"
    return "gmem"


def spmv_width(n_rows, nnz):
    """launch_csr_spmv: sub-wave width from ceil(nnz / n_rows)."""
    mean = -(-nnz // n_rows) if n_rows else 1
    for lim, sw in ((4, 2), (8, 4), (16, 8), (32, 16), (128, 32)):
        if mean <= lim:
            return sw
    return 64


def sddmm_width(d):
    return 4 if d <= 8 else 16 if d <= 32 else 32 if d <= 128 else 64


def linewise_blocks(n, d):
    """launch_linewise: blocks before the 4096 cap."""
    return max(1, (n * d // 4 + 255) // 256)


# --- uncompensated adds per output, counted from the kernels ---------------
# Every per-thread accumulator is Kahan-Babushka-Neumaier, i.e. Sum2 of Ogita,
# Rump and Oishi (2005): its result carries at most u|s| + gamma_{k-1}^2
# sum|x_i| over the k terms the thread adds. No thread sees more than 4096
# terms in any case here, so k^2 u^2 <= u and the accumulator counts as 2.
# Each later plain add of two partials p, q rounds by at most u|p + q| <=
# u sum|x_i| and counts as 1. Op 1 rounds each product x * x once more before
# it is added: one more u sum|x_i^2|, PRODUCT_ROUNDING.
KAHAN = 2
PRODUCT_ROUNDING = 1


def rows_adds(n, d):
    r = rows_route(n, d)
    if r["kernel"] == "thin":
        return KAHAN + int(math.log2(r["lw"]))   # log2(LW) shuffle steps
    return KAHAN + 6 + 4                         # 6 shuffle steps + 4 wave partials


def cols_adds(n, d):
    r = cols_route(n, d)
    if r["kernel"] == "skinny":
        # log2(rpt) shuffle steps, then one atomic per (wave, tile): 4 * gy
        return KAHAN + int(math.log2(r["rpt"])) + 4 * r["gy"]
    # four accumulators per thread: a1..a3 are folded into a0 with compensated
    # adds, but each of their get() calls is a plain sum + c that rounds (3);
    # gy > 1 adds one atomic partial per row tile
    return KAHAN + 3 + (r["gy"] if r["gy"] > 1 else 0)


NORMALIZE_SUM_ADDS = KAHAN + 6 + 4   # row_normalize_l2: as the block kernel


# --------------------------------------------------------------------------
# shapes the issue fixes
# --------------------------------------------------------------------------

# 1027 gives 1027 // 4 = 256 float4 per row: exactly ONE trip of the 256-thread
# float4 loop (and five trips of the scalar loops of min/max and fp64); 1031
# is added so that thread 0 takes a second float4 trip
ROWS_D = (1, 4, 5, 16, 17, 64, 65, 256, 257, 260, 1027, 1031)
ROWS_N = (1, 3, 33)
ROWS_SECOND_PASS = ((262150, 3), (8200, 65), (2050, 257))
COLS_GENERAL = ((1000, 33), (1025, 33), (2051, 300), (4095, 8))
COLS_SKINNY = tuple((n, d) for n in (4096, 4097, 8195)
                    for d in (1, 2, 3, 16, 17, 31))
ARGMIN_D = (1, 255, 256, 257, 777)
ARGMIN_ROWS = 2050
# 2055 // 8 = 256 bf16x8 vectors: one trip of the vector loop plus a 7-element
# tail; 2063 is added so that thread 0 takes a second vector trip. 65537 rows
# (second grid-stride pass) pair with d <= 9 only: 65537 x 2055 would be a
# 270 MB case
SQNORM_D = (1, 7, 8, 9, 2055, 2063)
SQNORM_N = (3, 65537)
SQNORM_SHAPES = tuple((n, d) for n in SQNORM_N for d in SQNORM_D
                      if n * d * 2 <= 8 << 20)
LINEWISE_SHAPES = ((1, 1), (1, 4), (3, 5), (333, 129), (4100, 1028))
LW_OPS = ("add", "sub", "mul", "div")
HIST_BINS = (1, 256, 4096, 4097, 16384, 16385)
HIST_D = (1, 3, 513)
HIST_N = (1, 4097, 20001)
BITSET_N = (31, 32, 33, 1000003)
BITSET_COUNT_BITS = 32 * (2048 * 256 + 77)   # more words than one grid pass
SPMV_L = (1, 4, 5, 8, 9, 16, 17, 32, 33, 128, 129, 300)
SPMV_ROWS = 37
SPMV_COLS = 411
SDDMM_D = (1, 8, 9, 32, 33, 128, 129, 300)
SDDMM_NNZ = (0, 1, 1000)


# --------------------------------------------------------------------------
# reductions
# --------------------------------------------------------------------------

def _main(v, op):
    if op == 1:
        return v * v
    if op in (2, 5):
        return v.abs()
    return v


def reduce_oracle(x, op, dim):
    """fp64 result of reduce op along dim (1: each row, 0: each column).
    NaN propagates through min/max as in torch; +/-inf sums as IEEE."""
    v = _main(x.detach().cpu().double(), op)
    if op <= 2:
        return v.sum(dim=dim)
    if op == 4:
        return v.min(dim=dim).values
    return v.max(dim=dim).values


def abs_mass(x, op, dim):
    """fp64 sum |main_op(x_i)| per output: the scale of every error bound."""
    return _main(x.detach().cpu().double(), op).abs().sum(dim=dim)


def _fsum_rows(m):
    return torch.tensor([math.fsum(r) for r in m.numpy()], dtype=torch.float64)


def exact_sum_oracle(x, op, dim):
    """Correctly rounded fp64 sums (math.fsum) for non-integer inputs, where
    an fp64 torch.sum would carry an error of the size under test when x is
    fp64 itself. Needs values with at most 24 significant bits, so that x * x
    is exact in fp64; what is left is one rounding, below 2^-53 |ref|."""
    v = x.detach().cpu().double()
    assert torch.equal(v, v.float().double()), "values must be fp32-representable"
    m = _main(v, op)
    return _fsum_rows(m if dim == 1 else m.t().contiguous())


def exact_ok(x, op, dim):
    """Integer-valued inputs whose every partial sum stays below 2^24."""
    xd = x.detach().cpu().double()
    return bool((xd == xd.round()).all()) and \
        float(abs_mass(x, op, dim).max()) < 2.0 ** 24


def same(a, b):
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def check_equal(out, ref, what=""):
    """out (any float/int dtype) equals the fp64/int64 ref, NaN == NaN."""
    o = out.detach().cpu()
    assert o.shape == ref.shape, f"{what}: shape {tuple(o.shape)} != {tuple(ref.shape)}"
    if ref.is_floating_point():
        ok = same(o.double(), ref)
    else:
        ok = o.to(torch.int64) == ref
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: first mismatch at {i}: got {o[i].item()!r}, "
                             f"want {ref[i].item()!r} ({int((~ok).sum())} wrong)")


def check_bound(out, ref, bound, what=""):
    """|out - ref| <= bound elementwise, everything in fp64."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, f"{what}: shape"
    err = (o - ref).abs()
    ok = err <= bound
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: at {i} error {err[i].item():.3e} > bound "
                             f"{bound[i].item():.3e}")
    return float((err / bound.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def int_matrix(n, d, seed=0, lo=-INT_LIM, hi=INT_LIM):
    """fp32 [n, d] of random integers in [lo, hi]."""
    return torch.randint(lo, hi + 1, (n, d), generator=_gen(seed)).float()


def boundary_positions(length, marks):
    """0, length-1 and both sides of every boundary in marks, inside range."""
    pos = {0, length - 1}
    for m in marks:
        pos.update((m - 1, m))
    return sorted(p for p in pos if 0 <= p < length)


def row_marks(n, d):
    """Lane, wave, tile and float4-tail boundaries along a reduced row."""
    r = rows_route(n, d)
    lw = r["lw"] or 256
    return boundary_positions(d, (lw, 2 * lw, WAVE, 128, 192, 256, 512,
                                  (d // 4) * 4))


def col_marks(n, d):
    """Row-tile, wave-step and r % 4 tail boundaries along a reduced column."""
    r = cols_route(n, d)
    t = r["rows_per_tile"]
    marks = [t * k for k in range(1, r["gy"])][:3] + [t * (r["gy"] - 1)]
    if r["kernel"] == "skinny":
        marks += [r["rpt"], 4 * r["rpt"]]
    marks += [4, (n // 4) * 4]
    return boundary_positions(n, marks)


def spike_matrix(n, d, dim, seed=1):
    """Integers in [-4, 4] with, along the reduced axis of each output, one +9
    and one -10 planted at boundary positions that rotate from output to
    output. max is 9, min is -10, max|x| is 10, wherever they sit; a kernel
    that skips a position loses one of them."""
    x = int_matrix(n, d, seed, -4, 4).clone()
    if dim == 1:
        pos = row_marks(n, d)
        for r in range(n if n <= 64 else 64):
            x[r, pos[r % len(pos)]] = 9
            x[r, pos[(r + 1) % len(pos)]] = -10
        if n > 64:   # tall matrices: also mark the last rows (second pass)
            for r in range(n - 8, n):
                x[r, pos[r % len(pos)]] = 9
                x[r, pos[(r + 1) % len(pos)]] = -10
    else:
        pos = col_marks(n, d)
        for c in range(d):
            x[pos[c % len(pos)], c] = 9
            x[pos[(c + 1) % len(pos)], c] = -10
    return x


def signed_matrix(n, d, sign, seed=2):
    """All-positive (1..8) or all-negative (-8..-1): a wrong min/max identity
    (0 in place of -/+inf) shows up here."""
    return int_matrix(n, d, seed, 1, INT_LIM) * sign


def cancel_matrix(n, d, dim, dtype, seed=3):
    """Random values with a cancellation pattern along the reduced axis: large
    +/-B pairs around small terms (needs a reduced length >= 3). Every value
    is fp32-representable in either dtype (see exact_sum_oracle); in fp64 the
    pairs are 2^57 and up, beyond 2^53 times the small terms, so a plain fp64
    sum loses them altogether."""
    x = torch.randn(n, d, generator=_gen(seed), dtype=torch.float32).double()
    big = 2.0 ** 27 if dtype == torch.float32 else 2.0 ** 57
    length = d if dim == 1 else n
    if length >= 3:
        g = _gen(seed + 1)
        for k in range(min(6, length // 2)):
            i, j = torch.randperm(length, generator=g)[:2].tolist()
            b = big * (k + 1)
            if dim == 1:
                x[:, i], x[:, j] = b, -b
            else:
                x[i, :], x[j, :] = b, -b
    return x.to(dtype)


def drift_matrix():
    """[2, 2^17] rows of the constant 0.1 and 0.7 (fp32): every add of a plain
    accumulator rounds the same way within a binade, so 512 terms per thread
    drift far beyond a few u sum|x|, while a compensated sum does not."""
    return torch.tensor([[0.1], [0.7]], dtype=torch.float32).repeat(1, 1 << 17)


def nan_positions_matrix(n, d, dim, seed=4):
    """spike_matrix with one NaN per output at rotating boundary positions
    (first, last, mid-lane, each tile); output 0 keeps no NaN as a control."""
    x = spike_matrix(n, d, dim, seed).clone()
    if dim == 1:
        pos = row_marks(n, d) + [d // 2]
        for r in range(1, n):
            x[r, pos[r % len(pos)]] = float("nan")
    else:
        pos = col_marks(n, d) + [n // 2]
        for c in range(1, d):
            x[pos[c % len(pos)], c] = float("nan")
    return x


def nonfinite_sum_rows(d, dtype):
    """[6, d] rows: +inf present, -inf present, both, NaN, positive overflow,
    negative overflow; the rest small integers. Built for d >= 4."""
    assert d >= 4
    big = 3e38 if dtype == torch.float32 else 1.5e308
    x = int_matrix(6, d, 5, -2, 2).clone().to(dtype)
    inf = float("inf")
    x[0, d // 2] = inf
    x[1, d - 1] = -inf
    x[2, 0], x[2, d - 1] = inf, -inf
    x[3, d // 3] = float("nan")
    x[4, :4] = big
    x[5, d - 4:] = -big
    return x


def nonfinite_oracle(x, op, dim):
    """What the CPU path gives: the fp64 result rounded to x's dtype (an fp32
    overflow becomes +/-inf), back in fp64 for comparison."""
    return reduce_oracle(x, op, dim).to(x.dtype).double()


# --------------------------------------------------------------------------
# argmin / argmax
# --------------------------------------------------------------------------

def argmin_oracle(x):
    """Lowest index of the minimum of each row; the first NaN if any."""
    d = x.detach().cpu().double()
    nan = torch.isnan(d)
    key = torch.where(nan, torch.full_like(d, -float("inf")), d)
    has_nan = nan.any(dim=1)
    # in a row with a NaN only a NaN may win, whatever else (-inf) it holds
    key = torch.where(has_nan.unsqueeze(1) & ~nan, torch.full_like(d, float("inf")), key)
    m = key.min(dim=1, keepdim=True).values
    idx = torch.arange(d.shape[1]).expand_as(d)
    big = d.shape[1]
    return torch.where(key == m, idx, torch.full_like(idx, big)).min(dim=1).values


@functools.lru_cache(maxsize=None)
def argmin_matrix(d, n=ARGMIN_ROWS, seed=6):
    """[n, d] fp32 integers in [0, 50] with engineered rows at the top AND at
    the bottom (rows past 2048 run in the second grid-stride pass):
    duplicated minimum at (j, j+1), (j, j+64), (j, j+256), (first, last), an
    all-equal row, an all-+inf row, a row with -inf, +inf-padded rows."""
    x = torch.randint(0, 51, (n, d), generator=_gen(seed)).float()
    inf = float("inf")

    def plant(r, cols, v=-3.0):
        for c in cols:
            if 0 <= c < d:
                x[r, c] = v

    for base in (0, n - 16):
        r = base
        for j in (0, 62, 63, 190, 254, 255):
            for gap in (1, 64, 256):
                if j + gap < d and r < base + 12:
                    plant(r, (j + gap, j))
                    r += 1
        plant(base + 12, (0, d - 1))
        x[base + 13, :] = 7.0
        x[base + 14, :] = inf
        x[base + 15, :] = inf
        plant(base + 15, (d - 1,), 5.0)
        plant(base + 15, (d // 2,), -inf)
        if d > 2:
            plant(base + 15, (d - 2,), -inf)
    return x


def argmin_nan_matrix(d, n=40, seed=7):
    """Rows with one or two NaN at boundary positions; row 0 has none. Some
    rows also hold -inf, which must not beat the NaN."""
    x = torch.randint(0, 51, (n, d), generator=_gen(seed)).float()
    pos = boundary_positions(d, (1, 63, 64, 65, 128, 256, d // 2))
    for r in range(1, n):
        x[r, pos[r % len(pos)]] = float("nan")
        if r % 3 == 0:
            x[r, pos[(r + 2) % len(pos)]] = float("nan")
        if r % 4 == 0 and d > 1:
            c = pos[(r + 1) % len(pos)]
            if not math.isnan(float(x[r, c])):
                x[r, c] = -float("inf")
    return x


# --------------------------------------------------------------------------
# histogram
# --------------------------------------------------------------------------

HIST_LO, HIST_HI = -4.0, 4.0


@functools.lru_cache(maxsize=None)
def dyadic_matrix(n, d, seed=8):
    """Multiples of 2^-6 in [-4, 4): (v - lo) * (n_bins / 8) is then an
    integer multiple of 2^-9 below 2^24 * 2^-9, exact in fp32 for every
    n_bins <= 16385."""
    k = torch.randint(-256, 256, (n, d), generator=_gen(seed))
    return (k.double() / 64).float()


def hist_edge_matrix(d):
    """Values below lo, above hi, exactly lo, exactly hi, +/-inf, NaN, and
    interior points, repeated over d columns with a per-column rotation."""
    inf, nan = float("inf"), float("nan")
    base = torch.tensor([-4.0, 4.0, -4.5, 1e30, -1e30, 4.0 - 2.0 ** -6, inf, -inf,
                         nan, 0.0, -0.0, 3.984375, nan, 1.0, -1.0, 2.5],
                        dtype=torch.float32)
    cols = [torch.roll(base, j) for j in range(d)]
    return torch.stack(cols, dim=1).contiguous()


def histogram_oracle(x, n_bins, lo, hi):
    """Exact fp64 binning: floor((v - lo) / (hi - lo) * n_bins) clamped to
    [0, n_bins), NaN counted nowhere -> int64 [n_bins, d]."""
    v = x.detach().cpu().double()
    keep = ~torch.isnan(v)
    b = ((v - lo) / ((hi - lo) or 1.0) * n_bins).floor().clamp(0, n_bins - 1)
    b = torch.where(keep, b, torch.zeros_like(b)).to(torch.int64)
    return _bincount_cols(b, keep, n_bins)


def histogram_fp32_formula(x, n_bins, lo, hi):
    """The kernel's own fp32 formula, floor((v - lo) * (n_bins / (hi - lo))),
    evaluated in fp32 on the CPU (IEEE sub, mul: no contraction possible)."""
    v = x.detach().cpu().float()
    keep = ~torch.isnan(v)
    lo32 = torch.tensor(lo, dtype=torch.float32)
    width = torch.tensor(hi, dtype=torch.float32) - lo32
    scale = torch.tensor(float(n_bins), dtype=torch.float32) / \
        (width if float(width) != 0.0 else torch.tensor(1.0))
    b = ((v - lo32) * scale).floor().clamp(0, n_bins - 1)
    b = torch.where(keep, b, torch.zeros_like(b)).to(torch.int64)
    return _bincount_cols(b, keep, n_bins)


def _bincount_cols(b, keep, n_bins):
    d = b.shape[1]
    flat = (b * d + torch.arange(d).unsqueeze(0))[keep]
    return torch.bincount(flat, minlength=n_bins * d).reshape(n_bins, d)


# --------------------------------------------------------------------------
# bitset
# --------------------------------------------------------------------------

def bitset_indices(n, seed=9):
    """Indices that hit bit 31 of a word (the int32 sign bit), bit n-1 (the
    tail word when n % 32 != 0), bit 0, and duplicates."""
    fixed = [0, n - 1, n - 1, 31 if n > 31 else n - 1, 0]
    fixed += [w * 32 + 31 for w in range(1, 4) if w * 32 + 31 < n]
    rnd = torch.randint(0, n, (min(n, 5000),), generator=_gen(seed))
    idx = torch.cat([torch.tensor(fixed, dtype=torch.int64), rnd, rnd[:50]])
    return idx


def bitset_oracle(n, set_idx, clear_idx=None):
    """Dense bool [n] after set(set_idx) then clear(clear_idx)."""
    dense = torch.zeros(n, dtype=torch.bool)
    dense[set_idx] = True
    if clear_idx is not None:
        dense[clear_idx] = False
    return dense


# --------------------------------------------------------------------------
# CSR SpMV / SDDMM
# --------------------------------------------------------------------------

def _csr_from_lengths(lengths, n_cols, seed, dtype, integer=True):
    g = _gen(seed)
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    indptr = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    indptr[1:] = lengths.cumsum(0)
    nnz = int(indptr[-1])
    indices = torch.randint(0, n_cols, (nnz,), generator=g)   # repeats allowed
    if integer:
        vals = torch.randint(-INT_LIM, INT_LIM + 1, (nnz,), generator=g).to(dtype)
        x = torch.randint(-INT_LIM, INT_LIM + 1, (n_cols,), generator=g).to(dtype)
    else:   # fp32-representable in either dtype: products are exact in fp64
        vals = torch.randn(nnz, generator=g, dtype=torch.float32).to(dtype)
        x = torch.randn(n_cols, generator=g, dtype=torch.float32).to(dtype)
    return dict(indptr=indptr.to(torch.int32), indices=indices.to(torch.int32),
                values=vals, x=x, n_rows=lengths.numel(), n_cols=n_cols)


@functools.lru_cache(maxsize=None)
def spmv_case(name, dtype=torch.float32):
    """Named CSR cases -> dict(indptr, indices, values, x, n_rows, n_cols)."""
    if name.startswith("uniform_"):
        L = int(name.split("_")[1])
        return _csr_from_lengths([L] * SPMV_ROWS, SPMV_COLS, 100 + L, dtype)
    if name == "power_law":
        # 2500 rows: one of 5000, the rest 0 (60 %), 1 or 2 -> mean
        # ceil(nnz / 2500) = 3 -> width 2, with empty rows and one very long row
        g = _gen(11)
        lengths = torch.randint(0, 5, (2500,), generator=g)
        lengths = torch.where(lengths >= 3, torch.zeros_like(lengths), lengths)
        lengths[1234] = 5000
        return _csr_from_lengths(lengths, 3001, 12, dtype)
    if name == "nnz0":
        return _csr_from_lengths([0] * 5, 7, 13, dtype)
    if name == "one_row":
        return _csr_from_lengths([77], 50, 14, dtype)
    if name == "repeated_cols":
        c = _csr_from_lengths([40] * 9, 3, 15, dtype)   # 40 entries over 3 columns
        return c
    if name == "random":
        return _csr_from_lengths([1, 0, 300, 17, 64, 5, 129] * 5, SPMV_COLS, 16,
                                 dtype, integer=False)
    raise KeyError(name)


SPMV_EXACT = tuple(f"uniform_{L}" for L in SPMV_L) + \
    ("power_law", "nnz0", "one_row", "repeated_cols")


def _csr_rows(c):
    lens = (c["indptr"][1:] - c["indptr"][:-1]).to(torch.int64)
    return torch.repeat_interleave(torch.arange(c["n_rows"]), lens), lens


def spmv_oracle(c):
    """fp64 y (products exact, each row summed with math.fsum: correctly
    rounded), fp64 sum |a_ij x_j| per row, row lengths."""
    rows, lens = _csr_rows(c)
    prod = c["values"].double() * c["x"].double()[c["indices"].to(torch.int64)]
    ptr = c["indptr"].tolist()
    pl = prod.tolist()
    y = torch.tensor([math.fsum(pl[ptr[r]:ptr[r + 1]]) for r in range(c["n_rows"])],
                     dtype=torch.float64)
    mass = torch.zeros(c["n_rows"], dtype=torch.float64).index_add_(0, rows, prod.abs())
    return y, mass, lens


def gamma(k, u):
    """Higham's gamma_k = k u / (1 - k u): k roundings in sequence."""
    k = torch.as_tensor(k, dtype=torch.float64)
    return k * u / (1 - k * u)


@functools.lru_cache(maxsize=None)
def sddmm_case(d, nnz, seed=17):
    """a [23, d], b [19, d] integer-valued; nnz edges with repeats (two equal
    edges whenever nnz >= 2)."""
    g = _gen(seed + d)
    a = torch.randint(-INT_LIM, INT_LIM + 1, (23, d), generator=g).float()
    b = torch.randint(-INT_LIM, INT_LIM + 1, (19, d), generator=g).float()
    rows = torch.randint(0, 23, (nnz,), generator=g).to(torch.int32)
    cols = torch.randint(0, 19, (nnz,), generator=g).to(torch.int32)
    if nnz >= 2:
        rows[-1], cols[-1] = rows[0], cols[0]
    return a, b, rows, cols


def sddmm_oracle(a, b, rows, cols):
    return (a.double()[rows.to(torch.int64)] * b.double()[cols.to(torch.int64)]).sum(dim=1)


# --------------------------------------------------------------------------
# linewise
# --------------------------------------------------------------------------

_LW_FN = {"add": torch.add, "sub": torch.sub, "mul": torch.mul, "div": torch.div}


@functools.lru_cache(maxsize=None)
def linewise_case(n, d, along_rows, seed=18):
    """x [n, d] and two vectors, fp32 randn; v2 has exact zeros (division by
    zero must give torch's inf / NaN) and x has zeros above them (0 / 0)."""
    g = _gen(seed + n + d)
    x = torch.randn(n, d, generator=g)
    m = d if along_rows else n
    v1 = torch.randn(m, generator=g)
    v2 = torch.randn(m, generator=g)
    v2[::7] = 0.0
    if along_rows:
        x[0, 0] = 0.0
    else:
        x[0, :] = 0.0
    return x, v1, v2


def linewise_oracle(x, v, op, along_rows):
    """The fp32 CPU result of one broadcast op (IEEE, correctly rounded)."""
    return _LW_FN[op](x, v.unsqueeze(0 if along_rows else 1))
