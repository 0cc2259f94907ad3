"""CPU half of the primitive-kernel tests (tests/primitive_inputs.py).

Three jobs, none of which needs a GPU:
  * every checker the GPU tests rely on REJECTS a planted wrong answer (an
    off-by-one index on a tie, one dropped tile, a dropped NaN, one count
    moved to the neighbouring bin, ...);
  * the project's own CPU paths, which the GPU paths must agree with, pass
    the same cases against the same oracles;
  * the conditions the exactness claims rest on hold for every case: integer
    inputs with partial sums below 2^24, an exactly representable histogram
    grid, and shapes that really reach the launcher route they are named for.
"""
import pytest
import torch

import primitive_inputs as P

F32, F64 = torch.float32, torch.float64


# --------------------------------------------------------------------------
# the shapes reach the routes they are named for
# --------------------------------------------------------------------------

def test_rows_shapes_reach_every_route():
    lws = {P.rows_route(3, d)["lw"] for d in P.ROWS_D}
    assert lws == {2, 8, 32, 64, None}              # every LW and the block kernel
    assert P.rows_route(3, 256)["kernel"] == "thin"
    assert P.rows_route(3, 257)["kernel"] == "block"
    tails = {d % 4 for d in P.ROWS_D if d > 256}
    assert tails == {0, 1, 3}                       # float4 tails 0, 1, 3
    assert 1027 > 4 * 256 and 1031 // 4 > 256       # second trip: scalar / float4 loop
    want = {(262150, 3): ("thin", 2), (8200, 65): ("thin", 64),
            (2050, 257): ("block", None)}
    for (n, d), (kern, lw) in want.items():
        r = P.rows_route(n, d)
        assert (r["kernel"], r["lw"]) == (kern, lw)
        assert r["grid"] == 2048 and r["passes"] == 2, (n, d, r)
    for n in P.ROWS_N:
        for d in P.ROWS_D:
            assert P.rows_route(n, d)["passes"] == 1


def test_cols_shapes_reach_every_route():
    r = P.cols_route(1000, 33)
    assert (r["kernel"], r["gx"], r["gy"]) == ("general", 1, 1)
    r = P.cols_route(1025, 33)
    assert (r["kernel"], r["gy"], r["rows_per_tile"]) == ("general", 2, 513)
    assert 1025 - 513 == 512                         # second tile one row short
    r = P.cols_route(2051, 300)
    assert (r["kernel"], r["gx"], r["gy"]) == ("general", 2, 3)
    assert {r["rows_per_tile"] % 4, (2051 - 2 * r["rows_per_tile"]) % 4} == {0, 3}
    assert P.cols_route(4095, 8)["kernel"] == "general"
    assert P.cols_route(4095, 8)["gy"] == 4
    for n, d in P.COLS_SKINNY:
        r = P.cols_route(n, d)
        assert r["kernel"] == "skinny" and r["gy"] == (1 if n == 4096 else
                                                       2 if n == 4097 else 3)
    assert {P.cols_route(4096, d)["rpt"] for _, d in P.COLS_SKINNY} == \
        {64, 32, 16, 4, 2}


def test_other_shapes_reach_their_routes():
    assert P.capped_passes(P.ARGMIN_ROWS, 2048) == 2      # argmin, normalize
    assert P.capped_passes(65537, 65536) == 2             # rows_sqnorm_bf16
    assert 2063 // 8 > 256 and 2055 % 8 == 7              # 2nd bf16x8 trip, tail
    assert {n for n, _ in P.SQNORM_SHAPES} == set(P.SQNORM_N)
    assert {d for _, d in P.SQNORM_SHAPES} == set(P.SQNORM_D)
    want = {1: "lds_multi", 256: "lds_multi", 4096: "lds_multi",
            4097: "lds_single", 16384: "lds_single", 16385: "gmem"}
    assert {b: P.histogram_strategy(b) for b in P.HIST_BINS} == want
    widths = {L: P.spmv_width(P.SPMV_ROWS, P.SPMV_ROWS * L) for L in P.SPMV_L}
    assert widths == {1: 2, 4: 2, 5: 4, 8: 4, 9: 8, 16: 8, 17: 16, 32: 16,
                      33: 32, 128: 32, 129: 64, 300: 64}
    c = P.spmv_case("power_law")
    nnz = c["values"].numel()
    lens = c["indptr"][1:] - c["indptr"][:-1]
    assert -(-nnz // c["n_rows"]) == 3 and P.spmv_width(c["n_rows"], nnz) == 2
    assert int(lens.max()) == 5000 and int((lens == 0).sum()) > 100
    assert {P.sddmm_width(d) for d in P.SDDMM_D} == {4, 16, 32, 64}
    assert P.linewise_blocks(4100, 1028) > 4096 and 1028 % 4 == 0
    assert P.linewise_blocks(333, 129) <= 4096 and 129 % 4 != 0
    assert P.BITSET_COUNT_BITS // 32 > 2048 * 256


# --------------------------------------------------------------------------
# exactness conditions
# --------------------------------------------------------------------------

def _reduce_shapes():
    rows = [(n, d, 1) for n in P.ROWS_N for d in P.ROWS_D]
    rows += [(n, d, 1) for n, d in P.ROWS_SECOND_PASS]
    cols = [(n, d, 0) for n, d in P.COLS_GENERAL + P.COLS_SKINNY]
    return rows + cols


@pytest.mark.parametrize("n,d,dim", _reduce_shapes())
def test_reduce_families_are_exact_in_fp32(n, d, dim):
    for x in (P.int_matrix(n, d), P.spike_matrix(n, d, dim),
              P.signed_matrix(n, d, 1), P.signed_matrix(n, d, -1)):
        for op in P.SUM_OPS:
            assert P.exact_ok(x, op, dim), (n, d, op)


def test_other_sum_families_are_exact():
    for n, d in P.SQNORM_SHAPES:
        x = P.int_matrix(n, d, 20)
        assert torch.equal(x.bfloat16().float(), x)          # exact in bf16
        assert P.exact_ok(x, 1, 1)
    for name in P.SPMV_EXACT:
        c = P.spmv_case(name)
        _, mass, _ = P.spmv_oracle(c)
        assert mass.numel() == 0 or float(mass.max()) < 2.0 ** 24, name
        assert bool((c["values"] == c["values"].round()).all())
    for d in P.SDDMM_D:
        a, b, rows, cols = P.sddmm_case(d, 1000)
        mass = (a.double()[rows.long()] * b.double()[cols.long()]).abs().sum(1)
        assert float(mass.max()) < 2.0 ** 24


@pytest.mark.parametrize("n_bins", P.HIST_BINS)
def test_dyadic_grid_bins_exactly_in_fp32(n_bins):
    """(v - lo) * scale is computed without rounding in fp32 for every v of
    the dyadic grid, so the kernel's fp32 formula IS the exact formula."""
    v = (torch.arange(-256, 256).double() / 64)
    scale32 = torch.tensor(float(n_bins)) / torch.tensor(P.HIST_HI - P.HIST_LO)
    assert float(scale32) == n_bins / 8
    t32 = (v.float() - torch.tensor(P.HIST_LO)) * scale32
    t64 = (v - P.HIST_LO) / (P.HIST_HI - P.HIST_LO) * n_bins
    assert torch.equal(t32.double(), t64)
    x = P.dyadic_matrix(4097, 3)
    assert torch.equal(P.histogram_fp32_formula(x, n_bins, P.HIST_LO, P.HIST_HI),
                       P.histogram_oracle(x, n_bins, P.HIST_LO, P.HIST_HI))


def test_error_bound_constants():
    """C per route, as derived next to rows_adds / cols_adds."""
    assert P.rows_adds(3, 4) == 2 + 1 and P.rows_adds(3, 16) == 2 + 3
    assert P.rows_adds(3, 64) == 2 + 5 and P.rows_adds(3, 256) == 2 + 6
    assert P.rows_adds(3, 257) == 2 + 6 + 4
    assert P.cols_adds(1000, 33) == 2 + 3 and P.cols_adds(2051, 300) == 2 + 3 + 3
    assert P.cols_adds(8195, 17) == 2 + 1 + 4 * 3     # rpt = 2, gy = 3
    assert P.cols_adds(4096, 1) == 2 + 6 + 4          # rpt = 64, gy = 1


# --------------------------------------------------------------------------
# checkers reject planted wrong answers
# --------------------------------------------------------------------------

def _rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_reduce_checker_rejects_dropped_tile_and_dropped_nan():
    n, d = 2051, 300
    x = P.int_matrix(n, d)
    t = P.cols_route(n, d)["rows_per_tile"]
    for op in P.SUM_OPS:
        ref = P.reduce_oracle(x, op, 0)
        P.check_equal(ref.float(), ref)
        dropped = P.reduce_oracle(torch.cat([x[:t], x[2 * t:]]), op, 0)
        _rejects(P.check_equal, dropped.float(), ref)
    # one element of the float4 tail missing
    x = P.spike_matrix(3, 1027, 1)
    for op in P.OPS:
        ref = P.reduce_oracle(x, op, 1)
        wrong = P.reduce_oracle(x[:, :-1], op, 1)
        if not torch.equal(wrong, ref):
            _rejects(P.check_equal, wrong.float(), ref)
    # spikes: dropping any boundary position changes min, max or max|x|
    pos = P.row_marks(3, 1027)
    for r in range(3):
        keep = [c for c in range(1027) if c not in (pos[r % len(pos)],
                                                    pos[(r + 1) % len(pos)])]
        for op in (3, 4, 5):
            assert not torch.equal(P.reduce_oracle(x[r:r + 1, keep], op, 1),
                                   P.reduce_oracle(x[r:r + 1], op, 1))
    # NaN dropped: the position-dependent max the old kernel computed
    xn = P.nan_positions_matrix(33, 257, 1)
    for op in (3, 4, 5):
        ref = P.reduce_oracle(xn, op, 1)
        assert bool(torch.isnan(ref[1:]).all()) and not bool(torch.isnan(ref[0]))
        dropped = P.reduce_oracle(torch.nan_to_num(xn, nan=0.0), op, 1)
        _rejects(P.check_equal, dropped.float(), ref)
    # wrong identity (0 instead of -inf) on an all-negative matrix
    xs = P.signed_matrix(33, 17, -1)
    ref = P.reduce_oracle(xs, 3, 1)
    _rejects(P.check_equal, torch.maximum(ref, torch.zeros(())).float(), ref)


def test_nonfinite_oracle_and_checker():
    for dtype in (F32, F64):
        x = P.nonfinite_sum_rows(17, dtype)
        inf = float("inf")
        ref = P.nonfinite_oracle(x, 0, 1)
        assert ref[0] == inf and ref[1] == -inf and ref[4] == inf and ref[5] == -inf
        assert bool(torch.isnan(ref[2])) and bool(torch.isnan(ref[3]))
        # what KahanAcc used to return: NaN for every non-finite row
        _rejects(P.check_equal, torch.full((6,), float("nan"), dtype=dtype), ref)
        for op in (1, 2):
            r = P.nonfinite_oracle(x, op, 1)
            assert r[0] == inf and r[1] == inf and r[2] == inf and r[4] == inf
            assert bool(torch.isnan(r[3]))


def test_bound_checker_rejects_plain_summation_error():
    x = P.cancel_matrix(3, 1027, 1, F32)
    ref = P.exact_sum_oracle(x, 0, 1)
    bound = P.rows_adds(3, 1027) * P.U[F32] * P.abs_mass(x, 0, 1)
    P.check_bound(ref.float(), ref, bound + 1.0)     # fp32 rounding of ref only
    _rejects(P.check_bound, (ref + 2 * bound + 1e-3).float(), ref, bound)
    # the cancellation family's bound scales with the large pairs, which a
    # plain sum survives; the drift family is the one an UNcompensated
    # per-thread sum misses: simulate the block kernel's 256 strided threads
    # with plain fp32 accumulators (and a perfect combine)
    x = P.drift_matrix()
    n, d = x.shape
    ref = P.exact_sum_oracle(x, 0, 1)
    bound = P.rows_adds(n, d) * P.U[F32] * P.abs_mass(x, 0, 1)
    acc = torch.zeros(n, 256)
    for step in x.view(n, d // 256, 256).unbind(1):
        acc = acc + step
    _rejects(P.check_bound, acc.double().sum(1), ref, bound)
    P.check_bound(ref.float(), ref, bound)


@pytest.mark.parametrize("d", P.ARGMIN_D)
def test_argmin_oracle_and_checker(d):
    x = P.argmin_matrix(d)
    ref = P.argmin_oracle(x)
    assert torch.equal(ref, x.argmin(dim=1))             # torch CPU agrees
    P.check_equal(ref.int(), ref)
    if d > 1:
        # off by one on a tie: pick the LAST minimum instead of the first
        last = (d - 1) - torch.flip(x, dims=[1]).argmin(dim=1)
        assert int((last != ref).sum()) >= 4
        _rejects(P.check_equal, last.int(), ref)
    xn = P.argmin_nan_matrix(d)
    refn = P.argmin_oracle(xn)
    assert torch.equal(refn, xn.argmin(dim=1))           # first NaN, as torch
    if d > 1:
        ignored = torch.nan_to_num(xn, nan=float("inf")).argmin(dim=1)
        _rejects(P.check_equal, ignored.int(), refn)
    # argmax through the same oracle
    assert torch.equal(P.argmin_oracle(-x), x.argmax(dim=1))
    assert torch.equal(P.argmin_oracle(-xn), xn.argmax(dim=1))


def test_histogram_checker_rejects_moved_count_and_binned_nan():
    x = P.dyadic_matrix(4097, 3)
    ref = P.histogram_oracle(x, 256, P.HIST_LO, P.HIST_HI)
    assert int(ref.sum()) == x.numel()
    wrong = ref.clone()
    b = int(ref[:, 1].nonzero()[0])
    wrong[b, 1] -= 1
    wrong[b + 1, 1] += 1
    _rejects(P.check_equal, wrong, ref)
    e = P.hist_edge_matrix(3)
    ref = P.histogram_oracle(e, 16, P.HIST_LO, P.HIST_HI)
    n_nan = int(torch.isnan(e).sum())
    assert n_nan == 6 and int(ref.sum()) == e.numel() - n_nan
    binned = ref.clone()
    binned[0] += 2                                        # NaN put into bin 0
    _rejects(P.check_equal, binned, ref)
    # lo and below -> bin 0; hi, above and +inf -> last bin
    one = P.histogram_oracle(torch.tensor([[-4.0], [-9.0], [-float("inf")]]), 16, -4., 4.)
    assert int(one[0, 0]) == 3
    one = P.histogram_oracle(torch.tensor([[4.0], [9.0], [float("inf")]]), 16, -4., 4.)
    assert int(one[15, 0]) == 3


def test_spmv_sddmm_linewise_checkers_reject():
    c = P.spmv_case("uniform_33")
    y, _, _ = P.spmv_oracle(c)
    P.check_equal(y.float(), y)
    # drop the last entry of every row (a sub-wave tail bug)
    short = dict(c)
    keep = torch.ones(c["values"].numel(), dtype=torch.bool)
    keep[c["indptr"][1:].long() - 1] = False
    short.update(values=c["values"] * keep)
    _rejects(P.check_equal, P.spmv_oracle(short)[0].float(), y)
    a, b, rows, cols = P.sddmm_case(33, 1000)
    ref = P.sddmm_oracle(a, b, rows, cols)
    assert ref[0] == ref[-1]                               # the repeated edge
    _rejects(P.check_equal, P.sddmm_oracle(a[:, :32], b[:, :32], rows, cols).float(), ref)
    x, v1, v2 = P.linewise_case(3, 5, True)
    ref = P.linewise_oracle(x, v2, "div", True)
    assert bool(torch.isinf(ref).any()) and bool(torch.isnan(ref).any())
    one_ulp = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    _rejects(P.check_equal, one_ulp, ref.double())


def test_bitset_oracle_covers_sign_bit_and_tail():
    for n in P.BITSET_N:
        idx = P.bitset_indices(n)
        assert int(idx.min()) == 0 and int(idx.max()) == n - 1
        assert idx.numel() > idx.unique().numel()          # duplicates
        if n > 31:
            assert bool((idx % 32 == 31).any())            # bit 31 of a word
        dense = P.bitset_oracle(n, idx, idx[::2])
        assert not bool(dense[idx[::2]].any())


# --------------------------------------------------------------------------
# the project's CPU paths against the same oracles
# --------------------------------------------------------------------------

_NAMES = {0: ("identity", "sum"), 1: ("sq", "sum"), 2: ("abs", "sum"),
          3: ("identity", "max"), 4: ("identity", "min"), 5: ("abs", "max")}


def _cpu_reduce(x, op, dim):
    from raft_amd.linalg.reduce import coalesced_reduction, strided_reduction
    main_op, red = _NAMES[op]
    fn = coalesced_reduction if dim == 1 else strided_reduction
    return fn(x, main_op=main_op, reduce_op=red)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,d,dim", [(33, 1027, 1), (3, 5, 1), (2051, 300, 0),
                                     (4097, 17, 0)])
def test_cpu_reduce_paths(n, d, dim, dtype):
    fams = [P.int_matrix(n, d), P.spike_matrix(n, d, dim),
            P.signed_matrix(n, d, -1), P.nan_positions_matrix(n, d, dim)]
    for x in fams:
        for op in P.OPS:
            out = _cpu_reduce(x.to(dtype), op, dim)
            assert out.dtype == dtype
            P.check_equal(out, P.reduce_oracle(x, op, dim), f"op {op}")


def test_cpu_reduce_nonfinite_and_empty():
    for dtype in (F32, F64):
        x = P.nonfinite_sum_rows(17, dtype)
        for op in P.SUM_OPS:
            P.check_equal(_cpu_reduce(x, op, 1), P.nonfinite_oracle(x, op, 1))
            P.check_equal(_cpu_reduce(x.t().contiguous(), op, 0),
                          P.nonfinite_oracle(x, op, 1))
    for op in P.SUM_OPS:
        assert torch.equal(_cpu_reduce(torch.zeros(5, 0), op, 1), torch.zeros(5))
        assert torch.equal(_cpu_reduce(torch.zeros(0, 5), op, 0), torch.zeros(5))
        assert _cpu_reduce(torch.zeros(0, 5), op, 1).shape == (0,)
        assert _cpu_reduce(torch.zeros(5, 0), op, 0).shape == (0,)
    for op in (3, 4, 5):
        with pytest.raises((RuntimeError, IndexError)):
            _cpu_reduce(torch.zeros(5, 0), op, 1)
        with pytest.raises((RuntimeError, IndexError)):
            _cpu_reduce(torch.zeros(0, 5), op, 0)
        assert _cpu_reduce(torch.zeros(0, 5), op, 1).shape == (0,)


def test_cpu_argmin_argmax_normalize_paths():
    from raft_amd.matrix.argminmax import argmin, argmax
    from raft_amd.linalg.norm import normalize
    for d in (1, 257):
        for x in (P.argmin_matrix(d), P.argmin_nan_matrix(d)):
            P.check_equal(argmin(x), P.argmin_oracle(x))
            P.check_equal(argmax(x), P.argmin_oracle(-x))
    with pytest.raises((RuntimeError, IndexError)):
        argmin(torch.zeros(3, 0))
    assert argmin(torch.zeros(0, 3)).shape == (0,)
    x = P.int_matrix(5, 257).clone()
    x[2] = 0.0
    out = normalize(x)
    assert torch.equal(out[2], torch.zeros(257))           # eps branch: 0 / eps
    ref = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    assert float((out.double() - ref).abs().max()) <= 4 * P.U[F32]
    assert normalize(torch.zeros(0, 4)).shape == (0, 4)


def test_cpu_histogram_path():
    from raft_amd.stats import histogram
    for n_bins in (1, 256, 4097):
        x = P.dyadic_matrix(4097, 3)
        P.check_equal(histogram(x, n_bins, P.HIST_LO, P.HIST_HI),
                      P.histogram_oracle(x, n_bins, P.HIST_LO, P.HIST_HI))
    e = P.hist_edge_matrix(3)
    h = histogram(e, 16, P.HIST_LO, P.HIST_HI)
    P.check_equal(h, P.histogram_oracle(e, 16, P.HIST_LO, P.HIST_HI))
    assert int(h.sum()) == int((~torch.isnan(e)).sum())    # NaN in no bin
    assert histogram(torch.zeros(5, 0), 4, 0.0, 1.0).shape == (4, 0)
    assert int(histogram(torch.zeros(0, 2), 4, 0.0, 1.0).sum()) == 0


def test_cpu_bitset_path():
    from raft_amd.core import Bitset
    for n in P.BITSET_N:
        idx = P.bitset_indices(n)
        bs = Bitset(n, device="cpu", default=False)
        bs.set(idx, True)
        dense = P.bitset_oracle(n, idx)
        assert torch.equal(bs.to_dense(), dense) and bs.count() == int(dense.sum())
        assert bool(bs.test(idx).all())
        bs.set(idx[::2], False)
        dense = P.bitset_oracle(n, idx, idx[::2])
        assert torch.equal(bs.to_dense(), dense) and bs.count() == int(dense.sum())
        assert torch.equal(bs.test(idx), dense[idx])
        full = Bitset(n, device="cpu", default=True)
        assert full.count() == n                            # tail word masked


def test_cpu_sparse_and_linewise_paths():
    from raft_amd.sparse.types import CSR
    from raft_amd.sparse.linalg import spmv, sddmm
    from raft_amd.linalg.matrix_vector import matrix_vector_op, linewise_fused
    for name in ("uniform_5", "uniform_129", "power_law", "nnz0", "one_row",
                 "repeated_cols"):
        for dtype in (F32, F64):
            c = P.spmv_case(name, dtype)
            a = CSR(c["indptr"], c["indices"], c["values"], c["n_rows"], c["n_cols"])
            P.check_equal(spmv(a, c["x"]), P.spmv_oracle(c)[0], name)
    for d in (1, 33):
        a, b, rows, cols = P.sddmm_case(d, 1000)
        order = torch.argsort(rows.long() * 19 + cols.long(), stable=True)
        rows, cols = rows[order], cols[order]
        indptr = torch.zeros(24, dtype=torch.int32)
        indptr[1:] = torch.bincount(rows.long(), minlength=23).cumsum(0).int()
        mask = CSR(indptr, cols, torch.ones(1000), 23, 19)
        P.check_equal(sddmm(a, b, mask).values, P.sddmm_oracle(a, b, rows, cols))
    for along in (True, False):
        x, v1, v2 = P.linewise_case(3, 5, along)
        for op in P.LW_OPS:
            P.check_equal(matrix_vector_op(x, v2, op, along),
                          P.linewise_oracle(x, v2, op, along).double())
            two = P.linewise_oracle(P.linewise_oracle(x, v1, "sub", along), v2, op, along)
            P.check_equal(linewise_fused(x, v1, "sub", v2, op, along), two.double())
