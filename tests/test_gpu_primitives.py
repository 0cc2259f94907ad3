"""GPU half of the primitive-kernel tests: every launcher route of the
reduction, argmin, normalize, bf16-norm, linewise, histogram, bitset, SpMV and
SDDMM kernels against the fp64 oracles of tests/primitive_inputs.py.

On the integer-valued families the kernels must EQUAL the oracle (every
partial sum is exact in fp32, see tests/test_primitive_oracle.py); one random
family per sum kernel checks the compensation against a bound counted from
the code. Behaviour (NaN, +/-inf, empty shapes, argument guards) is pinned to
the CPU path of the same public function. All tests REQUIRE the native
extension: there is no fallback.
"""
import pytest
import torch

import primitive_inputs as P

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
ERR = (RuntimeError, IndexError, AssertionError, ValueError)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


def _alive(dev):
    """No launch error is pending and the device still answers."""
    torch.cuda.synchronize()
    assert int(torch.ones(3, device=dev).sum().item()) == 3


_NAMES = {0: ("identity", "sum"), 1: ("sq", "sum"), 2: ("abs", "sum"),
          3: ("identity", "max"), 4: ("identity", "min"), 5: ("abs", "max")}


def _public_reduce(x, op, dim):
    from raft_amd.linalg.reduce import coalesced_reduction, strided_reduction
    main_op, red = _NAMES[op]
    fn = coalesced_reduction if dim == 1 else strided_reduction
    return fn(x, main_op=main_op, reduce_op=red)


def _reduce(ext, x, op, dim):
    return ext.reduce_rows(x, op) if dim == 1 else ext.reduce_cols(x, op)


def _exact_families(n, d, dim):
    return (("int", P.int_matrix(n, d)), ("spike", P.spike_matrix(n, d, dim)),
            ("pos", P.signed_matrix(n, d, 1)), ("neg", P.signed_matrix(n, d, -1)))


def _check_exact(ext, dev, n, d, dim, dtype, families=None):
    for fam, x in families or _exact_families(n, d, dim):
        xg = x.to(dev, dtype).contiguous()
        for op in P.OPS:
            out = _reduce(ext, xg, op, dim)
            assert out.dtype == dtype
            P.check_equal(out, P.reduce_oracle(x, op, dim),
                          f"{fam} ({n}, {d}) op {op} {dtype}")


def _check_compensated(ext, dev, n, d, dim, dtype, adds):
    """|out - ref| <= C u sum|main_op(x_i)| with C = adds (+ 1 for op 1), ref
    the correctly rounded exact sum, everything in fp64."""
    x = P.cancel_matrix(n, d, dim, dtype)
    xg = x.to(dev).contiguous()
    for op in P.SUM_OPS:
        c = adds + (P.PRODUCT_ROUNDING if op == 1 else 0)
        bound = c * P.U[dtype] * P.abs_mass(x, op, dim)
        worst = P.check_bound(_reduce(ext, xg, op, dim), P.exact_sum_oracle(x, op, dim),
                              bound, f"cancel ({n}, {d}) op {op} {dtype} C={c}")
        print(f"cancel ({n},{d}) dim {dim} op {op} {dtype}: C={c} "
              f"worst err/bound {worst:.3e}")


class TestReduceRows:
    @DTYPES
    @pytest.mark.parametrize("d", P.ROWS_D)
    def test_exact(self, dev, ext, d, dtype):
        """launch_reduce_rows: d <= 4 -> thin LW=2, <= 16 -> LW=8, <= 64 ->
        LW=32, <= 256 -> LW=64, else the 256-thread block kernel (float4
        loads in fp32: tails d % 4 = 0, 1, 3; 1031 // 4 = 257 > 256 float4
        gives thread 0 a second trip). Ops 0..5, fp32 and fp64, rows 1/3/33."""
        for n in P.ROWS_N:
            _check_exact(ext, dev, n, d, 1, dtype)

    @DTYPES
    @pytest.mark.parametrize("n,d", P.ROWS_SECOND_PASS)
    def test_second_grid_stride_pass(self, dev, ext, n, d, dtype):
        """Grid cap 2048 blocks (grid_1d / min(n, 2048)): 262150 x 3 -> LW=2,
        128 rows per block, 2048 * 128 = 262144 < 262150; 8200 x 65 -> LW=64,
        4 rows per block, 8192 < 8200; 2050 x 257 -> block kernel, 2048 <
        2050. The last rows are computed in the second pass."""
        r = P.rows_route(n, d)
        assert r["grid"] == 2048 and r["passes"] == 2
        _check_exact(ext, dev, n, d, 1, dtype,
                     (("int", P.int_matrix(n, d)), ("spike", P.spike_matrix(n, d, 1))))

    @DTYPES
    @pytest.mark.parametrize("d", (3, 16, 64, 65, 257, 1031))
    def test_compensation_bound(self, dev, ext, d, dtype):
        """C = 2 (the per-lane Neumaier accumulator, see primitive_inputs
        KAHAN) + log2(LW) shuffle adds for the thin kernel (LW = 2, 8, 32, 64
        -> C = 3, 5, 7, 8); block kernel: 2 + 6 shuffle steps + 4 wave
        partials summed through LDS = 12."""
        _check_compensated(ext, dev, 33, d, 1, dtype, P.rows_adds(33, d))

    @DTYPES
    @pytest.mark.parametrize("d", (5, 65, 257, 1027))
    def test_nan_any_position(self, dev, ext, d, dtype):
        """A NaN first, last, mid-lane or in any tile makes every op NaN."""
        x = P.nan_positions_matrix(33, d, 1)
        _check_exact(ext, dev, 33, d, 1, dtype, (("nan", x),))
        for op in (3, 4, 5):
            out = _public_reduce(x.to(dev, dtype), op, 1)
            P.check_equal(out, _public_reduce(x.to(dtype), op, 1).double(), "public")
            assert bool(torch.isnan(out[1:]).all()) and not bool(torch.isnan(out[0]))

    @DTYPES
    @pytest.mark.parametrize("d", (4, 5, 65, 257, 1027))
    def test_nonfinite_sums(self, dev, ext, d, dtype):
        """+inf (or overflow) -> +inf, -inf -> -inf, both or NaN -> NaN: what
        the CPU path of coalesced_reduction / row_norm returns."""
        from raft_amd.linalg import row_norm
        x = P.nonfinite_sum_rows(d, dtype)
        for op in P.SUM_OPS:
            out = _public_reduce(x.to(dev), op, 1)
            P.check_equal(out, P.nonfinite_oracle(x, op, 1), f"d {d} op {op}")
            P.check_equal(out, _public_reduce(x, op, 1).double(), "vs CPU path")
        P.check_equal(row_norm(x.to(dev)), row_norm(x).double(), "row_norm")

    def test_kahan_long_row_still_compensated(self, dev, ext):
        """2^17 terms: the non-finite guard must not cost the compensation."""
        x = torch.randn(2, 1 << 17, generator=torch.Generator().manual_seed(1))
        out = ext.reduce_rows(x.to(dev), 0)
        assert (1 << 17) // 256 <= 4096          # terms per thread, see KAHAN
        bound = P.rows_adds(2, 1 << 17) * P.U[F32] * P.abs_mass(x, 0, 1)
        P.check_bound(out, P.reduce_oracle(x, 0, 1), bound)

    def test_drift_needs_compensation(self, dev, ext):
        """Constant rows of 2^17 terms, 512 per thread of the block kernel: a
        plain per-thread fp32 sum misses this bound (shown on the CPU in
        test_primitive_oracle), the compensated one must meet it. C = 12."""
        x = P.drift_matrix()
        for op in P.SUM_OPS:
            c = P.rows_adds(*x.shape) + (P.PRODUCT_ROUNDING if op == 1 else 0)
            bound = c * P.U[F32] * P.abs_mass(x, op, 1)
            worst = P.check_bound(ext.reduce_rows(x.to(dev), op),
                                  P.exact_sum_oracle(x, op, 1), bound, f"drift op {op}")
            print(f"drift op {op}: C={c} worst err/bound {worst:.3e}")

    def test_empty(self, dev, ext):
        for dtype in (F32, F64):
            for op in P.OPS:
                assert ext.reduce_rows(torch.zeros(0, 5, device=dev, dtype=dtype), op).shape == (0,)
            for op in P.SUM_OPS:
                out = ext.reduce_rows(torch.zeros(5, 0, device=dev, dtype=dtype), op)
                assert torch.equal(out.cpu(), torch.zeros(5, dtype=dtype))
            for op in (3, 4, 5):
                with pytest.raises(ERR):
                    ext.reduce_rows(torch.zeros(5, 0, device=dev, dtype=dtype), op)
                with pytest.raises(ERR):
                    _public_reduce(torch.zeros(5, 0, device=dev, dtype=dtype), op, 1)
        _alive(dev)


class TestReduceCols:
    @DTYPES
    @pytest.mark.parametrize("n,d", P.COLS_GENERAL)
    def test_general_exact(self, dev, ext, n, d, dtype):
        """General kernel: gx = ceil(d / 256), gy = min(ceil(512 / gx),
        ceil(n / 1024)). (1000, 33): gy = 1, direct store. (1025, 33): gy = 2,
        tiles of 513 and 512 rows, atomic / CAS combine. (2051, 300): gx = 2,
        gy = 3, tiles 684, 684, 683 (r % 4 tails 0 and 3). (4095, 8): one row
        short of the skinny kernel, gy = 4."""
        assert P.cols_route(n, d)["kernel"] == "general"
        _check_exact(ext, dev, n, d, 0, dtype)

    @DTYPES
    @pytest.mark.parametrize("n,d", P.COLS_SKINNY)
    def test_skinny_exact(self, dev, ext, n, d, dtype):
        """Skinny kernel (d < 32 and n >= 4096): gy = ceil(n / 4096) = 1, 2,
        3 for n = 4096, 4097, 8195; 64 / pow2ceil(d) rows per wave step."""
        assert P.cols_route(n, d)["kernel"] == "skinny"
        _check_exact(ext, dev, n, d, 0, dtype)

    @DTYPES
    @pytest.mark.parametrize("n,d", ((1000, 33), (2051, 300), (4097, 3), (8195, 17)))
    def test_compensation_bound(self, dev, ext, n, d, dtype):
        """General: four Neumaier accumulators per thread; a1..a3 fold into a0
        with compensated adds but their three get() calls round -> C = 2 + 3,
        plus gy atomic partials when gy > 1 ((2051, 300): 5 + 3). Skinny: 2 +
        log2(rows per wave step) shuffle adds + 4 waves * gy atomics
        ((4097, 3): 2 + 4 + 8; (8195, 17): 2 + 1 + 12)."""
        _check_compensated(ext, dev, n, d, 0, dtype, P.cols_adds(n, d))

    @DTYPES
    @pytest.mark.parametrize("n,d", ((1000, 33), (2051, 300), (8195, 17)))
    def test_nan_any_position(self, dev, ext, n, d, dtype):
        x = P.nan_positions_matrix(n, d, 0)
        _check_exact(ext, dev, n, d, 0, dtype, (("nan", x),))
        for op in (3, 4, 5):
            P.check_equal(_public_reduce(x.to(dev, dtype), op, 0),
                          _public_reduce(x.to(dtype), op, 0).double(), "public")

    @DTYPES
    @pytest.mark.parametrize("n", (1000, 2051, 4097))
    def test_nonfinite_sums(self, dev, ext, n, dtype):
        """Columns of the non-finite family, padded with zero rows to reach
        the gy == 1, gy > 1 and skinny routes (6 columns)."""
        rows = P.nonfinite_sum_rows(17, dtype)
        x = torch.zeros(n, 6, dtype=dtype)
        at = torch.linspace(0, n - 1, 17).long()
        x[at] = rows.t()
        for op in P.SUM_OPS:
            out = _public_reduce(x.to(dev), op, 0)
            P.check_equal(out, P.nonfinite_oracle(x, op, 0), f"n {n} op {op}")
            P.check_equal(out, _public_reduce(x, op, 0).double(), "vs CPU path")

    def test_empty(self, dev, ext):
        for dtype in (F32, F64):
            for op in P.OPS:
                assert ext.reduce_cols(torch.zeros(5, 0, device=dev, dtype=dtype), op).shape == (0,)
            for op in P.SUM_OPS:
                out = ext.reduce_cols(torch.zeros(0, 5, device=dev, dtype=dtype), op)
                assert torch.equal(out.cpu(), torch.zeros(5, dtype=dtype))
            for op in (3, 4, 5):
                with pytest.raises(ERR):
                    ext.reduce_cols(torch.zeros(0, 5, device=dev, dtype=dtype), op)
        _alive(dev)


class TestArgmin:
    @pytest.mark.parametrize("d", P.ARGMIN_D)
    def test_ties_inf_and_second_pass(self, dev, ext, d):
        """row_argmin: one 256-thread block per row, grid min(n, 2048): 2050
        rows -> rows 2048, 2049 in the second pass. Ties at (j, j+1) meet in
        the wave shuffle, (j, j+64) across waves, (j, j+256) inside one
        thread; the lowest index must win, as torch.argmin."""
        from raft_amd.matrix.argminmax import argmin, argmax
        assert P.capped_passes(P.ARGMIN_ROWS, 2048) == 2
        x = P.argmin_matrix(d)
        ref = P.argmin_oracle(x)
        P.check_equal(ext.row_argmin(x.to(dev)), ref, f"row_argmin d {d}")
        P.check_equal(argmin(x.to(dev)), ref, "matrix.argmin")
        P.check_equal(argmax(x.to(dev)), P.argmin_oracle(-x), "matrix.argmax")
        P.check_equal(argmax((-x).to(dev)), ref, "matrix.argmax(-x)")

    @pytest.mark.parametrize("d", P.ARGMIN_D)
    def test_first_nan_wins(self, dev, ext, d):
        from raft_amd.matrix.argminmax import argmin, argmax
        x = P.argmin_nan_matrix(d)
        P.check_equal(argmin(x.to(dev)), argmin(x), "argmin vs CPU path")
        P.check_equal(argmin(x.to(dev)), P.argmin_oracle(x), "argmin")
        P.check_equal(argmax(x.to(dev)), argmax(x), "argmax vs CPU path")

    def test_empty(self, dev, ext):
        assert ext.row_argmin(torch.zeros(0, 3, device=dev)).shape == (0,)
        with pytest.raises(ERR):
            ext.row_argmin(torch.zeros(3, 0, device=dev))
        _alive(dev)


class TestNormalizeAndSqnorm:
    @pytest.mark.parametrize("d", (1, 257))
    def test_row_normalize_l2(self, dev, ext, d):
        """Grid min(n, 2048) on 2050 rows: second pass. The sum of squares
        carries C = 2 + 6 + 4 = 12 adds (Neumaier + shuffles + wave
        partials) plus 1 for the rounding of each square; all terms are
        non-negative, so its rel. error is 13u. sqrt halves it and rounds
        (u), the reciprocal rounds (u), the product rounds (u):
        |out - ref| <= (13 / 2 + 3) u |ref|, plus u |ref| for second-order
        terms. Zero rows take the eps branch and stay exactly zero."""
        n = 2050
        x = torch.randn(n, d, generator=torch.Generator().manual_seed(5))
        x[::5] = P.int_matrix(n, d, 21)[::5]
        x[7] = 0.0
        x[n - 1] = 0.0
        out = ext.row_normalize_l2(x.to(dev), 1e-12)
        xd = x.double()
        ref = xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12)
        c = (P.NORMALIZE_SUM_ADDS + P.PRODUCT_ROUNDING) / 2 + 3 + 1
        worst = P.check_bound(out, ref, c * P.U[F32] * ref.abs() + 1e-300, f"d {d}")
        print(f"row_normalize_l2 d {d}: C={c} worst err/bound {worst:.3e}")
        assert torch.equal(out[7].cpu(), torch.zeros(d))
        assert torch.equal(out[n - 1].cpu(), torch.zeros(d))

    @pytest.mark.parametrize("d", (5, 257))
    def test_row_normalize_inf_row(self, dev, ext, d):
        """A row holding +/-inf has norm inf: its finite entries become 0 and
        the infinite one NaN, as on the CPU path (the compensated sum used to
        turn the norm, and with it the whole row, into NaN)."""
        from raft_amd.linalg import normalize
        x = P.int_matrix(4, d, 22).clone()
        x[1, d // 2] = float("inf")
        x[2, d - 1] = -float("inf")
        out = normalize(x.to(dev))
        P.check_equal(out[1:3], normalize(x)[1:3].double(), f"d {d}")
        assert int(torch.isnan(out[1:3]).sum()) == 2
        assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all())

    def test_row_normalize_empty(self, dev, ext):
        assert ext.row_normalize_l2(torch.zeros(0, 4, device=dev), 1e-12).shape == (0, 4)
        assert ext.row_normalize_l2(torch.zeros(4, 0, device=dev), 1e-12).shape == (4, 0)
        _alive(dev)

    @pytest.mark.parametrize("n,d", P.SQNORM_SHAPES)
    def test_rows_sqnorm_bf16(self, dev, ext, n, d):
        """One block per row, grid min(n, 65536): 65537 rows -> the last row
        in the second pass. bf16x8 vector loop over d // 8 (2063 // 8 = 257:
        second trip) and a scalar tail of d % 8. Integers are exact in bf16
        and every partial sum in fp32."""
        x = P.int_matrix(n, d, 20)
        out = ext.rows_sqnorm_bf16(x.to(dev, torch.bfloat16))
        P.check_equal(out, P.reduce_oracle(x, 1, 1), f"({n}, {d})")

    def test_rows_sqnorm_bf16_empty(self, dev, ext):
        z = torch.zeros(0, 8, device=dev, dtype=torch.bfloat16)
        assert ext.rows_sqnorm_bf16(z).shape == (0,)
        _alive(dev)


def _bitwise(out, ref, what):
    """Same values (NaN == NaN) and the same sign on every zero. NaN payloads
    are not compared: they differ between host and device by design."""
    o = out.detach().cpu()
    P.check_equal(o, ref.double(), what)
    num = ~torch.isnan(ref)
    assert torch.equal(torch.signbit(o)[num], torch.signbit(ref)[num]), f"{what}: sign of zero"


class TestLinewise:
    @pytest.mark.parametrize("along_rows", [True, False], ids=["rows", "cols"])
    @pytest.mark.parametrize("n,d", P.LINEWISE_SHAPES)
    def test_single_ops_bitwise(self, dev, ext, n, d, along_rows):
        """float4 path when d % 4 == 0, scalar path otherwise; (4100, 1028)
        needs 4100 * 1028 / 4 / 256 = 4117 blocks > the 4096-block cap, so
        the float4 loop strides. The build uses no fast-math or approximate
        division flag, so all four ops, div included, must match the fp32
        CPU result bit for bit; the divisor holds zeros (inf and NaN)."""
        from raft_amd.linalg.matrix_vector import matrix_vector_op
        x, v1, v2 = P.linewise_case(n, d, along_rows)
        xg, vg = x.to(dev), v2.to(dev)
        for op in P.LW_OPS:
            ref = P.linewise_oracle(x, v2, op, along_rows)
            _bitwise(matrix_vector_op(xg, vg, op, along_rows), ref, f"{op} ({n}, {d})")

    @pytest.mark.parametrize("along_rows", [True, False], ids=["rows", "cols"])
    @pytest.mark.parametrize("n,d", ((3, 5), (33, 8)))
    def test_all_fused_pairs(self, dev, ext, n, d, along_rows):
        """All 16 (op1, op2) pairs equal the two-step fp32 CPU computation."""
        from raft_amd.linalg.matrix_vector import linewise_fused
        x, v1, v2 = P.linewise_case(n, d, along_rows)
        for op1 in P.LW_OPS:
            step = P.linewise_oracle(x, v1, op1, along_rows)
            for op2 in P.LW_OPS:
                ref = P.linewise_oracle(step, v2, op2, along_rows)
                out = linewise_fused(x.to(dev), v1.to(dev), op1, v2.to(dev), op2, along_rows)
                _bitwise(out, ref, f"{op1}-{op2} ({n}, {d})")

    def test_guards(self, dev, ext):
        """Host, wrong-dtype or wrong-length vectors raise from the binding."""
        x = torch.zeros(4, 8, device=dev)
        good = torch.ones(8, device=dev)
        for bad in (torch.ones(8), torch.ones(8, device=dev, dtype=F64),
                    torch.ones(7, device=dev)):
            with pytest.raises(RuntimeError):
                ext.linewise(x, bad, None, True, 0, 0)
            with pytest.raises(RuntimeError):
                ext.linewise(x, good, bad, True, 0, 0)
        with pytest.raises(RuntimeError):
            ext.linewise(x, good, None, True, 4, 0)
        from raft_amd.linalg.matrix_vector import matrix_vector_op
        with pytest.raises(ERR):
            matrix_vector_op(x, torch.ones(8), "add", True)
        _alive(dev)


class TestHistogram:
    @pytest.mark.parametrize("d", P.HIST_D)
    @pytest.mark.parametrize("n_bins", P.HIST_BINS)
    def test_dyadic_exact(self, dev, ext, n_bins, d):
        """Strategy by n_bins with NW = 4 waves: 4 * n_bins * 4 B <= 64 KiB
        -> LDS-MULTI (1, 256, 4096); n_bins * 4 B <= 64 KiB -> LDS-SINGLE
        (4097, 16384); else GMEM (16385). Row chunks: ceil(512 / d), reduced
        to ceil(n / 4096) when a chunk would be under 4096 rows (n = 4097 ->
        2 chunks, 20001 -> 5 for d <= 3; d = 513 -> 1). On the dyadic grid
        the fp32 bin formula is exact, so counts equal the fp64 oracle.
        (20001, 513) is left out: a 41 MB input and a 67 MB output."""
        for n in P.HIST_N:
            if n * d * 4 > 16 << 20:
                continue
            x = P.dyadic_matrix(n, d)
            out = ext.histogram_f32(x.to(dev), n_bins, P.HIST_LO, P.HIST_HI)
            ref = P.histogram_oracle(x, n_bins, P.HIST_LO, P.HIST_HI)
            P.check_equal(out, ref, f"{P.histogram_strategy(n_bins)} n {n} d {d}")
            assert int(out.sum()) == n * d

    @pytest.mark.parametrize("n_bins", P.HIST_BINS)
    def test_random_same_fp32_formula(self, dev, ext, n_bins):
        x = torch.rand(20001, 3, generator=torch.Generator().manual_seed(3)) * 10 - 5
        out = ext.histogram_f32(x.to(dev), n_bins, -5.0, 5.0)
        P.check_equal(out, P.histogram_fp32_formula(x, n_bins, -5.0, 5.0), str(n_bins))

    @pytest.mark.parametrize("n_bins", P.HIST_BINS)
    def test_edges_inf_and_nan(self, dev, ext, n_bins):
        """Below lo and -inf -> bin 0; hi, above and +inf -> last bin; NaN in
        no bin, on the GPU and CPU paths of stats.histogram alike."""
        from raft_amd.stats import histogram
        x = P.hist_edge_matrix(3)
        out = histogram(x.to(dev), n_bins, P.HIST_LO, P.HIST_HI)
        P.check_equal(out, P.histogram_oracle(x, n_bins, P.HIST_LO, P.HIST_HI), "oracle")
        P.check_equal(out, histogram(x, n_bins, P.HIST_LO, P.HIST_HI), "CPU path")
        assert int(out.sum()) == int((~torch.isnan(x)).sum())

    def test_empty(self, dev, ext):
        assert ext.histogram_f32(torch.zeros(5, 0, device=dev), 4, 0.0, 1.0).shape == (4, 0)
        out = ext.histogram_f32(torch.zeros(0, 2, device=dev), 4, 0.0, 1.0)
        assert out.shape == (4, 2) and int(out.sum()) == 0
        with pytest.raises(RuntimeError):
            ext.histogram_f32(torch.zeros(5, 2, device=dev), 0, 0.0, 1.0)
        _alive(dev)


class TestBitset:
    @pytest.mark.parametrize("n", P.BITSET_N)
    def test_set_clear_test_count(self, dev, ext, n):
        """Bit 31 of a word (the int32 sign bit), bit n-1 in the tail word,
        duplicates, set then clear."""
        from raft_amd.core import Bitset
        idx = P.bitset_indices(n)
        bs = Bitset(n, device=dev, default=False)
        bs.set(idx.to(dev), True)
        dense = P.bitset_oracle(n, idx)
        assert torch.equal(bs.to_dense().cpu(), dense)
        assert bs.count() == int(dense.sum())
        assert bool(bs.test(idx.to(dev)).all())
        bs.set(idx[::2].to(dev), False)
        dense = P.bitset_oracle(n, idx, idx[::2])
        assert torch.equal(bs.to_dense().cpu(), dense)
        assert bs.count() == int(dense.sum())
        assert torch.equal(bs.test(idx.to(dev)).cpu(), dense[idx])
        bs.set(torch.zeros(0, dtype=torch.int64, device=dev), True)    # k = 0
        assert bs.test(torch.zeros(0, dtype=torch.int64, device=dev)).shape == (0,)
        assert bs.count() == int(dense.sum())

    def test_count_grid_stride(self, dev, ext):
        """bitset_count: grid min(ceil(words / 256), 2048); 2048 * 256 + 77
        words need a second grid-stride pass."""
        from raft_amd.core import Bitset
        n = P.BITSET_COUNT_BITS
        assert Bitset(n, device=dev, default=True).count() == n
        words = torch.randint(-2 ** 31, 2 ** 31, (n // 32,), dtype=torch.int64,
                              generator=torch.Generator().manual_seed(4)).to(torch.int32)
        import numpy as np
        want = int(np.unpackbits(words.numpy().view(np.uint8)).sum())
        assert int(ext.bitset_count(words.to(dev)).item()) == want

    def test_guards_and_empty(self, dev, ext):
        words = torch.zeros(4, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError):
            ext.bitset_set_(words, torch.zeros(2, dtype=torch.int64), True)
        with pytest.raises(RuntimeError):
            ext.bitset_test(words, torch.zeros(2, dtype=torch.int64))
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        assert int(ext.bitset_count(empty).item()) == 0
        _alive(dev)


def _spmv(ext, dev, c):
    return ext.csr_spmv(c["indptr"].to(dev), c["indices"].to(dev), c["values"].to(dev),
                        c["x"].to(dev), c["n_rows"], c["n_cols"])


class TestSpmv:
    @DTYPES
    @pytest.mark.parametrize("L", P.SPMV_L)
    def test_uniform_rows_every_width(self, dev, ext, L, dtype):
        """Sub-wave width from mean nnz per row: <= 4 -> 2, <= 8 -> 4, <= 16
        -> 8, <= 32 -> 16, <= 128 -> 32, else 64. 37 rows of L entries with
        L on both sides of every threshold; integer-valued, so exact."""
        c = P.spmv_case(f"uniform_{L}", dtype)
        assert P.spmv_width(c["n_rows"], c["values"].numel()) == \
            {1: 2, 4: 2, 5: 4, 8: 4, 9: 8, 16: 8, 17: 16, 32: 16, 33: 32,
             128: 32, 129: 64, 300: 64}[L]
        P.check_equal(_spmv(ext, dev, c), P.spmv_oracle(c)[0], f"L {L} {dtype}")

    @DTYPES
    @pytest.mark.parametrize("name", ("power_law", "nnz0", "one_row", "repeated_cols"))
    def test_shapes_exact(self, dev, ext, name, dtype):
        """power_law: mean ceil(nnz / rows) = 3 -> width 2 walking one row of
        5000 entries, with empty rows; nnz0: mean 0 -> width 2, y = 0;
        one_row: 77 entries -> width 32, a single block."""
        from raft_amd.sparse.types import CSR
        from raft_amd.sparse.linalg import spmv
        c = P.spmv_case(name, dtype)
        y = P.spmv_oracle(c)[0]
        P.check_equal(_spmv(ext, dev, c), y, name)
        a = CSR(c["indptr"].to(dev), c["indices"].to(dev), c["values"].to(dev),
                c["n_rows"], c["n_cols"])
        P.check_equal(spmv(a, c["x"].to(dev)), y, f"{name} public")

    @DTYPES
    def test_random_bound(self, dev, ext, dtype):
        """|y - ref| <= gamma_len sum|a_ij x_j| per row, gamma_k = k u / (1 -
        k u): one rounding per product and at most len - 1 adds (chain,
        shuffles and fused multiply-adds included), len >= 1."""
        c = P.spmv_case("random", dtype)
        y, mass, lens = P.spmv_oracle(c)
        bound = P.gamma(lens.clamp_min(1), P.U[dtype]) * mass
        P.check_bound(_spmv(ext, dev, c), y, bound, f"random {dtype}")

    def test_empty_and_guards(self, dev, ext):
        i32 = dict(dtype=torch.int32, device=dev)
        z = torch.zeros(0, device=dev)
        y = ext.csr_spmv(torch.zeros(1, **i32), torch.zeros(0, **i32), z, z, 0, 0)
        assert y.shape == (0,)
        c = P.spmv_case("uniform_5")
        ip, ix, v, x = (c[k].to(dev) for k in ("indptr", "indices", "values", "x"))
        n, m = c["n_rows"], c["n_cols"]
        bad_calls = [
            (ip, ix, v, c["x"], n, m),                 # host x
            (ip, ix, v, x.double(), n, m),             # wrong dtype x
            (ip, ix, v, x[:-1], n, m),                 # wrong-length x
            (ip, ix, v, torch.zeros(2 * m, device=dev)[::2], n, m),  # strided x
            (ip, ix, c["values"], x, n, m),            # host values
            (ip[:-1], ix, v, x, n, m),                 # short indptr
            (ip, ix[:-1], v, x, n, m),                 # indices / values mismatch
            (c["indptr"], ix, v, x, n, m),             # host indptr
            (ip, ix.long(), v, x, n, m),               # int64 indices
            (ip, ix, v.half(), x.half(), n, m),        # unsupported dtype
        ]
        for args in bad_calls:
            with pytest.raises(RuntimeError):
                ext.csr_spmv(*args)
        from raft_amd.sparse.types import CSR
        from raft_amd.sparse.linalg import spmv
        with pytest.raises(ERR):
            spmv(CSR(ip, ix, v, n, m), x[:-1])
        _alive(dev)


class TestSddmm:
    @pytest.mark.parametrize("nnz", P.SDDMM_NNZ)
    @pytest.mark.parametrize("d", P.SDDMM_D)
    def test_exact(self, dev, ext, d, nnz):
        """Sub-wave per edge: d <= 8 -> 4 lanes, <= 32 -> 16, <= 128 -> 32,
        else 64; nnz = 0 launches nothing. Repeated edges, integer-valued."""
        a, b, rows, cols = P.sddmm_case(d, nnz)
        out = ext.sddmm(a.to(dev), b.to(dev), rows.to(dev), cols.to(dev))
        P.check_equal(out, P.sddmm_oracle(a, b, rows, cols), f"d {d} nnz {nnz}")

    def test_guards(self, dev, ext):
        a, b, rows, cols = P.sddmm_case(8, 1000)
        for args in ((a.to(dev), b, rows.to(dev), cols.to(dev)),
                     (a.to(dev), b.to(dev), rows, cols.to(dev)),
                     (a.to(dev), b.to(dev), rows.to(dev), cols[:-1].to(dev)),
                     (a.to(dev), b.double().to(dev), rows.to(dev), cols.to(dev))):
            with pytest.raises(RuntimeError):
                ext.sddmm(*args)
        _alive(dev)
