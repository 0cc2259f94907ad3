"""Every select_k engine on adversarial rows, checked exactly against the
fp64 CPU oracle of tests/select_k_inputs.py: in-range distinct indices,
gathered values bitwise equal to the output, output equal to the oracle.

The engines are called through the extension directly (ext.select_k with an
explicit algo code, ext.select_k_generic), so the kernel under test is
certain; the public raft_amd.matrix.select_k and sparse csr_select_k routes
are then checked with the same checker. Shapes are the smallest that reach
each branch of csrc/select_k.hip."""
import pytest
import torch

import select_k_inputs as S

pytestmark = pytest.mark.gpu

RADIX, WARPSORT = 1, 2
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
F32_FAMILIES = S.families_for(4099, F32)          # all of them


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[1]
    if isinstance(v, bool):
        return "min" if v else "max"
    return None


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


@pytest.fixture(params=[True, False], ids=["min", "max"])
def select_min(request):
    return request.param


def run_fp32(ext, dev, x, k, select_min, algo, do_sort):
    """One fp32 engine, then the checker. The binding returns int32 indices
    (the public wrapper widens them); everything else is checked as is."""
    vals, idx = ext.select_k(x.to(dev), k, select_min, algo, do_sort)
    assert idx.dtype == torch.int32
    S.check_select(x, vals, idx.long(), k, select_min, do_sort)


def run_generic(ext, dev, x, k, select_min):
    vals, idx = ext.select_k_generic(x.to(dev), None, k=k, select_min=select_min)
    S.check_select(x, vals, idx, k, select_min, False)   # output is unsorted


def ragged(x, lens, dev):
    """Flat values and int64 row offsets of the rows x[r, :lens[r]]."""
    flat = torch.cat([x[r, :ln] for r, ln in enumerate(lens)])
    off = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
    return flat.to(dev), off.to(dev)


# --------------------------------------------------------------------------
# block radix, compacted-candidate fast path
# --------------------------------------------------------------------------

class TestRadixFastPath:
    @pytest.mark.parametrize("name", F32_FAMILIES)
    def test_odd_row_length(self, dev, ext, name, select_min):
        """n = 4099: the scalar tail of the float4 scan, and rows 1.. start
        off a 16-byte boundary. k on both sides of the warpsort bound and at
        the LDS sort capacity."""
        x = S.family(name, 5, 4099)
        for k in (1, 64, 65, 1000, 2048):
            for do_sort in (True, False):
                run_fp32(ext, dev, x, k, select_min, RADIX, do_sort)

    @pytest.mark.parametrize("name", S.families_for(2048, F32))
    def test_whole_row(self, dev, ext, name, select_min):
        x = S.family(name, 5, 2048)
        for do_sort in (True, False):
            run_fp32(ext, dev, x, 2048, select_min, RADIX, do_sort)


class TestRadixFallback:
    """More than CAND_CAP = 16384 elements share the top ordinal byte with
    the k-th: the kernel re-scans the full row instead of its workspace."""

    @pytest.mark.parametrize("n", [16384, 16385, 20001])
    def test_same_exponent(self, dev, ext, n, select_min):
        x = S.family("same_exponent", 3, n)
        for k in (1, 100, 2048):
            for do_sort in (True, False):
                run_fp32(ext, dev, x, k, select_min, RADIX, do_sort)

    @pytest.mark.parametrize("name", ["few_values", "all_equal"])
    def test_ties(self, dev, ext, name, select_min):
        x = S.family(name, 3, 20001)
        for k in (1, 100, 2048):
            run_fp32(ext, dev, x, k, select_min, RADIX, True)


def test_radix_grid_stride(dev, ext, select_min):
    """batch > 4096 blocks: every block takes a second row with the same
    candidate workspace and LDS counters, on rows full of ties."""
    run_fp32(ext, dev, S.family("few_values", 4100, 4099), 70, select_min,
             RADIX, True)


# --------------------------------------------------------------------------
# wave-register warpsort queue
# --------------------------------------------------------------------------

class TestWarpsort:
    @pytest.mark.parametrize("name", F32_FAMILIES)
    def test_shapes(self, dev, ext, name, select_min):
        """batch = 7 is no multiple of the 4 waves of a block."""
        for n, k in [(1, 1), (63, 63), (64, 64), (65, 64), (127, 2),
                     (4096, 64), (10000, 33)]:
            run_fp32(ext, dev, S.family(name, 7, n), k, select_min, WARPSORT,
                     True)

    def test_launch_cap(self, dev, ext, select_min):
        """more rows than 65536 blocks of 4 waves: the row loop strides."""
        run_fp32(ext, dev, S.family("randn", 262149, 64), 8, select_min,
                 WARPSORT, True)


# --------------------------------------------------------------------------
# generic threshold + filter engine
# --------------------------------------------------------------------------

class TestGeneric:
    @pytest.mark.parametrize(
        "dtype,name", [(dt, f) for dt in (F32, F64, BF16, F16)
                       for f in S.families_for(5000, dt)], ids=_id)
    def test_dtypes(self, dev, ext, dtype, name, select_min):
        x = S.family(name, 3, 5000, dtype)
        for k in (1, 2049, 5000):
            run_generic(ext, dev, x, k, select_min)

    @pytest.mark.parametrize("name", ["randn", "few_values"])
    def test_grid_stride_fp64(self, dev, ext, name, select_min):
        run_generic(ext, dev, S.family(name, 4100, 64, F64), 3, select_min)

    @pytest.mark.parametrize("dtype", [F32, F64, BF16, F16], ids=_id)
    @pytest.mark.parametrize("name", ["nan_mix", "inf_heavy", "few_values"])
    def test_ragged_rows(self, dev, ext, name, dtype, select_min):
        k = 8
        lens = S.ragged_lens(k, 5000)
        x = S.family(name, len(lens), 5000, dtype)
        flat, off = ragged(x, lens, dev)
        vals, pos = ext.select_k_generic(flat, off, k=k, select_min=select_min)
        S.check_select(x, vals, pos, k, select_min, False, pad_lens=lens)


# --------------------------------------------------------------------------
# public raft_amd.matrix.select_k
# --------------------------------------------------------------------------

def run_public(dev, x, k, select_min, x_dev=None):
    from raft_amd.matrix import select_k
    x_dev = x.to(dev) if x_dev is None else x_dev
    for sorted_ in (True, False):
        vals, idx = select_k(x_dev, k, select_min=select_min, sorted=sorted_)
        S.check_select(x, vals, idx, k, select_min, sorted_)


class TestPublicSelectK:
    @pytest.mark.parametrize("name", ["randn", "ulp_ladder", "few_values",
                                      "inf_heavy", "nan_mix", "nan_tail"])
    @pytest.mark.parametrize("n,k", [(4096, 64), (4097, 64), (5000, 2048),
                                     (5000, 2049)])
    def test_native_dispatch_boundaries(self, dev, ext, n, k, name, select_min):
        """warpsort | radix | radix at its largest k | generic."""
        run_public(dev, S.family(name, 5, n), k, select_min)

    @pytest.mark.parametrize("name", ["randn", "ulp_ladder", "few_values",
                                      "inf_heavy"])
    def test_vendor_dispatch_boundary(self, dev, ext, name, select_min):
        """k = 65 at n = 4096 goes to the vendor top-k, whose NaN order is
        torch's own: the NaN families are left to the native routes."""
        run_public(dev, S.family(name, 5, 4096), 65, select_min)

    @pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
    @pytest.mark.parametrize("name", ["randn", "few_values", "inf_heavy",
                                      "nan_mix", "nan_tail"])
    def test_half_widen_route(self, dev, ext, name, dtype, select_min):
        run_public(dev, S.family(name, 3, 5000, dtype), 100, select_min)

    @pytest.mark.parametrize("dtype,k", [(F64, 16), (F64, 5000), (F32, 2049),
                                         (BF16, 2049), (F16, 2049)], ids=_id)
    @pytest.mark.parametrize("name", ["randn", "few_values", "inf_heavy",
                                      "nan_mix", "nan_tail"])
    def test_generic_route_sorted(self, dev, ext, name, dtype, k, select_min):
        """the [batch, k] slab is ordered in Python: NaN last both ways."""
        run_public(dev, S.family(name, 3, 5000, dtype), k, select_min)

    @pytest.mark.parametrize("dtype,n,k", [(F32, 500, 16), (F32, 5000, 100),
                                           (F32, 5000, 2049), (F64, 5000, 16),
                                           (BF16, 5000, 100)], ids=_id)
    def test_non_contiguous(self, dev, ext, dtype, n, k, select_min):
        x = S.family("nan_mix", 6, n, dtype)
        x_dev = x.t().contiguous().to(dev).t()       # [6, n] view of [n, 6]
        assert not x_dev.is_contiguous()
        run_public(dev, x, k, select_min, x_dev=x_dev)

    @pytest.mark.parametrize("name", ["randn", "inf_heavy", "all_equal",
                                      "nan_mix", "nan_tail"])
    @pytest.mark.parametrize("n", [262144, 262147])
    def test_two_level_split(self, dev, ext, n, name, select_min):
        """batch < 256 over a long row: per-segment select, then a select
        over the candidates. n = 262147 leaves a remainder; with nan_tail the
        row has 3 numbers, so k - 3 slots must be the row's own NaNs."""
        for batch in (1, 3):
            x = S.family(name, batch, n)
            x_dev = x.to(dev)
            for k in (8, 100):
                run_public(dev, x, k, select_min, x_dev=x_dev)


# --------------------------------------------------------------------------
# sparse csr_select_k, GPU branch
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, F64], ids=_id)
@pytest.mark.parametrize("name", ["nan_mix", "nan_tail", "few_values"])
def test_csr_select_k(dev, ext, name, dtype, select_min):
    """Ragged rows; column ids are a random injection per row, mapped back
    to the position in the row so that the same gather rule applies."""
    from raft_amd.sparse.select_k import csr_select_k
    from raft_amd.sparse.types import CSR
    k, n_cols = 8, 100000
    lens = S.ragged_lens(k, 5000)
    x = S.family(name, len(lens), 5000, dtype)
    flat, off = ragged(x, lens, dev)
    g = torch.Generator().manual_seed(5)
    col_rows = [torch.randperm(n_cols, generator=g)[:ln] for ln in lens]
    a = CSR(off.to(torch.int32), torch.cat(col_rows).to(torch.int32).to(dev),
            flat, len(lens), n_cols)
    vals, cols = csr_select_k(a, k, select_min=select_min)
    assert cols.dtype == torch.int64
    cols = cols.cpu()
    pos = torch.empty_like(cols)
    for r, row_cols in enumerate(col_rows):
        where = {int(c): p for p, c in enumerate(row_cols.tolist())}
        # a column id that is not in the row becomes an out-of-range position
        pos[r] = torch.tensor([-1 if c == -1 else where.get(c, lens[r])
                               for c in cols[r].tolist()])
    S.check_select(x, vals, pos, k, select_min, True, pad_lens=lens)
