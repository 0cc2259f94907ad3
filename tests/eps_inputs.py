"""Shared inputs and fp64 ground truth for the epsilon-neighborhood tests
(tests/test_epsilon_neighborhood.py on the CPU, tests/test_gpu_epsilon_
neighborhood.py on the GPU). Everything here runs on the CPU; references are
computed once per process and never modified."""
import functools

import torch

#: (m, n, d), one edge each: single element; d-pad + one partial tile + n not
#: a multiple of 32; two row tiles + ragged column tile; five column tiles +
#: multi-K; a plain multi-tile; a second super-tile group on each axis
SHAPES = [(1, 1, 1), (65, 63, 33), (130, 200, 100), (129, 513, 257),
          (257, 300, 64), (1030, 40, 64), (40, 1030, 64)]

#: a pair may be left out of a real-valued comparison only inside this band:
#: |d2_fp64 - eps_sq| <= BAND * (xn + yn), 4x the largest fp32 expanded-form
#: error measured for the offset input (0.6e-6 * (xn + yn))
BAND = 4e-6
MAX_EXCLUDED_SHARE = 1e-3
#: at most this many pairs sit inside the band for any input here (the
#: quantile thresholds are themselves sample points, so shapes with fewer
#: than 1000 pairs cannot meet the share bound with even one tie)
MAX_EXCLUDED_PAIRS = 2


def d2_fp64(x, y):
    """Ground truth: fp64 squared distances (what torch.cdist computes before
    its square root; exact for the small-integer inputs)."""
    xd, yd = x.double(), y.double()
    out = torch.empty(xd.shape[0], yd.shape[0], dtype=torch.float64)
    step = max(1, (1 << 24) // max(yd.shape[0] * yd.shape[1], 1))
    for r0 in range(0, xd.shape[0], step):
        diff = xd[r0:r0 + step, None, :] - yd[None, :, :]
        out[r0:r0 + step] = (diff * diff).sum(-1)
    return out


def fp32_round(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def randn_case(m, n, d):
    """randn inputs with eps_sq at the fp32-rounded 5% and 50% quantiles of
    the true distances. Returns (x, y, d2, band, [eps...])."""
    g = torch.Generator().manual_seed(1000 + 7 * m + 3 * n + d)
    x = torch.randn(m, d, generator=g)
    y = torch.randn(n, d, generator=g)
    d2 = d2_fp64(x, y)
    flat = d2.flatten().sort().values
    eps = [fp32_round(flat[int(q * (flat.numel() - 1))]) for q in (0.05, 0.5)]
    if m * n == 1:
        # the only pair IS every quantile; add thresholds that decide it
        eps += [fp32_round(0.5 * flat[0]), fp32_round(2.0 * flat[0])]
    return x, y, d2, band_of(x, y), eps


def band_of(x, y):
    xn = x.double().pow(2).sum(1)
    yn = y.double().pow(2).sum(1)
    return BAND * (xn[:, None] + yn[None, :])


def compare_outside_band(adj, d2, band, eps):
    """Assert adj equals the fp64 truth for every pair outside the band and
    that the band holds only a negligible share. Returns the excluded count."""
    truth = d2 <= eps
    excluded = (d2 - eps).abs() <= band
    n_excl = int(excluded.sum())
    limit = max(MAX_EXCLUDED_PAIRS, MAX_EXCLUDED_SHARE * d2.numel())
    print(f"eps_sq={eps:.9g} pairs={d2.numel()} neighbors={int(truth.sum())} "
          f"excluded={n_excl}")
    assert n_excl <= limit, (n_excl, limit)
    wrong = (adj.cpu() != truth) & ~excluded
    assert int(wrong.sum()) == 0, f"{int(wrong.sum())} pairs wrong outside the band"
    return n_excl


@functools.lru_cache(maxsize=None)
def tie_case():
    """Small integers: every product and sum is exact in bf16 and fp32, so
    no exclusion is allowed. Returns (x, y, d2)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (130, 70), generator=g).float()
    y = torch.randint(-3, 4, (200, 70), generator=g).float()
    return x, y, d2_fp64(x, y)


TIE_EPS = 519.0


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """tie_case with a few y rows copied from x: at eps_sq = 0 the result is
    exactly the duplicates."""
    x, y, _ = tie_case()
    y = y.clone()
    for j, i in ((0, 5), (63, 129), (64, 0), (199, 77)):
        y[j] = x[i]
    return x, y, d2_fp64(x, y)


@functools.lru_cache(maxsize=None)
def offset_cloud_case():
    """The input that proves the recheck: norms ~1090 against eps_sq = 0.5,
    so an unverified 1-slice bf16 evaluation misplaces hundreds of pairs.
    Returns (x, y, d2, band, eps_sq)."""
    g = torch.Generator().manual_seed(11)
    m, d = 192, 64
    x = 4 + torch.randn(m, d, generator=g)
    u = torch.randn(3 * m, d, generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    r2 = 0.5 * (0.5 + torch.rand(3 * m, generator=g))
    y = torch.cat([x.repeat_interleave(3, 0) + u * r2.sqrt()[:, None],
                   4 + torch.randn(61, d, generator=g)])
    return x, y, d2_fp64(x, y), band_of(x, y), 0.5


def unpack(words, n):
    """int32 [m, ceil(n/32)] words -> bool [m, n], plus the tail bits."""
    words = words.cpu()
    shifts = torch.arange(32, dtype=torch.int32)
    bits = ((words.unsqueeze(2) >> shifts) & 1).bool().reshape(words.shape[0], -1)
    return bits[:, :n], bits[:, n:]


def csr_to_dense(indptr, indices, m, n):
    indptr, indices = indptr.cpu(), indices.cpu()
    dense = torch.zeros(m, n, dtype=torch.bool)
    rows = torch.repeat_interleave(torch.arange(m), indptr[1:] - indptr[:-1])
    dense[rows, indices.long()] = True
    return dense


def check_contract(adj, words, csr, vd, m, n, device_type):
    """Output contract + the packed <-> bool <-> CSR equivalences."""
    indptr, indices, vd_csr = csr
    assert adj.dtype == torch.bool and tuple(adj.shape) == (m, n)
    assert words.dtype == torch.int32 and tuple(words.shape) == (m, (n + 31) // 32)
    assert vd.dtype == torch.int64 and tuple(vd.shape) == (m + 1,)
    assert indptr.dtype == torch.int64 and tuple(indptr.shape) == (m + 1,)
    assert indices.dtype == torch.int32 and indices.dim() == 1
    for t in (adj, words, vd, indptr, indices, vd_csr):
        assert t.device.type == device_type
    bits, tail = unpack(words, n)
    assert not bool(tail.any()), "tail bits must be zero"
    assert torch.equal(bits, adj.cpu())
    assert torch.equal(csr_to_dense(indptr, indices, m, n), adj.cpu())
    vd, indptr, indices = vd.cpu(), indptr.cpu(), indices.cpu()
    assert torch.equal(vd, vd_csr.cpu())
    assert torch.equal(vd[:m], adj.cpu().sum(1))
    assert int(vd[m]) == int(vd[:m].sum()) == indices.numel()
    assert int(indptr[0]) == 0 and torch.equal(indptr[1:], vd[:m].cumsum(0))
    if indices.numel() > 1:
        # strictly increasing inside every row: a non-increase may only sit
        # on a row boundary
        drop = (indices[1:] <= indices[:-1]).nonzero().flatten() + 1
        starts = set(indptr.tolist())
        assert all(int(p) in starts for p in drop), "indices not sorted in a row"
