"""Shared inputs and checks of the sparse-distance tests (CPU and GPU files)."""
import torch

from raft_amd.sparse import CSR

# (metric name, p)
METRICS = [("inner_product", 2.0), ("sqeuclidean", 2.0), ("euclidean", 2.0),
           ("sqeuclidean_unexp", 2.0), ("euclidean_unexp", 2.0), ("cosine", 2.0),
           ("correlation", 2.0), ("l1", 2.0), ("lp", 3.0), ("canberra", 2.0),
           ("hamming", 2.0), ("jensenshannon", 2.0), ("hellinger", 2.0),
           ("jaccard", 2.0), ("dice", 2.0), ("russelrao", 2.0)]
METRIC_IDS = [m for m, _ in METRICS]
UNSUPPORTED = ["linf", "kl_divergence", "braycurtis", "haversine"]
# compared on the squares: the sqrt of a near-zero cancelling sum cannot carry
# an absolute tolerance set for the sum
SQUARED = {"euclidean", "euclidean_unexp", "jensenshannon", "hellinger"}


def kind_for(metric):
    if metric in ("jensenshannon", "hellinger"):
        return "prob"
    if metric in ("russelrao", "jaccard", "dice"):
        return "binary"
    return "signed"


def csr_from_mask(mask, vals, dtype=torch.float64, shuffle_seed=None):
    """CSR holding vals[i, c] at every True position of mask (zeros in vals
    become stored explicit zeros). shuffle_seed permutes the entries inside
    each row, so column ids come out unsorted."""
    m, d = mask.shape
    lengths = mask.sum(dim=1)
    indptr = torch.zeros(m + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lengths, 0)
    rows, cols = mask.nonzero(as_tuple=True)
    v = vals[rows, cols]
    if shuffle_seed is not None:
        g = torch.Generator().manual_seed(shuffle_seed)
        key = rows.double() + torch.rand(rows.numel(), generator=g, dtype=torch.float64) * 0.5
        order = torch.argsort(key)
        cols, v = cols[order], v[order]
    return CSR(indptr.to(torch.int32), cols.to(torch.int32), v.to(dtype), m, d)


def random_csr(m, d, density, seed, kind="signed", dtype=torch.float64, fill_first=True,
               shuffle_seed=None):
    """Random CSR [m, d]. kind: "signed" values in [-1, 1]; "prob" rows that
    sum to 1; "binary" ones; "int" integers in {-3..3} (zeros are kept as
    stored explicit zeros). fill_first stores entry (0, 0), so even a 1 x 1
    matrix holds one value."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(m, d, generator=g) < density
    if fill_first and m > 0 and d > 0:
        mask[0, 0] = True
    if kind == "signed":
        vals = torch.rand(m, d, generator=g, dtype=torch.float64) * 2 - 1
    elif kind == "prob":
        vals = (torch.rand(m, d, generator=g, dtype=torch.float64) + 1e-3) * mask
        vals = vals / vals.sum(dim=1, keepdim=True).clamp_min(1e-300)
    elif kind == "binary":
        vals = torch.ones(m, d, dtype=torch.float64)
    elif kind == "int":
        vals = torch.randint(-3, 4, (m, d), generator=g).double()
    else:
        raise ValueError(kind)
    # what the GPU sees in fp32 is what the fp64 reference sees
    vals = vals.float().double()
    return csr_from_mask(mask, vals, dtype, shuffle_seed)


def with_empty_rows(a, rows):
    """Copy of CSR a with the given rows emptied."""
    lengths = a.row_lengths().to(torch.int64)
    keep_row = torch.ones(a.n_rows, dtype=torch.bool)
    keep_row[list(rows)] = False
    keep = torch.repeat_interleave(keep_row, lengths)
    new_len = lengths * keep_row
    indptr = torch.zeros(a.n_rows + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(new_len, 0)
    return CSR(indptr.to(a.indptr.dtype), a.indices[keep], a.values[keep], a.n_rows, a.n_cols)


def empty_csr(m, d, dtype=torch.float64):
    return CSR(torch.zeros(m + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
               torch.zeros(0, dtype=dtype), m, d)


def cast(a, dtype):
    return CSR(a.indptr, a.indices, a.values.to(dtype), a.n_rows, a.n_cols)


def check_close(metric, got, ref, rtol, atol):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    if metric in SQUARED:
        got, ref = got * got, ref * ref
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)


def check_knn(metric, got_d, got_i, ref_d, true, rtol, atol):
    """Tie-tolerant kNN check: the returned distances are close to the
    reference's, and the true distances at the returned indices reproduce them."""
    got, ref = got_d.double().cpu(), ref_d.double().cpu()
    gathered = true.double().cpu().gather(1, got_i.cpu())
    assert got.shape == ref.shape
    if metric in SQUARED:
        got, ref, gathered = got * got, ref * ref, gathered * gathered
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)
    torch.testing.assert_close(gathered, got, rtol=rtol, atol=atol)
