"""The fp64 reference and the comparison of the refine tests (CPU and GPU).

Bound, u = 2^-24: every term carries one rounding of the difference and one of
the fma (or square) and passes through fewer than d additions in any order:
gamma_(d+2) * S, S the fp64 sum of (x - q)^2 or of |x * q|; the second-order
part is below 4u at d <= 8192, so (d + 8) * u * S. Euclidean: the same, relative, on the root.
"""
import torch

U = 2.0 ** -24
METRICS = ("sqeuclidean", "euclidean", "inner_product")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def reference(dataset, queries, candidates, k, metric):
    """(dists fp64, ids, S) [q, k]: gather, fp64 distance, sort by (value, id), fill."""
    x, qs, cand = dataset.cpu().double(), queries.cpu().double(), candidates.cpu()
    ip = metric == "inner_product"
    bad = float("-inf") if ip else float("inf")
    dists = torch.full((cand.shape[0], k), bad, dtype=torch.float64)
    ids = torch.full((cand.shape[0], k), -1, dtype=torch.int64)
    sums = torch.zeros_like(dists)
    for i, row in enumerate(cand.tolist()):
        c = torch.tensor(sorted(v for v in row if 0 <= v < x.shape[0]), dtype=torch.int64)[:, None]
        term = x[c[:, 0]] * qs[i] if ip else (x[c[:, 0]] - qs[i]) ** 2
        val, s = term.sum(dim=1), term.abs().sum(dim=1)
        val = torch.where(val.isnan(), torch.full_like(val, bad), val)
        top = torch.argsort(-val if ip else val, stable=True)[:k]
        m = top.numel()
        dists[i, :m], ids[i, :m], sums[i, :m] = val[top], c[top, 0], s[top]
    if metric == "euclidean":
        dists, sums = dists.sqrt(), sums.sqrt()
    return dists, ids, sums


def assert_exact(got, ref, metric, d):
    """ids equal; dists equal (euclidean: within the bound of the root)."""
    (gd, gi), (rd, ri, rs) = got, ref
    assert (gd.dtype, gi.dtype) == (torch.float32, torch.int64)
    assert torch.equal(gi.cpu(), ri), (gi, ri)
    gd = gd.cpu().double()
    if metric == "euclidean":
        fin = rd.isfinite()
        assert torch.equal(gd[~fin], rd[~fin])
        assert bool(((gd - rd)[fin].abs() <= (d + 8) * U * rs[fin]).all()), (gd, rd)
    else:
        assert torch.equal(gd, rd), (gd, rd)


def assert_close(got, dataset, queries, candidates, k, metric):
    """Returned distances within the bound of the fp64 one of the returned id, best
    first; no valid candidate left out beats the k-th by more than their bounds."""
    gd, gi = got[0].cpu().double(), got[1].cpu()
    n, d = dataset.shape
    sign = -1.0 if metric == "inner_product" else 1.0
    for i in range(candidates.shape[0]):
        own = gi[i][:, None]
        assert bool((own >= 0).all())
        rd, _, rs = reference(dataset, queries[i].expand(k, d), own, 1, metric)
        tol = (d + 8) * U * rs[:, 0]
        assert bool(((gd[i] - rd[:, 0]).abs() <= tol).all()), (i, gd[i], rd[:, 0], tol)
        assert bool((sign * (gd[i][1:] - gd[i][:-1]) >= 0).all()), (i, gd[i])
        left = [v for v in candidates[i].tolist() if 0 <= v < n and v not in set(gi[i].tolist())]
        ld, _, ls = reference(dataset, queries[i].expand(len(left), d),
                              torch.tensor(left)[:, None], 1, metric)
        slack = (d + 8) * U * ls[:, 0] + tol[-1]
        assert bool((sign * (ld[:, 0] - rd[-1, 0]) >= -slack).all()), (i, ld, rd[-1])
