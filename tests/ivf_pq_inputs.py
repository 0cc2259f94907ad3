"""The fp64 oracle, acceptance rules and cases of the IVF-PQ tests (CPU and
GPU). The oracle runs on the CPU from index.centroids, index.codebooks,
unpack_list and the probes; inputs are seeded torch.randn.

Tolerances, u = 2^-24, D the exact value, R = |q - c|, e = (q - c) - cb exact:
  Squared L2. The code subtracts rho = fl(q - c), rounded BEFORE a possibly
    nearly equal codebook entry is subtracted from it: the computed difference
    is e_i + eps_i with |eps_i| <= u |q_i - c_i| + u |e_i| to first order, so
    the sum of squares is off by 2 sum |e_i eps_i| + sum eps_i^2
    <= 2u (sqrt(D) R + D) + 2 u^2 (R^2 + D) (Cauchy-Schwarz). The d_rot fmas
    and pq_dim + 3 additions of non-negative terms add (d_rot + pq_dim + 3) u D
    in any order. Doubled for the second-order terms:
      4u sqrt(D) R + 2 (d_rot + pq_dim + 4) u D + 4 u^2 R^2.
  Euclidean: the same through the square root (d sqrt(D) = dD / (2 sqrt(D)))
    plus its own rounding: 2u R + (d_rot + pq_dim + 4) u sqrt(D).
  InnerProduct: d_rot + pq_dim + 2 products and additions of terms bounded by
    |q| (|c| + |cb|): 2 (d_rot + pq_dim + 2) u sum |q| (|c| + |cb|).
  Encode: the unexpanded sum of pq_len non-negative terms, each difference
    rounded twice: a chosen entry's fp64 distance is within
    2 (pq_len + 3) u relative of the subspace's fp64 minimum.
"""
from types import SimpleNamespace

import torch

from raft_amd.core.bitset import Bitset
from raft_amd.core.resources import Resources
from raft_amd.neighbors import (IvfPqParams, ivf_pq_build, ivf_pq_extend, ivf_pq_load,
                                ivf_pq_save, ivf_pq_search)

U = 2.0 ** -24
METRICS = ("sqeuclidean", "euclidean", "inner_product")
#: (d, pq_dim): pq_len 3, 1, 1, 1, 2, 32; d_rot > d at (10, 4); 128 KiB table at (256, 128)
SHAPES = ((10, 4), (16, 16), (24, 24), (7, 7), (256, 128), (96, 3))
FORCED_SIZES = (0, 1, 63, 64, 65, 200)


def _decoded(index, l):
    """fp64 decoded residuals [size, d_rot] and ids of list l."""
    codes, ids = index.unpack_list(l)
    books = index.codebooks.double().permute(0, 2, 1)          # [pq_dim, 256, pq_len]
    dec = books[torch.arange(index.pq_dim), codes.long()]
    return dec.reshape(codes.shape[0], index.d_rot), ids


def oracle(index, lists, query, probes, mask=None):
    """(ids, fp64 distance, tolerance) of the admissible rows of the probes."""
    m, n = index.metric.name, index.d_rot + index.pq_dim
    q = torch.zeros(index.d_rot, dtype=torch.float64)
    q[:index.dim] = query.double()
    ids, dist, tol = [], [], []
    for l in probes:
        dec, lid = lists[l]
        c = torch.zeros_like(q)
        c[:index.dim] = index.centroids[l].double()
        if m == "InnerProduct":
            dl = (c + dec) @ q
            tl = 2 * (n + 2) * U * ((c.abs() + dec.abs()) @ q.abs())
        else:
            r = q - c
            big_r = r.norm()
            dl = ((r - dec) ** 2).sum(dim=1)
            if m == "L2SqrtExpanded":
                dl = dl.sqrt()
                tl = 2 * U * big_r + (n + 4) * U * dl
            else:
                tl = (4 * U * dl.sqrt() * big_r + 2 * (n + 4) * U * dl
                      + 4 * U * U * big_r ** 2)
        ids.append(lid), dist.append(dl), tol.append(tl)
    ids, dist, tol = torch.cat(ids), torch.cat(dist), torch.cat(tol)
    if mask is not None:
        keep = mask[ids]
        ids, dist, tol = ids[keep], dist[keep], tol[keep]
    return ids, dist, tol


def check(index, queries, probes, dists, ids, k, mask=None):
    """Per query: valid count and padding; ids unique and admissible; distances
    within tolerance; nothing worse than the k-th best by 2 tol; best first."""
    index = index.to("cpu")
    lists = [_decoded(index, l) for l in range(index.n_lists)]
    dists, ids, probes = dists.cpu(), ids.cpu(), probes.cpu()
    nq = queries.shape[0]
    assert (dists.dtype, ids.dtype) == (torch.float32, torch.int64)
    assert tuple(dists.shape) == tuple(ids.shape) == (nq, k)
    sign = -1.0 if index.metric.name == "InnerProduct" else 1.0
    for i in range(nq):
        cid, cd, ctol = oracle(index, lists, queries[i], probes[i].tolist(), mask)
        n_valid = min(k, cid.numel())
        got_d, got_i = dists[i].double(), ids[i]
        assert bool(((got_i >= 0) == (torch.arange(k) < n_valid)).all()), (i, got_i)
        assert bool((got_i[n_valid:] == -1).all()), (i, got_i)
        assert bool((got_d[n_valid:] == sign * float("inf")).all()), (i, got_d)
        if n_valid == 0:
            continue
        vi, vd = got_i[:n_valid], got_d[:n_valid]
        assert vi.unique().numel() == n_valid, (i, vi)
        where = {int(v): j for j, v in enumerate(cid.tolist())}
        assert all(int(v) in where for v in vi.tolist()), (i, vi)
        at = torch.tensor([where[int(v)] for v in vi.tolist()])
        err = (vd - cd[at]).abs()
        assert bool((err <= ctol[at]).all()), (i, err, ctol[at])
        top = torch.argsort(cd, descending=sign < 0, stable=True)[:k]
        slack = 2 * torch.maximum(ctol[at], ctol[top].max())
        assert bool((sign * (cd[at] - cd[top[-1]]) <= slack).all()), (i, cd[at], slack)
        assert bool((sign * (vd[1:] - vd[:-1]) >= 0).all()), (i, vd)


def codes_by_id(index):
    """(codes [n, pq_dim], list of every row) in dataset-id order."""
    index = index.to("cpu")
    parts = [index.unpack_list(l) for l in range(index.n_lists)]
    codes, ids = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    label = torch.repeat_interleave(torch.arange(index.n_lists), index.list_sizes)
    order = torch.argsort(ids)
    assert torch.equal(ids[order], torch.arange(index.n_rows))
    return codes[order], label[order]


def check_codes(index, x, codes, label):
    """The encode rule of the module docstring."""
    index = index.to("cpu")
    r = torch.zeros(x.shape[0], index.d_rot, dtype=torch.float64)
    r[:, :index.dim] = (x - index.centroids[label]).double()    # fp32, as encoded
    r = r.view(-1, index.pq_dim, index.pq_len).permute(1, 0, 2)
    dist = torch.cdist(r, index.codebooks.double().permute(0, 2, 1)) ** 2   # [s, n, 256]
    got = dist.gather(2, codes.long().t().unsqueeze(2)).squeeze(2)
    assert bool((got <= dist.min(dim=2).values * (1 + 2 * (index.pq_len + 3) * U)).all())


def forced_data(d, pq_dim, n_lists=len(FORCED_SIZES), sizes=FORCED_SIZES, nq=33):
    """Far centroids (8 on coordinate l) with sizes[l] rows of spread 0.5
    around each, random codebooks of the residuals' scale."""
    g = torch.Generator().manual_seed(1000 * d + pq_dim)
    centroids = torch.zeros(n_lists, d)
    centroids[torch.arange(n_lists), torch.arange(n_lists)] = 8.0
    label = torch.repeat_interleave(torch.arange(n_lists), torch.tensor(sizes))
    label = label[torch.randperm(label.numel(), generator=g)]
    x = centroids[label] + 0.5 * torch.randn(label.numel(), d, generator=g)
    q = centroids[torch.arange(nq) % n_lists] + 0.5 * torch.randn(nq, d, generator=g)
    books = 0.5 * torch.randn(pq_dim, -(-d // pq_dim), 256, generator=g)
    return SimpleNamespace(x=x, q=q, centroids=centroids, books=books, label=label)


def forced_index(device, metric, d, pq_dim, **kw):
    f = forced_data(d, pq_dim, **kw)
    index = ivf_pq_build(f.x.to(device), IvfPqParams(metric=metric),
                         centroids=f.centroids.to(device), codebooks=f.books.to(device))
    assert index.codes.numel() == index.indices.numel() * index.pq_dim_pad
    return f, index


def _search(index, q, k, n_probes, **kw):
    return ivf_pq_search(index, q.to(index.device), k, n_probes, return_probes=True, **kw)


def case_search(device, metric, d, pq_dim):
    """Forced list sizes; n_probes 1, 3, all; k beyond a query's candidates."""
    f, index = forced_index(device, metric, d, pq_dim)
    assert index.list_sizes.tolist() == list(FORCED_SIZES)
    assert (index.pq_len, index.d_rot) == (-(-d // pq_dim), pq_dim * -(-d // pq_dim))
    for n_probes, k in ((1, 5), (3, 70), (len(FORCED_SIZES), 400)):
        dd, ii, pp = _search(index, f.q, k, n_probes)
        assert dd.device.type == device and tuple(pp.shape) == (f.q.shape[0], n_probes)
        check(index, f.q, pp, dd, ii, k)
    probes = torch.zeros((3, 1), dtype=torch.int64, device=device)     # the empty list
    dd, ii, pp = _search(index, f.q[:3], 2, 1, probes=probes)
    assert bool((ii == -1).all()) and bool(torch.isinf(dd).all())


def case_long_list(device, metric):
    """One query on one 1000-row list: the scan's grid y is 4."""
    f, index = forced_index(device, metric, 20, 5, n_lists=2, sizes=(1000, 0), nq=1)
    dd, ii, pp = _search(index, f.q, 7, 1)
    assert pp.tolist() == [[0]] and index.list_sizes.tolist() == [1000, 0]
    check(index, f.q, pp, dd, ii, 7)


def case_filter(device, metric):
    f, index = forced_index(device, metric, 10, 4)
    mask = torch.rand(f.x.shape[0], generator=torch.Generator().manual_seed(3)) < 0.5
    d1, i1, p1 = _search(index, f.q, 9, 3, filter=mask.to(device))
    check(index, f.q, p1, d1, i1, 9, mask=mask)
    d2, i2, _ = _search(index, f.q, 9, 3, filter=Bitset.from_dense(mask.to(device)))
    assert torch.equal(i1, i2) and torch.equal(d1, d2)


def case_chunking(device, metric):
    """Two workspace budgets (all queries at once, 4 per chunk): bitwise equal."""
    f, index = forced_index(device, metric, 24, 24)
    d0, i0, p0 = _search(index, f.q, 9, 3)
    res = Resources(torch.device(device))
    res.set_workspace_limit(2 * 4 * 4 * 3 * index.max_list_pad)
    d1, i1, p1 = _search(index, f.q, 9, 3, res=res)
    assert torch.equal(p0, p1) and torch.equal(d0, d1) and torch.equal(i0, i1)


def encode_data(pq_len, pq_dim=3, n=300):
    """Rows 100.. are exactly centroid + entry; entry 200 repeats entry 17."""
    d = pq_dim * pq_len - (pq_len > 1)                  # the last feature is padding
    g = torch.Generator().manual_seed(40 + pq_len)
    books = 0.5 * torch.randn(pq_dim, pq_len, 256, generator=g)
    books[:, :, 200] = books[:, :, 17]
    if pq_len > 1:
        books[-1, -1] = 0.0                             # as training on zeros gives
    centroids = torch.zeros(4, d)
    centroids[torch.arange(4), torch.arange(4) % d] = 8.0 * (1 + torch.arange(4) // d)
    label = torch.arange(n) % 4
    want = torch.randint(0, 256, (n, pq_dim), generator=g)
    want[100:110] = 200
    entry = books.permute(0, 2, 1)[torch.arange(pq_dim), want].reshape(n, -1)[:, :d]
    x = centroids[label] + torch.cat([0.3 * torch.randn(100, d, generator=g), entry[100:]])
    want[want == 200] = 17
    return SimpleNamespace(x=x, centroids=centroids, books=books, label=label, want=want)


def case_encode(device, pq_len):
    e = encode_data(pq_len)
    index = ivf_pq_build(e.x.to(device), IvfPqParams(), centroids=e.centroids.to(device),
                         codebooks=e.books.to(device))
    assert index.pq_len == pq_len
    codes, label = codes_by_id(index)
    assert torch.equal(label, e.label)
    check_codes(index, e.x, codes, label)
    assert torch.equal(codes[100:].long(), e.want[100:])
    pad = index.to("cpu")._padded_codes()
    assert bool((pad[:, index.pq_dim:] == 0).all())
    return index, codes


def blobs(n=2000, d=16, n_centers=8):
    g = torch.Generator().manual_seed(11)
    centers = 4 * torch.randn(n_centers, d, generator=g)
    x = centers[torch.arange(n) % n_centers] + torch.randn(n, d, generator=g)
    return SimpleNamespace(x=x, q=x[:20] + 0.1 * torch.randn(20, d, generator=g))


def case_end_to_end(device, path):
    """Training, extend, save / load, reconstruct_list: 2000 x 16 blobs, pq_dim
    = 8, n_lists = 8. On the CPU path with this seed the mean squared
    reconstruction error is 0.290, the residual norm 45.6: a factor of 157."""
    b = blobs()
    x = b.x.to(device)
    first = ivf_pq_build(x[:1500], IvfPqParams(n_lists=8, pq_dim=8, metric="euclidean"))
    index = ivf_pq_extend(first, x[1500:])
    assert (first.n_rows, index.n_rows, int(index.list_sizes.sum())) == (1500, 2000, 2000)
    old, _ = codes_by_id(first)
    new, label = codes_by_id(index)                     # asserts the ids are a permutation
    assert torch.equal(new[:1500], old)                 # old codes are kept
    dd, ii, pp = _search(index, b.q, 10, 3)
    check(index, b.q, pp, dd, ii, 10)
    ivf_pq_save(index, path)
    back = ivf_pq_load(path, device=device)
    assert (back.metric, back.dim, back.pq_dim, back.n_rows) == (index.metric, 16, 8, 2000)
    for name in ("centroids", "codebooks", "list_offsets", "list_sizes", "codes", "indices"):
        assert torch.equal(getattr(back, name), getattr(index, name)), name
    d1, i1, p1 = _search(back, b.q, 10, 3)
    assert torch.equal(p1, pp) and torch.equal(i1, ii) and torch.equal(d1, dd)
    err = res = 0.0
    for l in range(index.n_lists):
        rows, ids = index.reconstruct_list(l)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (ids.numel(), 16)
        err += float(((rows - x[ids]) ** 2).sum())
        res += float(((x[ids] - index.centroids[l]) ** 2).sum())
    assert err < res
