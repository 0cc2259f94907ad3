"""Shared inputs, the fp64 oracle and the acceptance rules of the IVF-Flat
tests (tests/test_ivf_flat.py on the CPU, tests/test_gpu_ivf_flat.py on the
GPU). Everything here runs on the CPU; data sets are generated once per
process and never modified.

Tolerances follow from the arithmetic, u = 2^-24:
  L2 (squared or with square root): rtol = 2 * (d + 3) * u. Every term of the
    unexpanded sum is non-negative, so the bound is relative and independent
    of the summation order.
  InnerProduct: atol = 2 * d * u * sum_i |x_i| * |q_i|, in fp64 per pair.
"""
import functools
from types import SimpleNamespace

import torch

from raft_amd.distance import DistanceType
from raft_amd.neighbors import IvfFlatParams, ivf_flat_build

U = 2.0 ** -24
METRICS = ("sqeuclidean", "euclidean", "inner_product")
DTYPES = (torch.float32, torch.bfloat16)
DTYPE_IDS = dict(ids=lambda v: str(v).replace("torch.", ""))
#: the tolerance the project's own default-mode pairwise test uses
#: (tests/test_gpu_kernels.py, test_l2_epilogue_and_pairwise)
PAIRWISE_RTOL, PAIRWISE_ATOL = 1e-3, 1e-3
#: list sizes of the forced-shape case (list l has FORCED_SIZES[l] rows)
FORCED_SIZES = (0, 1, 63, 64, 65, 200)


def is_ip(metric):
    return metric in ("inner_product", DistanceType.InnerProduct)


def is_sqrt(metric):
    return metric in ("euclidean", DistanceType.L2SqrtExpanded)


def dist_fp64(rows, query, metric):
    """fp64 distances of rows [c, d] to one query [d] and their tolerances."""
    x, q = rows.double(), query.double()
    d = x.shape[1]
    if is_ip(metric):
        return x @ q, 2 * d * U * (x.abs() @ q.abs())
    dist = ((x - q) ** 2).sum(dim=1)
    if is_sqrt(metric):
        dist = dist.sqrt()
    return dist, 2 * (d + 3) * U * dist


def best_k(dist, k, metric):
    """Positions of the k best of dist (all of them when fewer), best first."""
    order = torch.argsort(dist, descending=is_ip(metric), stable=True)
    return order[:k]


def unpacked(index):
    """[(rows, ids)] of every list of a CPU index."""
    return [index.unpack_list(l) for l in range(index.n_lists)]


def oracle(lists, query, probes, metric, mask=None):
    """The admissible rows of the probed lists: (ids, fp64 dist, tol)."""
    rows = torch.cat([lists[l][0] for l in probes])
    ids = torch.cat([lists[l][1] for l in probes])
    if mask is not None:
        keep = mask[ids]
        rows, ids = rows[keep], ids[keep]
    dist, tol = dist_fp64(rows, query, metric)
    return ids, dist, tol


def check(index, queries, probes, dists, ids, k, mask=None):
    """Properties (a)-(e) of every query against the oracle over its probes.
    index: a CPU index; mask: bool over dataset ids or None."""
    metric = index.metric
    lists = unpacked(index)
    dists, ids, probes = dists.cpu(), ids.cpu(), probes.cpu()
    q = queries.shape[0]
    assert dists.dtype == torch.float32 and tuple(dists.shape) == (q, k)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (q, k)
    sign = -1.0 if is_ip(metric) else 1.0
    bad = sign * float("inf")
    worst_c = worst_d = 0.0
    for i in range(q):
        cid, cd, ctol = oracle(lists, queries[i].float(), probes[i].tolist(), metric, mask)
        n_valid = min(k, cid.numel())
        got_d, got_i = dists[i].double(), ids[i]
        # (a) valid count, the rest (+/-inf, -1)
        assert bool((got_i[:n_valid] >= 0).all()), (i, got_i)
        assert bool((got_i[n_valid:] == -1).all()), (i, got_i)
        assert bool((got_d[n_valid:] == bad).all()), (i, got_d)
        if n_valid == 0:
            continue
        vi, vd = got_i[:n_valid], got_d[:n_valid]
        # (b) unique, inside the probed lists, admitted by the filter
        assert vi.unique().numel() == n_valid, (i, vi)
        where = {int(v): j for j, v in enumerate(cid.tolist())}
        assert all(int(v) in where for v in vi.tolist()), (i, vi)
        at = torch.tensor([where[int(v)] for v in vi.tolist()])
        # (c) the returned distance is the fp64 distance of its id
        err = (vd - cd[at]).abs()
        assert bool((err <= ctol[at]).all()), (i, err, ctol[at])
        # (d) no returned id is worse than the k-th best, widened by twice the
        # tolerance (its own, and the largest among the true k best)
        top = best_k(cd, k, metric)
        t = cd[top[-1]]
        slack = 2 * torch.maximum(ctol[at], ctol[top].max())
        assert bool((sign * (cd[at] - t) <= slack).all()), (i, cd[at], t, slack)
        # (e) best first
        assert bool((sign * (vd[1:] - vd[:-1]) >= 0).all()), (i, vd)
        worst_c = max(worst_c, float((err / ctol[at].clamp_min(1e-300)).max()))
        worst_d = max(worst_d, float((sign * (cd[at] - t) / slack.clamp_min(1e-300)).max()))
    print(f"q={q} k={k} max_err/tol={worst_c:.3g} max_excess/slack={worst_d:.3g}")


def check_full_scan(x, metric, queries, dists, ids, k, id_of_row=None):
    """Exactness against an fp64 scan of ALL rows of x: the j-th returned
    distance matches the j-th fp64 best within the tolerance, and the id sets
    match except where fp64 distances are within the tolerance of the k-th."""
    dists, ids = dists.cpu().double(), ids.cpu()
    sign = -1.0 if is_ip(metric) else 1.0
    differ = 0
    for i in range(queries.shape[0]):
        dist, tol = dist_fp64(x.float(), queries[i].float(), metric)
        top = best_k(dist, k, metric)
        want = top if id_of_row is None else id_of_row[top]
        assert bool((ids[i] >= 0).all())
        rows = ids[i] if id_of_row is None else torch.tensor(
            [int((id_of_row == v).nonzero()[0]) for v in ids[i].tolist()])
        slack = torch.maximum(tol[rows], tol[top].max())
        assert bool(((dists[i] - dist[top]).abs() <= slack).all()), (i, dists[i], dist[top])
        extra = set(ids[i].tolist()) ^ set(want.tolist())
        differ += len(extra)
        t = dist[top[-1]]
        for v in extra:
            r = v if id_of_row is None else int((id_of_row == v).nonzero()[0])
            assert abs(float(dist[r] - t)) <= 2 * float(slack.max()), (i, v, dist[r], t)
    print(f"ids outside the fp64 top-k (near ties): {differ}")


def check_probes(index, queries, probes):
    """Every chosen centroid's fp64 distance is no worse than the fp64
    n_probes-th best within the pairwise tolerance (applied, as in the
    project's pairwise tests, to squared L2 distances and to products)."""
    metric = index.metric
    c, qd = index.centroids.cpu().double(), queries.cpu().double()
    probes = probes.cpu()
    n_probes = probes.shape[1]
    assert probes.dtype == torch.int64 and probes.shape[0] == queries.shape[0]
    ref = qd @ c.t() if is_ip(metric) else torch.cdist(qd, c) ** 2
    sign = -1.0 if is_ip(metric) else 1.0
    for i in range(queries.shape[0]):
        assert probes[i].unique().numel() == n_probes
        t = ref[i][best_k(ref[i], n_probes, metric)[-1]]
        got = ref[i][probes[i]]
        tol = 2 * PAIRWISE_ATOL + PAIRWISE_RTOL * (got.abs() + t.abs())
        assert bool((sign * (got - t) <= tol).all()), (i, got, t)


def sets_match_up_to_ties(index, queries, probes, ids_a, ids_b, k, mask=None):
    """Two results over the same probes hold the same ids except where the
    fp64 distance is within twice the tolerance of the k-th best."""
    lists = unpacked(index)
    ids_a, ids_b, probes = ids_a.cpu(), ids_b.cpu(), probes.cpu()
    for i in range(queries.shape[0]):
        extra = (set(ids_a[i].tolist()) ^ set(ids_b[i].tolist())) - {-1}
        if not extra:
            continue
        cid, cd, ctol = oracle(lists, queries[i].float(), probes[i].tolist(),
                               index.metric, mask)
        top = best_k(cd, k, index.metric)
        t = cd[top[-1]]
        for v in extra:
            j = int((cid == v).nonzero()[0])
            assert abs(float(cd[j] - t)) <= 2 * float(max(ctol[j], ctol[top].max()))


@functools.lru_cache(maxsize=None)
def base_data():
    """Case 1: n = 5000, d = 100, 70 queries, random normal."""
    g = torch.Generator().manual_seed(1234)
    return SimpleNamespace(x=torch.randn(5000, 100, generator=g),
                           q=torch.randn(70, 100, generator=g), n_lists=16, k=10)


@functools.lru_cache(maxsize=None)
def base_index(metric, dtype, device="cpu"):
    b = base_data()
    return ivf_flat_build(b.x.to(device, dtype),
                          IvfFlatParams(n_lists=b.n_lists, metric=metric))


@functools.lru_cache(maxsize=None)
def width_data(d, n=600):
    g = torch.Generator().manual_seed(77 + d)
    return SimpleNamespace(x=torch.randn(n, d, generator=g),
                           q=torch.randn(20, d, generator=g))


@functools.lru_cache(maxsize=None)
def forced_data(d=10):
    """Well-separated centroids (8 on coordinate l for list l) with
    FORCED_SIZES[l] points of spread 0.5 around each."""
    g = torch.Generator().manual_seed(99)
    n_lists = len(FORCED_SIZES)
    centroids = torch.zeros(n_lists, d)
    centroids[torch.arange(n_lists), torch.arange(n_lists)] = 8.0
    label = torch.repeat_interleave(torch.arange(n_lists), torch.tensor(FORCED_SIZES))
    perm = torch.randperm(label.numel(), generator=g)   # lists interleaved in x
    label = label[perm]
    x = centroids[label] + 0.5 * torch.randn(label.numel(), d, generator=g)
    q = centroids[torch.arange(40) % n_lists] + 0.5 * torch.randn(40, d, generator=g)
    # query 0 sits between the empty list 0 and the 1-row list 1
    q[0] = (centroids[0] + centroids[1]) / 2
    return SimpleNamespace(x=x, q=q, centroids=centroids, label=label)


def forced_index(metric="sqeuclidean", dtype=torch.float32, device="cpu"):
    f = forced_data()
    index = ivf_flat_build(f.x.to(device, dtype), IvfFlatParams(metric=metric),
                           centroids=f.centroids.to(device))
    assert index.list_sizes.tolist() == list(FORCED_SIZES), index.list_sizes
    return index


@functools.lru_cache(maxsize=None)
def one_list_data(d=20, n=200):
    """Two far centroids, every row and every query near the first."""
    g = torch.Generator().manual_seed(5)
    centroids = torch.zeros(2, d)
    centroids[1, 0] = 100.0
    return SimpleNamespace(x=torch.randn(n, d, generator=g),
                           q=torch.randn(33, d, generator=g), centroids=centroids)


def half_mask(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) < 0.5


# ---------------------------------------------------------------------------
# The cases, shared by the CPU and the GPU test file (device = "cpu" / "cuda")
# ---------------------------------------------------------------------------

def _search(index, q, k, n_probes, **kw):
    from raft_amd.neighbors import ivf_flat_search
    return ivf_flat_search(index, q.to(index.device), k, n_probes, return_probes=True, **kw)


def case_exactness(device, metric, dtype):
    """Case 1: n_probes = n_lists against the fp64 full scan."""
    b = base_data()
    index = base_index(metric, dtype, device)
    d, i, p = _search(index, b.q, b.k, b.n_lists)
    assert d.device.type == device and i.device.type == device
    check_full_scan(b.x.to(dtype), metric, b.q, d, i, b.k)
    check(index.to("cpu"), b.q, p, d, i, b.k)


def case_few_probes(device, metric, dtype, n_probes):
    """Case 2: the oracle over the returned probes, and the probes themselves."""
    b = base_data()
    index = base_index(metric, dtype, device)
    d, i, p = _search(index, b.q, b.k, n_probes)
    assert tuple(p.shape) == (b.q.shape[0], n_probes)
    check_probes(index, b.q, p)
    check(index.to("cpu"), b.q, p, d, i, b.k)


def case_forced_lists(device, metric, dtype):
    """Case 3: list sizes {0, 1, 63, 64, 65, 200}."""
    f = forced_data()
    index = forced_index(metric, dtype, device)
    cpu = index.to("cpu")
    for n_probes, k in ((1, 5), (2, 70), (6, 300)):
        d, i, p = _search(index, f.q, k, n_probes)
        check(cpu, f.q, p, d, i, k)
    if not is_ip(metric):
        # query 0 probes only the empty and the 1-row list: one valid result
        d, i, p = _search(index, f.q[:1], 4, 2)
        assert set(p[0].tolist()) == {0, 1}
        assert int((i[0] >= 0).sum()) == 1 and i[0, 1:].tolist() == [-1, -1, -1]
    # the empty list alone
    probes = torch.zeros((3, 1), dtype=torch.int64)
    d, i, p = _search(index, f.q[:3], 2, 1, probes=probes.to(index.device))
    assert bool((i == -1).all()) and bool(torch.isinf(d).all())
    check(cpu, f.q[:3], p, d, i, 2)


def case_width(device, d, dtype, n=600, n_lists=4, given_centroids=False, **kw):
    """Case 4: feature widths that are no multiple of the 16-byte chunk, and
    the wide rows of the three query-group tiers."""
    w = width_data(d, n)
    x = w.x.to(device, dtype)
    centroids = w.x[:n_lists].to(device) if given_centroids else None
    index = ivf_flat_build(x, IvfFlatParams(n_lists=n_lists), centroids=centroids)
    assert index.d_pad % index.vec == 0 and index.d_pad >= d
    d_, i_, p_ = _search(index, w.q, 5, 2, **kw)
    check(index.to("cpu"), w.q, p_, d_, i_, 5)
    return index


def case_filter(device, metric, dtype):
    """Case 6: Bitset and bool masks; a mask that removes a whole probed list."""
    from raft_amd.core.bitset import Bitset
    b = base_data()
    index = base_index(metric, dtype, device)
    cpu = index.to("cpu")
    mask = half_mask(b.x.shape[0])
    d1, i1, p1 = _search(index, b.q, b.k, 3, filter=mask.to(index.device))
    check(cpu, b.q, p1, d1, i1, b.k, mask=mask)
    assert bool(mask[i1.cpu()[i1.cpu() >= 0]].all())
    bits = Bitset.from_dense(mask.to(index.device))
    d2, i2, _ = _search(index, b.q, b.k, 3, filter=bits)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)
    # remove the first probed list of query 0 entirely
    gone = int(p1[0, 0])
    mask2 = torch.ones(b.x.shape[0], dtype=torch.bool)
    mask2[cpu.unpack_list(gone)[1]] = False
    d3, i3, p3 = _search(index, b.q, b.k, 3, filter=mask2.to(index.device))
    check(cpu, b.q, p3, d3, i3, b.k, mask=mask2)
    assert bool(mask2[i3.cpu()[i3.cpu() >= 0]].all())


def case_chunking(device, metric, dtype, exact):
    """Case 7: a workspace limit that forces several query chunks."""
    from raft_amd.core.resources import Resources
    b = base_data()
    index = base_index(metric, dtype, device)
    n_probes = 3
    d0, i0, p0 = _search(index, b.q, b.k, n_probes)
    res = Resources(torch.device(device))
    per_query = 4 * n_probes * index.max_list_pad
    res.set_workspace_limit(2 * 16 * per_query)      # 16 queries per chunk
    d1, i1, p1 = _search(index, b.q, b.k, n_probes, res=res)
    assert torch.equal(p0, p1)
    if exact:
        assert torch.equal(d0, d1) and torch.equal(i0, i1)
    else:
        check(index.to("cpu"), b.q, p1, d1, i1, b.k)
        assert torch.equal(i0, i1)


def case_extend(device, metric, dtype):
    """Case 8: build on one half, extend with the other."""
    from raft_amd.neighbors import ivf_flat_extend
    b = base_data()
    x = b.x.to(device, dtype)
    n = x.shape[0]
    half = n // 2
    first = ivf_flat_build(x[:half], IvfFlatParams(n_lists=b.n_lists, metric=metric))
    full = ivf_flat_extend(first, x[half:])
    assert full.n_rows == n and first.n_rows == half
    assert torch.equal(full.centroids, first.centroids)
    d, i, _ = _search(full, b.q, b.k, b.n_lists)
    check_full_scan(b.x.to(dtype), metric, b.q, d, i, b.k)
    # explicit ids for the new rows
    new_ids = torch.arange(n + 1000, n + 1000 + (n - half), device=x.device)
    shifted = ivf_flat_extend(first, x[half:], new_ids)
    id_of_row = torch.cat([torch.arange(half), new_ids.cpu()])
    d, i, _ = _search(shifted, b.q, b.k, b.n_lists)
    check_full_scan(b.x.to(dtype), metric, b.q, d, i, b.k, id_of_row=id_of_row)
    # an index without data, then extend
    empty = ivf_flat_build(x, IvfFlatParams(n_lists=b.n_lists, metric=metric,
                                            add_data_on_build=False))
    assert empty.n_rows == 0 and empty.indices.numel() == 0
    d, i, _ = _search(empty, b.q, 3, 2)
    assert bool((i == -1).all())
    d, i, _ = _search(ivf_flat_extend(empty, x), b.q, b.k, b.n_lists)
    check_full_scan(b.x.to(dtype), metric, b.q, d, i, b.k)


def case_pack_unpack(device, dtype):
    """Case 9: unpack_list is the inverse of the packing."""
    for index, x in ((base_index("sqeuclidean", dtype, device), base_data().x),
                     (forced_index("sqeuclidean", dtype, device), forced_data().x)):
        x = x.to(dtype)
        assert bool((index.list_offsets % 64 == 0).all())
        assert int(index.list_offsets[-1]) == index.indices.numel()
        assert index.data.numel() == index.indices.numel() * index.d_pad
        rows, ids = zip(*unpacked(index))
        assert [r.shape[0] for r in rows] == index.list_sizes.tolist()
        rows, ids = torch.cat(rows).cpu(), torch.cat(ids).cpu()
        order = torch.argsort(ids)
        assert torch.equal(ids[order], torch.arange(x.shape[0]))
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(rows[order].view(bits), x.view(bits))
        assert int((index.indices == -1).sum()) == index.indices.numel() - x.shape[0]
        for l in range(index.n_lists):
            r0, r1 = int(index.list_offsets[l]), int(index.list_offsets[l + 1])
            size = int(index.list_sizes[l])
            assert bool((index.indices[r0:r0 + size] >= 0).all())
            assert bool((index.indices[r0 + size:r1] == -1).all())


def case_save_load(device, metric, dtype, path):
    """Case 10: the round trip through one file."""
    from raft_amd.neighbors import ivf_flat_load, ivf_flat_save
    b = base_data()
    index = base_index(metric, dtype, device)
    ivf_flat_save(index, path)
    back = ivf_flat_load(path, device=device)
    assert back.metric == index.metric and back.dim == index.dim
    assert back.n_rows == index.n_rows and back.dtype == index.dtype
    assert back.device.type == device
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(back.data.view(bits), index.data.view(bits))
    for name in ("centroids", "list_offsets", "list_sizes", "indices"):
        assert torch.equal(getattr(back, name), getattr(index, name)), name
    d0, i0, p0 = _search(index, b.q, b.k, 3)
    d1, i1, p1 = _search(back, b.q, b.k, 3)
    assert torch.equal(p0, p1) and torch.equal(i0, i1) and torch.equal(d0, d1)
