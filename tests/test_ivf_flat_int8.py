"""IVF-Flat over int8 / uint8 rows: the dot4 list-scan kernel on the GPU and the
int64 torch path on the CPU against an int64 reference over the probed lists.
Both are exact, so distances are compared bit for bit; only which of several
exactly tied rows sits at the k-th place is left open."""
import pytest
import torch

from ivf_flat_inputs import FORCED_SIZES
from raft_amd.core.bitset import Bitset
from raft_amd.distance import DistanceType
from raft_amd.neighbors import (IvfFlatParams, IvfPqParams, ivf_flat_build, ivf_flat_extend,
                                ivf_flat_load, ivf_flat_save, ivf_flat_search, ivf_pq_build)
from raft_amd.neighbors.ivf_flat import IvfFlatIndex, _pack

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
METRICS = ["sqeuclidean", "euclidean", "inner_product"]
RANGE = {torch.int8: (-128, 128), torch.uint8: (0, 256)}
INT_IDS = dict(ids=lambda v: str(v).replace("torch.", ""))
_G = torch.Generator().manual_seed(808)
#: 500 rows and 12 queries of 17 features over the full range of each dtype
X = {t: torch.randint(*r, (500, 17), dtype=t, generator=_G) for t, r in RANGE.items()}
Q = {t: torch.randint(*r, (12, 17), dtype=t, generator=_G) for t, r in RANGE.items()}
#: two centroids, the second so far that every byte row falls into list 0
FAR = torch.zeros(2, 4096)
FAR[1, 0] = 1e5


def check(index, queries, probes, dists, ids, k, mask=None):
    """Every query against the int64 reference over its probed lists."""
    index, queries, probes = index.to("cpu"), queries.cpu().long(), probes.cpu()
    dists, ids = dists.cpu(), ids.cpu()
    ip = index.metric == DistanceType.InnerProduct
    bad = float("-inf") if ip else float("inf")
    assert dists.dtype == torch.float32 and tuple(dists.shape) == (queries.shape[0], k)
    assert ids.dtype == torch.int64 and ids.shape == dists.shape
    for i, q in enumerate(queries):
        rows, rid = zip(*(index.unpack_list(l) for l in probes[i].tolist()))
        rows, rid = torch.cat(rows).long(), torch.cat(rid)
        if mask is not None:
            rows, rid = rows[mask[rid]], rid[mask[rid]]
        exact = (rows * q).sum(1) if ip else ((rows - q) ** 2).sum(1)
        want = (exact.double().sqrt().float()
                if index.metric == DistanceType.L2SqrtExpanded else exact.float())
        n = min(k, rid.numel())
        # missing slots are (+/-inf, -1)
        assert bool((dists[i, n:] == bad).all()) and bool((ids[i, n:] == -1).all()), i
        if n == 0:
            continue
        # the k best exact values, converted once, bit for bit
        assert torch.equal(dists[i, :n], want.sort(descending=ip).values[:n]), (i, dists[i])
        # unique ids of probed, admitted rows whose own distance is the returned one
        got = ids[i, :n]
        assert got.unique().numel() == n, (i, got)
        where = (got[:, None] == rid[None, :]).int().argmax(1)
        assert torch.equal(rid[where], got), (i, got)
        assert torch.equal(want[where], dists[i, :n]), (i, got)


@pytest.mark.parametrize("d", [1, 17, 100])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_forced_list_sizes(device, dtype, metric, d):
    """Lists of 0, 1, 63, 64, 65 and 200 rows, all probed, k above the longest."""
    g = torch.Generator().manual_seed(d)
    n = sum(FORCED_SIZES)
    x = torch.randint(*RANGE[dtype], (n, d), dtype=dtype, generator=g).to(device)
    q = torch.randint(*RANGE[dtype], (9, d), dtype=dtype, generator=g).to(device)
    labels = torch.repeat_interleave(torch.arange(len(FORCED_SIZES)),
                                     torch.tensor(FORCED_SIZES))
    labels = labels[torch.randperm(n, generator=g)].to(device)
    empty = ivf_flat_build(x, IvfFlatParams(metric=metric, add_data_on_build=False),
                           centroids=x[:len(FORCED_SIZES)].float())
    index = IvfFlatIndex(empty.centroids, *_pack(x, torch.arange(n, device=device), labels,
                                                 empty.n_lists, d), metric, d, n)
    assert index.list_sizes.tolist() == list(FORCED_SIZES) and index.d_pad % 16 == 0
    dists, ids, probes = ivf_flat_search(index, q, 250, len(FORCED_SIZES),
                                         return_probes=True)
    check(index, q, probes, dists, ids, 250)


@pytest.mark.gpu
@pytest.mark.parametrize("qg", [4, 32])
@pytest.mark.parametrize("nq", [1, 8, 9, 33])
@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
def test_pair_group_boundaries(dtype, nq, qg):
    """One list of 500 rows: full and short pair groups, and the row split."""
    g = torch.Generator().manual_seed(nq)
    q = torch.randint(*RANGE[dtype], (nq, 17), dtype=dtype, generator=g).cuda()
    index = ivf_flat_build(X[dtype].cuda(), centroids=FAR[:, :17])
    assert index.list_sizes.tolist() == [500, 0]
    probes = torch.zeros((nq, 1), dtype=torch.int64, device="cuda")
    dists, ids = ivf_flat_search(index, q, 7, probes=probes, qg=qg)
    check(index, q, probes, dists, ids, 7)


@pytest.mark.parametrize("device", DEVICES)
def test_range_at_the_widest_tier(device):
    """d = 4096, every element at an extreme: the largest int32 intermediates."""
    if device == "cuda":
        from raft_amd._ext import require_ext
        assert require_ext().ivf_flat_scan_max_qg(4096, 1) == 8
        assert require_ext().ivf_flat_scan_max_qg(4096) == 4
    full = lambda v, rows, dtype: torch.full((rows, 4096), v, dtype=dtype, device=device)
    x = torch.cat([full(255, 64, torch.uint8), full(0, 64, torch.uint8)])
    q = torch.cat([full(255, 1, torch.uint8), full(0, 1, torch.uint8)])
    index = ivf_flat_build(x, centroids=FAR)
    assert index.list_sizes.tolist() == [128, 0]
    probes = torch.zeros((2, 1), dtype=torch.int64, device=device)
    dists, ids = ivf_flat_search(index, q, 128, probes=probes)
    check(index, q, probes, dists, ids, 128)
    assert torch.equal(dists.cpu(), torch.tensor([0.0] * 64 + [266342400.0] * 64).expand(2, 128))
    x, q = full(-128, 128, torch.int8), full(127, 9, torch.int8)
    probes = torch.zeros((9, 1), dtype=torch.int64, device=device)
    for metric, value in (("inner_product", -66584576.0), ("sqeuclidean", 266342400.0),
                          ("euclidean", 16320.0)):
        index = ivf_flat_build(x, IvfFlatParams(metric=metric), centroids=FAR)
        dists, ids = ivf_flat_search(index, q, 128, probes=probes)
        check(index, q, probes, dists, ids, 128)
        assert bool((dists == value).all()), (metric, dists)


@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_bitset_filter(device, dtype):
    x, q = X[dtype].to(device), Q[dtype].to(device)
    index = ivf_flat_build(x, IvfFlatParams(metric="euclidean"), centroids=x[:4].float())
    mask = torch.rand(500, generator=torch.Generator().manual_seed(3)) < 0.5
    dists, ids, probes = ivf_flat_search(index, q, 10, 2, return_probes=True,
                                         filter=Bitset.from_dense(mask.to(device)))
    check(index, q, probes, dists, ids, 10, mask=mask)


@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_extend_and_its_dtype_check(device, dtype):
    x, q = X[dtype].to(device), Q[dtype].to(device)
    first = ivf_flat_build(x[:250], centroids=x[:4].float())
    index = ivf_flat_extend(first, x[250:])
    assert index.n_rows == 500 and first.n_rows == 250 and index.dtype == dtype
    dists, ids, probes = ivf_flat_search(index, q, 10, 4, return_probes=True)
    check(index, q, probes, dists, ids, 10)
    other = torch.uint8 if dtype == torch.int8 else torch.int8
    for wrong in (x[250:].to(other), x[250:].float()):
        with pytest.raises(ValueError):
            ivf_flat_extend(first, wrong)


@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_save_load(device, dtype, tmp_path):
    x, q = X[dtype].to(device), Q[dtype].to(device)
    index = ivf_flat_build(x, IvfFlatParams(metric="inner_product"), centroids=x[:4].float())
    ivf_flat_save(index, str(tmp_path / "index.ivf"))
    back = ivf_flat_load(str(tmp_path / "index.ivf"), device=device)
    assert back.dtype == dtype and back.metric == index.metric and back.dim == 17
    assert torch.equal(back.data, index.data) and torch.equal(back.indices, index.indices)
    for a, b in zip(ivf_flat_search(index, q, 10, 2), ivf_flat_search(back, q, 10, 2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("device", DEVICES)
def test_query_dtype_and_ivf_pq_rejections(device):
    x, q = X[torch.int8].to(device), Q[torch.int8].to(device)
    index = ivf_flat_build(x, centroids=x[:4].float())
    for wrong in (q.float(), q.to(torch.uint8), q.bfloat16()):
        with pytest.raises(ValueError):
            ivf_flat_search(index, wrong, 5, 2)
    with pytest.raises(ValueError):
        ivf_pq_build(x, IvfPqParams(n_lists=4))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
def test_gpu_against_cpu(dtype, metric):
    """The index built on the CPU and moved, with the CPU's probes."""
    cpu = ivf_flat_build(X[dtype], IvfFlatParams(metric=metric),
                         centroids=X[dtype][:4].float())
    d0, _, probes = ivf_flat_search(cpu, Q[dtype], 10, 2, return_probes=True)
    d1, i1 = ivf_flat_search(cpu.to("cuda"), Q[dtype].cuda(), 10, probes=probes.cuda())
    assert torch.equal(d0, d1.cpu())
    check(cpu, Q[dtype], probes, d1, i1, 10)
