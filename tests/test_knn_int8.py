"""Exact int8 / uint8 pairwise distances and brute-force kNN: the integer MFMA
kernels on the GPU and the int64 torch path on the CPU against an unexpanded
int64 reference, converted to fp32 once. Both are exact, so distances are
compared bit for bit; only which of several exactly tied rows is returned is
left open."""
import pytest
import torch

from raft_amd.distance import pairwise_distance
from raft_amd.neighbors.brute_force import BruteForceIndex, knn

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
METRICS = ["sqeuclidean", "euclidean", "inner_product"]
RANGE = {torch.int8: (-128, 128), torch.uint8: (0, 256)}
INT_IDS = dict(ids=lambda v: str(v).replace("torch.", ""))


def rand(dtype, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(*RANGE[dtype], shape, dtype=dtype, generator=g)


def reference(x, y, metric):
    """[m, n] from int64 sums over the features, 16 rows of x at a time."""
    x, y = x.cpu().long(), y.cpu().long()
    if metric == "inner_product":
        return (x @ y.t()).float()
    sq = torch.cat([((c[:, None, :] - y[None, :, :]) ** 2).sum(-1) for c in x.split(16)])
    return sq.double().sqrt().float() if metric == "euclidean" else sq.float()


def check(dists, ids, want, k):
    """The k smallest reference values bit for bit; unique ids whose own
    reference distance is the returned one."""
    dists, ids = dists.cpu(), ids.cpu()
    assert dists.dtype == torch.float32 and tuple(dists.shape) == (want.shape[0], k)
    assert ids.dtype == torch.int64 and ids.shape == dists.shape
    assert torch.equal(dists, want.sort(dim=1).values[:, :k])
    assert all(row.unique().numel() == k for row in ids)
    assert int(ids.min()) >= 0 and int(ids.max()) < want.shape[1]
    assert torch.equal(torch.gather(want, 1, ids), dists)


# ragged edges over several tiles; an interior tile and one K step; d padded to
# two steps; three steps, where the double buffer wraps
@pytest.mark.parametrize("shape", [(1, 1, 1), (129, 257, 17), (256, 128, 128),
                                   (130, 131, 129), (128, 128, 384)], ids=str)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_pairwise(device, dtype, metric, shape):
    m, n, d = shape
    x, y = rand(dtype, (m, d), m + d), rand(dtype, (n, d), n * d)
    out = pairwise_distance(x.to(device), y.to(device), metric=metric)
    assert out.dtype == torch.float32 and out.device.type == device
    assert torch.equal(out.cpu(), reference(x, y, metric))


@pytest.mark.parametrize("device", DEVICES)
def test_extremes_at_the_widest_d(device):
    """d = 4096, every element at an extreme: the largest int32 intermediates."""
    full = lambda v, dtype: torch.full((3, 4096), v, dtype=dtype, device=device)
    cases = [(full(-128, torch.int8), full(127, torch.int8), -66584576.0),
             (full(0, torch.uint8), full(255, torch.uint8), 0.0),
             (full(255, torch.uint8), full(255, torch.uint8), 255.0 * 255 * 4096)]
    for a, b, ip in cases:
        sq, root = (0.0, 0.0) if a[0, 0] == b[0, 0] else (266342400.0, 16320.0)
        for metric, value in (("inner_product", ip), ("sqeuclidean", sq), ("euclidean", root)):
            out = pairwise_distance(a, b, metric=metric)
            assert bool((out == value).all()), (metric, out)


# n = 2000 takes the filter path on the GPU and n = 50 the tiled one; at
# d = 300 a squared distance can pass 2^24, where fp32 stops being exact
@pytest.mark.parametrize("n, d", [(2000, 17), (50, 17), (2000, 300)])
@pytest.mark.parametrize("metric", METRICS[:2])
@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_knn(device, dtype, metric, n, d):
    x, q = rand(dtype, (n, d), n), rand(dtype, (130, d), d)
    want = reference(q, x, metric)
    x, q = x.to(device), q.to(device)
    check(*knn(x, q, 10, metric=metric), want, 10)
    check(*BruteForceIndex(x, metric=metric).search(q, 10), want, 10)


@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_knn_inner_product(device, dtype):
    """The tiled path, which selects the smallest values of any metric."""
    x, q = rand(dtype, (500, 17), 5), rand(dtype, (9, 17), 6)
    dists, ids = knn(x.to(device), q.to(device), 10, metric="inner_product")
    check(dists, ids, reference(q, x, "inner_product"), 10)


@pytest.mark.parametrize("dtype", RANGE, **INT_IDS)
@pytest.mark.parametrize("device", DEVICES)
def test_overflow_fallback(device, dtype):
    """20000 identical rows all pass the filter: more than the 16384 slots."""
    x, q = torch.full((20000, 16), 7, dtype=dtype), rand(dtype, (3, 16), 7)
    dists, ids = knn(x.to(device), q.to(device), 5)
    check(dists, ids, reference(q, x[:1], "sqeuclidean").expand(3, 20000), 5)


@pytest.mark.parametrize("device", DEVICES)
def test_rejections(device):
    x = torch.zeros((100, 17), dtype=torch.int8, device=device)
    for other in (x.to(torch.uint8), x.float()):
        with pytest.raises(ValueError):
            pairwise_distance(x, other)
        with pytest.raises(ValueError):
            knn(x, other[:5], 3)
    with pytest.raises(ValueError):
        pairwise_distance(x, x, metric="cosine")
    with pytest.raises(ValueError):
        knn(x, x[:5], 3, metric="l1")
    if device == "cuda":
        wide = torch.zeros((100, 4097), dtype=torch.int8, device=device)
        with pytest.raises(ValueError):
            pairwise_distance(wide, wide)
        with pytest.raises(ValueError):
            knn(wide, wide[:5], 3)
