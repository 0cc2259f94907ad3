"""Every route of the k-means driver (cluster/kmeans.py) against exact truth.

x = c_true[label] + noise and c0 = c_true + jitter are small integers (c_true
in [-8, 8], noise and jitter in {-1, 0, 1}), so bf16 slice 0 holds every value
exactly and the residual slices are zero. Every distance, centroid sum, count
and the inertia (<= 1000 * 1088 * 4 < 2^24) is an integer that fp32 holds
exactly, whatever the order of the adds and of the atomics. So every fp32
mode, on the minimal-dispatch loop and on the generic loop alike, compares
with torch.equal against int64 truth; the one rounding, sums / counts, is a
single correctly rounded fp32 division on both sides.

1000 rows and k = 37 (padded to 128 centroid rows on the fast loop). d = 64
needs no feature padding, d = 70 pads to 128, and padded d = 1088 > 1024 is
where the verified modes leave the fast loop for the generic one while the
unverified modes stay on it. In the base data the best and second-best
distances of every row differ by at least 1 (asserted), so no tie-break
matters; the dup variant makes centroid 20 an exact copy of centroid 5, which
ties every row near them at margin 0: the exact rescan must keep the smaller
index, and cluster 20 ends empty and keeps its old centroid.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

M, K = 1000, 37
VERIFIED = ["auto", "bf16x1v", "bf16x2v"]
MODES = VERIFIED + ["bf16x2", "bf16x3", "native"]
DUP = (5, 20)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _case(d, dup=False, weighted=False):
    """Inputs and int64 truth of one Lloyd step from c0, all on the CPU."""
    g = torch.Generator().manual_seed(1234 + d)
    c_true = torch.randint(-8, 9, (K, d), generator=g)
    label = torch.randint(0, K, (M,), generator=g)
    x = c_true[label] + torch.randint(-1, 2, (M, d), generator=g)
    c0 = c_true + torch.randint(-1, 2, (K, d), generator=g)
    w = torch.randint(1, 4, (M,), generator=g) if weighted else torch.ones(M, dtype=torch.long)
    if dup:
        c0[DUP[1]] = c0[DUP[0]]
    D = ((x * x).sum(1)[:, None] + (c0 * c0).sum(1)[None, :] - 2 * (x @ c0.T))
    best2 = D.sort(dim=1).values[:, :2]
    margin = best2[:, 1] - best2[:, 0]
    if dup:
        # the tied rows are exactly those nearest the duplicated pair
        tied = margin == 0
        assert tied.any() and torch.equal(tied, D[:, DUP[0]] == best2[:, 0])
        assert (margin[~tied] >= 1).all()
    else:
        assert (margin >= 1).all()
    labels = (D * K + torch.arange(K)).argmin(1)            # ties: smallest index
    dmin = D[torch.arange(M), labels]
    sums = torch.zeros(K, d, dtype=torch.long).index_add_(0, labels, x * w[:, None])
    counts = torch.zeros(K, dtype=torch.long).index_add_(0, labels, w)
    inertia = int((dmin * w).sum())
    assert inertia < 2 ** 24 and int(sums.abs().max()) < 2 ** 24
    if not dup:
        assert int(counts.min()) > 0                        # no relocation in kmeans_fit
    c0f = c0.float()
    centroids = torch.where((counts > 0)[:, None],
                            sums.float() / counts.float()[:, None], c0f)
    return dict(x=x.float(), c0=c0f, w=w.float(), labels=labels,
                centroids=centroids, inertia=inertia, n_tied=int((margin == 0).sum()))


def _iterate_cases():
    for d in (64, 70):
        for mode in MODES:
            yield d, mode, False
        for mode in VERIFIED:
            yield d, mode, True
    # padded d > 1024: "auto" takes the generic loop, "bf16x2" stays on the
    # fast loop (its update kernel has a 64-register instance)
    yield 1088, "auto", False
    yield 1088, "bf16x2", False


@pytest.mark.parametrize("d,mode,dup", list(_iterate_cases()))
def test_iterate_one_step_exact(dev, d, mode, dup):
    from raft_amd.cluster.kmeans import kmeans_iterate
    t = _case(d, dup)
    assert (t["n_tied"] > 0) == dup
    c, inertia = kmeans_iterate(t["x"].to(dev), t["c0"].to(dev), 1, fp32_mode=mode)
    assert torch.equal(c.cpu(), t["centroids"])
    assert inertia == t["inertia"]


@pytest.mark.parametrize("d", [64, 70])
@pytest.mark.parametrize("mode", ["auto", "bf16x2", "native"])
def test_fit_one_step_exact(dev, d, mode):
    from raft_amd.cluster import KMeansParams, kmeans_fit
    t = _case(d)
    m = kmeans_fit(t["x"].to(dev), KMeansParams(n_clusters=K, max_iter=1, fp32_mode=mode),
                   init_centroids=t["c0"].to(dev))
    assert torch.equal(m.centroids.cpu(), t["centroids"])
    assert torch.equal(m.labels.cpu(), t["labels"])
    assert m.inertia == t["inertia"]


@pytest.mark.parametrize("d", [64, 70])
@pytest.mark.parametrize("mode", ["auto", "native"])
def test_fit_sample_weights_exact(dev, d, mode):
    from raft_amd.cluster import KMeansParams, kmeans_fit
    t = _case(d, weighted=True)
    m = kmeans_fit(t["x"].to(dev), KMeansParams(n_clusters=K, max_iter=1, fp32_mode=mode),
                   init_centroids=t["c0"].to(dev), sample_weights=t["w"].to(dev))
    assert torch.equal(m.centroids.cpu(), t["centroids"])
    assert torch.equal(m.labels.cpu(), t["labels"])
    assert m.inertia == t["inertia"]


def test_update_verify_binding_rejects_wide_d(dev):
    """A direct caller past the 1024 columns the kernel covers fails loudly
    (the check sits in the binding, before any launch)."""
    from raft_amd._ext import require_ext
    x, c = torch.zeros(8, 1088, device=dev), torch.zeros(2, 1088, device=dev)
    f = [torch.zeros(8, device=dev) for _ in range(3)]
    i = [torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(3)]
    with pytest.raises(RuntimeError, match="1024"):
        require_ext().kmeans_update_verify(
            x, i[0], i[1], c, f[0], f[1], i[2], f[2], torch.zeros(1, device=dev),
            torch.zeros(2, 1088, device=dev), torch.zeros(2, device=dev),
            torch.zeros(1, device=dev), lead=2.0 ** -7, tail=2.0 ** -12)


def test_state_reused_and_widened(dev):
    """One "auto" state serves repeated calls and, passed with a 2-slice
    mode, gains the residual slice in place."""
    from raft_amd.cluster.kmeans import kmeans_iter_state, kmeans_iterate
    t = _case(64)
    x, c0 = t["x"].to(dev), t["c0"].to(dev)
    state = kmeans_iter_state(x, "auto")
    assert len(state.slices) == 1
    for mode in ("auto", "auto", "bf16x2v"):
        c, inertia = kmeans_iterate(x, c0, 1, fp32_mode=mode, state=state)
        assert torch.equal(c.cpu(), t["centroids"])
        assert inertia == t["inertia"]
    assert len(state.slices) == 2
    assert kmeans_iter_state(x.cpu(), "auto") is None
    assert kmeans_iter_state(x, "native") is None
