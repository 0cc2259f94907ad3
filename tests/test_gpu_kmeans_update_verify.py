"""ext.kmeans_update_verify (csrc/kmeans.hip) called directly, against exact
truth.

x and the centroids are integers in [-3, 3]: every distance (<= 36 d), every
centroid sum, every count and the inertia (<= 1000 * 36 * 320 < 2^24) is an
integer that fp32 holds exactly, whatever the order of the adds and of the
atomics between waves. So every output compares with torch.equal against
int64 truth.

1000 rows give a chunk of 8 rows per wave and 125 waves; k = 37 sorted keys
give runs of ~27 rows that start and end inside the row batches and at chunk
edges. dmin / dmin2 are supplied by hand: most rows get a huge margin (no
rescan); every tenth row gets margin 0 and rescans; every second one of those
carries a wrong label, so the rescan reassigns it and moves its contribution.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

M, K = 1000, 37
LEAD, TAIL = 2.0 ** -7, 2.0 ** -12      # the bf16x1v bound


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from raft_amd._ext import require_ext
    return require_ext()


@functools.lru_cache(maxsize=None)
def _case(d):
    g = torch.Generator().manual_seed(4321 + d)
    x = torch.randint(-3, 4, (M, d), generator=g).cuda()
    c = torch.randint(-3, 4, (K, d), generator=g).cuda()
    D = ((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :]
         - 2 * (x.double() @ c.double().T).long())           # int64 [M, K]
    true = (D * K + torch.arange(K, device=D.device)).argmin(1)   # ties: smallest
    rows = torch.arange(M, device=D.device)
    rescans = rows % 10 == 3
    wrong = rescans & (rows % 20 == 13)
    given = torch.where(wrong, (true + 1) % K, true)
    final = true                      # unrescanned rows were given the truth
    dmin_in = torch.zeros(M, device=D.device)
    dmin2_in = torch.where(rescans, 0.0, 1.0e6).to(dmin_in)
    sums = torch.zeros(K, d, dtype=torch.long, device=D.device).index_add_(0, final, x)
    counts = torch.bincount(final, minlength=K)
    dmin = D[rows, final]
    return dict(x=x.float(), c=c.float(), xn=(x * x).sum(1).float(),
                cn_max=(c * c).sum(1).max().float().reshape(1), given=given.int(),
                dmin_in=dmin_in, dmin2_in=dmin2_in, sums=sums.float(),
                counts=counts.float(), dmin=dmin.float(), amin=final.int(),
                inertia=dmin.sum().float().reshape(1),
                n_wrong=int(wrong.sum()), n_rescan=int(rescans.sum()))


# d = 192: the scalar column map; 256: VEC4 at 4 registers per row; 320: VEC4
# at 16 registers per row with a ragged last quad
@pytest.mark.parametrize("d", [192, 256, 320])
def test_update_verify_exact(dev, ext, d):
    t = _case(d)
    assert t["n_rescan"] == 100 and t["n_wrong"] == 50
    assert float(t["inertia"]) < 2 ** 24
    keys_sorted, perm = torch.sort(t["given"])
    dmin, amin = t["dmin_in"].clone(), t["given"].clone()
    sums = torch.zeros(K, d, device=dev)
    counts = torch.zeros(K, device=dev)
    inertia = torch.zeros(1, device=dev)
    ext.kmeans_update_verify(t["x"], perm.to(torch.int32), keys_sorted, t["c"], t["xn"],
                             dmin, amin, t["dmin2_in"], t["cn_max"], sums, counts,
                             inertia, lead=LEAD, tail=TAIL)
    assert torch.equal(amin, t["amin"])
    assert torch.equal(dmin, t["dmin"])
    assert torch.equal(counts, t["counts"])
    assert torch.equal(sums, t["sums"])
    assert torch.equal(inertia, t["inertia"])
