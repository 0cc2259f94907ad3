"""csrc/nn_descent.hip (engine="kernel") against the torch paths of neighbors.nn_descent,
which tests/test_nn_descent.py checks against literal loops."""
import pytest
import torch

import cagra_inputs as C
import nn_descent_inputs as N
from refine_inputs import U
from raft_amd.core.resources import Resources
from raft_amd.neighbors import nn_descent, nn_descent_kernel_serves
from raft_amd.neighbors.nn_descent import local_join, merge_candidates, row_sqnorms

pytestmark = pytest.mark.gpu


def equal(got, ref):
    return all(a.dtype == b.dtype and torch.equal(a.cpu(), b) for a, b in zip(got, ref))


@pytest.mark.parametrize("n,d,S,dtype,view", [
    (300, 20, 4, torch.float32, None),                       # ragged chunk
    (300, 1, 8, torch.float32, None),
    (500, 128, 32, torch.bfloat16, None),                    # the full 64 x 128 tile
    (400, 200, 16, torch.float16, None),                     # several chunks, ragged end
    (300, 4096, 8, torch.float32, None),
    (300, 48, 8, torch.float32, slice(1, 41)),               # misaligned column slice
    (300, 48, 8, torch.bfloat16, slice(1, 41))])
@pytest.mark.parametrize("metric", C.METRICS[::2])
def test_join_kernel_equals_the_torch_path(n, d, S, dtype, view, metric):
    x = C.integer_rows(n, d, n + d, dtype)
    gx = x.cuda()
    if view is not None:
        x, gx = x[:, view].contiguous(), gx[:, view]
        assert not gx.is_contiguous()
    new, old = N.random_samples(n, 40, S, d)
    norms = row_sqnorms(x)
    ref = local_join(x, norms, new, old, metric)
    got = local_join(gx, norms.cuda(), new.cuda(), old.cuda(), metric, engine="kernel")
    assert equal(got, ref), (got, ref)


@pytest.mark.parametrize("K", [8, 33, 256])
def test_merge_kernel_equals_the_torch_path(K):
    # row 0 is the zero row among rows of +-4: the nearest of almost every row, a hub
    g = torch.Generator().manual_seed(7)
    x = (torch.randint(0, 2, (700, 20), generator=g) * 8 - 4).float()
    x[0] = 0
    lists, _, _, (tgt, cid, val) = N.torch_rounds(x, K, 8, 2)
    tgt = torch.where(tgt == 5, -1, tgt)                     # a target with no triples
    assert int((tgt == 0).sum()) > 512 - K                   # more than one chunk of the kernel
    assert bool((cid.long().unsqueeze(2) == lists[1][tgt.long().clamp(min=0)]).any())  # relisted
    *ref, ref_updates = merge_candidates(*lists, tgt, cid, val)
    *got, updates = merge_candidates(*(t.cuda() for t in (*lists, tgt, cid, val)), engine="kernel")
    assert equal(got, ref) and updates == ref_updates, (got, ref)
    assert all(torch.equal(a[5], b[5]) for a, b in zip(ref, lists))


@pytest.mark.parametrize("n,d,K,S", [(300, 20, 8, 4), (1000, 128, 32, 32), (20, 8, 32, 32)])
@pytest.mark.parametrize("metric", C.METRICS)
def test_nn_descent_equals_the_torch_path(n, d, K, S, metric):
    assert nn_descent_kernel_serves(d, K, S)
    x = C.integer_rows(n, d, 3 * n)
    ref = nn_descent(x, K, n_samples=S, metric=metric)
    got = nn_descent(x.cuda(), K, n_samples=S, metric=metric, engine="kernel")
    assert equal(got, ref), (got, ref)
    assert bool((ref[1][:, n - 1:] == -1).all()) and bool((ref[1][:, 0] >= 0).all())


def test_nn_descent_in_several_node_chunks():
    x = C.integer_rows(1000, 128, 3000)
    res = Resources(torch.device("cuda", 0))
    res.set_workspace_limit(2 << 20)                         # 113 nodes of 6 * 32 triples
    got = nn_descent(x.cuda(), 32, engine="kernel", res=res)
    assert equal(got, nn_descent(x, 32))


@pytest.mark.parametrize("dtype,floor", [(torch.float32, 0.8764), (torch.bfloat16, 0.8762)])
def test_real_values(dtype, floor):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2000, 96, generator=g).to(dtype)
    dists, ids = (t.cpu() for t in nn_descent(x.cuda(), 32, engine="kernel"))
    N.check_invariants(dists, ids, 32)
    exact = ((x[ids].double() - x.double().unsqueeze(1)) ** 2).sum(dim=2)
    assert bool(((dists.double() - exact).abs() <= (96 + 8) * U * exact).all())
    # floor: the recall of the torch path on this input, measured on the CPU. The margin of
    # 0.02 is for one-slice bf16 selection (SPLIT_BOUND[1]) swapping near-tied candidates
    # inside a join: the final exact re-rank cannot bring back an id never inserted.
    got = N.recall(ids, x, 32)
    print(f"recall {got:.4f}, torch path {floor}")
    assert got >= floor - 0.02


@pytest.mark.parametrize("d,k", [(8, 257), (4097, 8)])
def test_beyond_the_kernel_auto_takes_the_torch_path(d, k):
    assert not nn_descent_kernel_serves(d, k, 32)
    x = C.integer_rows(300, d, 9)
    assert equal(nn_descent(x.cuda(), k, max_iterations=3), nn_descent(x, k, max_iterations=3))
    with pytest.raises(ValueError):
        nn_descent(x.cuda(), k, engine="kernel")
