"""Bitwise Hamming over bit-packed uint8 rows (pairwise, brute-force kNN) and
pack_bits: the xor + popcount kernels on the GPU and the table path on the CPU
against int64 counts from numpy.unpackbits. Both are exact, so distances are
compared bit for bit; only which of several tied rows is returned is left open."""
import numpy as np
import pytest
import torch

from raft_amd.distance import pack_bits, pairwise_distance
from raft_amd.neighbors.brute_force import BruteForceIndex, knn
from test_knn_int8 import check

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
S = 64  # bytes of a row per K step of csrc/pairwise_bits.hip


def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def reference(x, y):
    """[m, n] from int64 sums over the unpacked bits, 16 rows of x at a time."""
    xb = torch.from_numpy(np.unpackbits(x.cpu().numpy(), axis=1)).long()
    yb = torch.from_numpy(np.unpackbits(y.cpu().numpy(), axis=1)).long()
    return torch.cat([(c[:, None, :] != yb[None, :, :]).sum(-1) for c in xb.split(16)]).float()


# one byte; ragged tiles, nbytes no multiple of 4; interior tiles and one K
# step; padded into a second, partial step; three steps, where the double
# buffer wraps
@pytest.mark.parametrize("shape", [(1, 1, 1), (129, 257, 5), (256, 128, S),
                                   (130, 131, S + 1), (128, 128, 3 * S)], ids=str)
@pytest.mark.parametrize("device", DEVICES)
def test_pairwise(device, shape):
    m, n, nbytes = shape
    x, y = rand((m, nbytes), m + nbytes), rand((n, nbytes), n * nbytes)
    out = pairwise_distance(x.to(device), y.to(device), metric="bitwise_hamming")
    assert out.dtype == torch.float32 and out.device.type == device
    assert torch.equal(out.cpu(), reference(x, y))


@pytest.mark.parametrize("nbytes", [5, 3 * S + 1])
@pytest.mark.parametrize("device", DEVICES)
def test_pad_bytes_are_not_counted(device, nbytes):
    ones = torch.full((3, nbytes), 0xFF, dtype=torch.uint8, device=device)
    zeros = torch.zeros((130, nbytes), dtype=torch.uint8, device=device)
    assert bool((pairwise_distance(ones, zeros, metric="bitwise_hamming") == 8 * nbytes).all())
    assert bool((pairwise_distance(ones, ones, metric="bitwise_hamming") == 0).all())


# n = 2000 takes the filter path on the GPU and n = 50 the tiled one
@pytest.mark.parametrize("n, nbytes", [(2000, 16), (50, 16), (2000, 37)])
@pytest.mark.parametrize("device", DEVICES)
def test_knn(device, n, nbytes):
    x, q = rand((n, nbytes), n), rand((130, nbytes), nbytes)
    want = reference(q, x)
    x, q = x.to(device), q.to(device)
    check(*knn(x, q, 10, metric="bitwise_hamming"), want, 10)
    check(*BruteForceIndex(x, metric="bitwise_hamming").search(q, 10), want, 10)


@pytest.mark.parametrize("device", DEVICES)
def test_overflow_fallback(device):
    """20000 identical rows all pass the filter: more than the 16384 slots."""
    x, q = torch.full((20000, 16), 7, dtype=torch.uint8), rand((3, 16), 7)
    dists, ids = knn(x.to(device), q.to(device), 5, metric="bitwise_hamming")
    check(dists, ids, reference(q, x[:1]).expand(3, 20000), 5)


@pytest.mark.parametrize("d", [1, 8, 63, 64, 65, 200])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("device", DEVICES)
def test_pack_bits(device, dtype, d):
    g = torch.Generator().manual_seed(d)
    wide = torch.randn((37, d + 3), generator=g).to(dtype).to(device)
    for x, t in ((wide[:, :d].contiguous(), 0.0), (wide[:, :d], 0.25)):  # and a row-strided view
        want = np.packbits(x.float().cpu().numpy() > t, axis=1, bitorder="little")
        out = pack_bits(x, t)
        assert out.dtype == torch.uint8 and out.device.type == device
        assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("device", DEVICES)
def test_rejections(device):
    x = torch.zeros((100, 16), dtype=torch.uint8, device=device)
    for other in (x.float(), x.to(torch.int8), x[:, :15]):
        with pytest.raises(ValueError):
            pairwise_distance(x, other, metric="bitwise_hamming")
        with pytest.raises(ValueError):
            knn(x, other[:5], 3, metric="bitwise_hamming")
    with pytest.raises(ValueError):
        BruteForceIndex(x.float(), metric="bitwise_hamming")
    wide = torch.zeros((0, 1 << 21), dtype=torch.uint8, device=device)  # 2^24 bits
    with pytest.raises(ValueError):
        pairwise_distance(wide, wide, metric="bitwise_hamming")
