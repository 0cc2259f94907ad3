"""Cases of the 4-bit IVF-PQ tests (CPU and GPU). The fp64 oracle, acceptance
rules, tolerances and input generators are those of tests/ivf_pq_inputs.py,
which are book-size agnostic; the 16-entry books are the first 16 entries of
its 256."""
import struct

import pytest
import torch

import ivf_pq_inputs as I
from raft_amd.core.bitset import Bitset
from raft_amd.core.resources import Resources
from raft_amd.neighbors import (IvfPqParams, ivf_pq_build, ivf_pq_extend, ivf_pq_load,
                                ivf_pq_save, ivf_pq_search, refine)

#: (d, pq_dim): pq_len 3 with d_rot > d; a pad nibble in a live byte; one chunk;
#: a second chunk with one live byte; pq_len 32; eight chunks (2 queries a
#: block); pq_len 32 with the largest residuals at 8 queries a block; then the
#: two remaining group sizes: 4 queries a block, and 1 (16 + 17 KiB a query)
SHAPES = ((10, 4), (7, 7), (32, 32), (33, 33), (96, 3), (256, 256), (1024, 32),
          (128, 128), (4352, 256))
_search = I._search


def forced_index(device, metric, d, pq_dim, **kw):
    f = I.forced_data(d, pq_dim, **kw)
    f.books = f.books[..., :16].contiguous()
    index = ivf_pq_build(f.x.to(device), IvfPqParams(metric=metric),
                         centroids=f.centroids.to(device), codebooks=f.books.to(device))
    assert (index.pq_bits, index.book_size) == (4, 16)
    assert index.row_bytes == -(-(-(-pq_dim // 2)) // 16) * 16
    assert index.codes.numel() == index.indices.numel() * index.row_bytes
    assert index.kernels_serve == (device == "cuda" and pq_dim <= 256)
    return f, index


def case_search(device, metric, d, pq_dim):
    """Forced list sizes, 33 queries; n_probes 1, 3, all; k beyond a query's
    candidates; a probe of the empty list."""
    f, index = forced_index(device, metric, d, pq_dim)
    assert index.list_sizes.tolist() == list(I.FORCED_SIZES)
    for n_probes, k in ((1, 5), (3, 70), (len(I.FORCED_SIZES), 400)):
        dd, ii, pp = _search(index, f.q, k, n_probes)
        assert dd.device.type == device and tuple(pp.shape) == (f.q.shape[0], n_probes)
        I.check(index, f.q, pp, dd, ii, k)
    probes = torch.zeros((3, 1), dtype=torch.int64, device=device)
    dd, ii, pp = _search(index, f.q[:3], 2, 1, probes=probes)
    assert bool((ii == -1).all()) and bool(torch.isinf(dd).all())


def case_long_list(device, metric):
    """One query on one 1000-row list: the scan's grid y is 4."""
    f, index = forced_index(device, metric, 20, 5, n_lists=2, sizes=(1000, 0), nq=1)
    dd, ii, pp = _search(index, f.q, 7, 1)
    assert pp.tolist() == [[0]] and index.list_sizes.tolist() == [1000, 0]
    I.check(index, f.q, pp, dd, ii, 7)


def case_filter(device, metric):
    f, index = forced_index(device, metric, 10, 4)
    mask = torch.rand(f.x.shape[0], generator=torch.Generator().manual_seed(3)) < 0.5
    d1, i1, p1 = _search(index, f.q, 9, 3, filter=mask.to(device))
    I.check(index, f.q, p1, d1, i1, 9, mask=mask)
    d2, i2, _ = _search(index, f.q, 9, 3, filter=Bitset.from_dense(mask.to(device)))
    assert torch.equal(i1, i2) and torch.equal(d1, d2)


def case_chunking(device, metric):
    """Two workspace budgets (all queries at once, 4 per chunk) group a list's
    queries differently: bitwise equal."""
    f, index = forced_index(device, metric, 33, 33)
    d0, i0, p0 = _search(index, f.q, 9, 3)
    res = Resources(torch.device(device))
    res.set_workspace_limit(2 * 4 * 4 * 3 * index.max_list_pad)
    d1, i1, p1 = _search(index, f.q, 9, 3, res=res)
    assert torch.equal(p0, p1) and torch.equal(d0, d1) and torch.equal(i0, i1)


def case_encode(device, pq_len, pq_dim=3, n=300):
    """Rows 100.. are exactly centroid + entry; entry 12 repeats entry 5."""
    d = pq_dim * pq_len - (pq_len > 1)                  # the last feature is padding
    g = torch.Generator().manual_seed(40 + pq_len)
    books = 0.5 * torch.randn(pq_dim, pq_len, 16, generator=g)
    books[:, :, 12] = books[:, :, 5]
    if pq_len > 1:
        books[-1, -1] = 0.0                             # as training on zeros gives
    centroids = torch.zeros(4, d)
    centroids[torch.arange(4), torch.arange(4) % d] = 8.0 * (1 + torch.arange(4) // d)
    label = torch.arange(n) % 4
    want = torch.randint(0, 16, (n, pq_dim), generator=g)
    want[100:110] = 12
    entry = books.permute(0, 2, 1)[torch.arange(pq_dim), want].reshape(n, -1)[:, :d]
    x = centroids[label] + torch.cat([0.3 * torch.randn(100, d, generator=g), entry[100:]])
    want[want == 12] = 5
    index = ivf_pq_build(x.to(device), IvfPqParams(), centroids=centroids.to(device),
                         codebooks=books.to(device))
    assert (index.pq_len, index.pq_bits, index.row_bytes) == (pq_len, 4, 16)
    codes, got_label = I.codes_by_id(index)
    assert torch.equal(got_label, label) and int(codes.max()) < 16
    # 25 rows at a time: up to there check_codes' fp64 cdist is the direct sum,
    # beyond it the matmul expansion, whose cancellation error (1e-14 absolute)
    # tells the repeated entry from its twin on rows at distance 0
    for s in range(0, n, 25):
        I.check_codes(index, x[s:s + 25], codes[s:s + 25], label[s:s + 25])
    assert torch.equal(codes[100:].long(), want[100:])
    pad = index.to("cpu")._padded_codes()               # 3 nibbles live in 16 bytes
    assert bool((pad[:, 2:] == 0).all()) and bool((pad[:, 1] < 16).all())
    return codes


def case_layout(device):
    """Every stored byte at the documented address is lo | hi << 4 of
    unpack_list's codes (odd pq_dim, two chunks, several groups)."""
    _, index = forced_index(device, "sqeuclidean", 33, 33)
    index = index.to("cpu")
    t = torch.arange(index.row_bytes)
    for l in range(index.n_lists):
        codes, _ = index.unpack_list(l)
        even = torch.zeros(codes.shape[0], 2 * index.row_bytes, dtype=torch.uint8)
        even[:, :index.pq_dim] = codes
        slot = int(index.list_offsets[l]) + torch.arange(codes.shape[0])[:, None]
        at = ((slot // 64 * (index.row_bytes // 16) + t // 16) * 64 + slot % 64) * 16 + t % 16
        assert torch.equal(index.codes[at], even[:, 0::2] | (even[:, 1::2] << 4))


def case_end_to_end(device, path):
    """Training, extend, save / load, reconstruct_list, refine: 2000 x 16 blobs,
    pq_bits 4, pq_dim 16, n_lists 8."""
    b = I.blobs()
    x = b.x.to(device)
    params = IvfPqParams(n_lists=8, pq_dim=16, metric="euclidean", pq_bits=4)
    first = ivf_pq_build(x[:1500], params)
    index = ivf_pq_extend(first, x[1500:])
    assert tuple(index.codebooks.shape) == (16, 1, 16) and index.row_bytes == 16
    assert (first.n_rows, index.n_rows, int(index.list_sizes.sum())) == (1500, 2000, 2000)
    old, _ = I.codes_by_id(first)
    new, _ = I.codes_by_id(index)
    assert torch.equal(new[:1500], old)                 # old codes are kept
    dd, ii, pp = _search(index, b.q, 10, 3)
    I.check(index, b.q, pp, dd, ii, 10)
    ivf_pq_save(index, path)
    back = ivf_pq_load(path, device=device)
    assert (back.metric, back.dim, back.pq_bits, back.n_rows) == (index.metric, 16, 4, 2000)
    for name in ("centroids", "codebooks", "list_offsets", "list_sizes", "codes", "indices"):
        assert torch.equal(getattr(back, name), getattr(index, name)), name
    d1, i1, p1 = _search(back, b.q, 10, 3)
    assert torch.equal(p1, pp) and torch.equal(i1, ii) and torch.equal(d1, dd)
    err = res = 0.0
    for l in range(index.n_lists):
        rows, ids = index.reconstruct_list(l)
        err += float(((rows - x[ids]) ** 2).sum())
        res += float(((x[ids] - index.centroids[l]) ** 2).sum())
    assert err < res
    # the re-ranked search is refine over the plain search's 2k candidates
    q = b.q.to(device)
    want = refine(x, q, ivf_pq_search(index, q, 20, 3)[1], 10, index.metric)
    got = ivf_pq_search(index, q, 10, 3, dataset=x, refine_ratio=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    raw = bytearray(open(path, "rb").read())
    assert struct.unpack_from("<q", raw, 16) == (2,)
    struct.pack_into("<q", raw, 16, 1)                  # a version-1 header, 16-entry books
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError):
        ivf_pq_load(path)
    with pytest.raises(ValueError):
        ivf_pq_build(x, IvfPqParams(n_lists=8, pq_dim=16, pq_bits=5))
