"""GPU kernels of csrc/pairwise_metrics.hip against the CPU fp64 path:
the register-tiled KL / Jensen-Shannon / Bray-Curtis contraction, the
Haversine kernel and the Hellinger / Russel-Rao / Jaccard / Dice epilogue.
"""
import pytest
import torch

from raft_amd.distance import pairwise_distance, DistanceType

pytestmark = pytest.mark.gpu

UNEXPANDED = ["kl_divergence", "jensenshannon", "braycurtis"]
EXPANDED = ["hellinger", "russelrao", "jaccard", "dice"]
# compared on the squares: the sqrt of a near-zero cancelling sum cannot carry
# an absolute tolerance set for the sum
SQUARED = {"jensenshannon", "hellinger"}
# (1,1,1); 64-tile edge; K-chunk tail + two row tiles; long K with the ragged
# float4 tail of the epilogue (7*5 = 35 outputs)
SHAPES = [(1, 1, 1), (65, 63, 33), (130, 70, 100), (7, 5, 257)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def prob_rows(m, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(m, d, generator=g) + 1e-3
    return x / x.sum(dim=1, keepdim=True)


def binary_rows(m, d, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(m, d, generator=g) < 0.3).to(dtype)
    x[:, 0] = 1
    return x


def latlon_rows(m, seed):
    g = torch.Generator().manual_seed(seed)
    lat = (torch.rand(m, generator=g) - 0.5) * 3.14159
    lon = (torch.rand(m, generator=g) - 0.5) * 6.28318
    return torch.stack([lat, lon], dim=1)


def inputs_for(metric, m, n, d):
    if metric in ("russelrao", "jaccard", "dice"):
        return binary_rows(m, d, 1), binary_rows(n, d, 2)
    if metric == "haversine":
        return latlon_rows(m, 3), latlon_rows(n, 4)
    return prob_rows(m, d, 5), prob_rows(n, d, 6)


def check(metric, got, ref, rtol, atol):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    assert (got >= 0).all()
    if metric in SQUARED:
        got, ref = got * got, ref * ref
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)


@pytest.mark.parametrize("m,n,d", SHAPES)
@pytest.mark.parametrize("metric", UNEXPANDED + EXPANDED)
def test_parity_fp32(dev, metric, m, n, d):
    x, y = inputs_for(metric, m, n, d)
    got = pairwise_distance(x.to(dev), y.to(dev), metric)
    assert got.dtype == torch.float32 and got.is_cuda
    check(metric, got, pairwise_distance(x.double(), y.double(), metric), 1e-4, 1e-4)


def test_parity_haversine(dev):
    x, y = inputs_for("haversine", 65, 63, 2)
    got = pairwise_distance(x.to(dev), y.to(dev), DistanceType.Haversine)
    check("haversine", got, pairwise_distance(x.double(), y.double(), "haversine"),
          1e-4, 1e-4)
    with pytest.raises(ValueError):
        pairwise_distance(torch.rand(4, 3, device=dev), None, "haversine")


def test_zero_and_negative_entries(dev):
    """x <= 0 / a == 0 / zero-denominator conventions on the GPU, on a shape
    with a K tail so that zero-filled lanes take part."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand(9, 21, generator=g)
    y = torch.rand(6, 21, generator=g)
    x[x < 0.3] = 0.0
    y[y < 0.3] = 0.0
    x[0] = 0.0
    y[0] = 0.0
    x[1, :5] = -1.0
    for metric in UNEXPANDED + ["hellinger", "jaccard", "dice"]:
        got = pairwise_distance(x.to(dev), y.to(dev), metric)
        ref = pairwise_distance(x.double(), y.double(), metric)
        if metric == "kl_divergence":  # may be negative on unnormalised rows
            torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-4, atol=1e-4)
        else:
            check(metric, got, ref, 1e-4, 1e-4)


def test_self_distance(dev):
    x = prob_rows(70, 40, 8).to(dev)
    # exact by construction of the Jensen-Shannon and Bray-Curtis kernels
    assert pairwise_distance(x, x, "jensenshannon").diagonal().abs().max() == 0.0
    assert pairwise_distance(x, x, "braycurtis").diagonal().abs().max() == 0.0
    assert pairwise_distance(x, x, "kl_divergence").diagonal().abs().max() < 1e-4


@pytest.mark.parametrize("metric", EXPANDED)
def test_emulated_gemm(dev, metric):
    x, y = inputs_for(metric, 130, 70, 128)
    got = pairwise_distance(x.to(dev), y.to(dev), metric, fp32_mode="bf16x3")
    check(metric, got, pairwise_distance(x.double(), y.double(), metric), 5e-3, 5e-3)


@pytest.mark.parametrize("metric", ["jaccard", "dice", "russelrao"])
def test_bf16_binary_inputs(dev, metric):
    # 0/1 entries and counts <= 96 are exact in bf16 and fp32: only the
    # epilogue division rounds
    x = binary_rows(65, 96, 9, torch.bfloat16)
    y = binary_rows(63, 96, 10, torch.bfloat16)
    got = pairwise_distance(x.to(dev), y.to(dev), metric)
    assert got.dtype == torch.float32
    ref = pairwise_distance(x.double(), y.double(), metric)
    torch.testing.assert_close(got.double().cpu(), ref, rtol=0, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_inputs_widen(dev, dtype):
    x = prob_rows(33, 20, 11).to(dtype)
    y = prob_rows(17, 20, 12).to(dtype)
    for metric in ("braycurtis", "hellinger"):
        got = pairwise_distance(x.to(dev), y.to(dev), metric)
        assert got.dtype == torch.float32
        # the reference sees the same rounded rows
        check(metric, got, pairwise_distance(x.double(), y.double(), metric), 1e-4, 1e-4)


@pytest.mark.parametrize("metric", ["kl_divergence", "jensenshannon", "russelrao"])
def test_no_mnd_materialisation(dev, metric):
    m = n = 512
    d = 64
    x, y = inputs_for(metric, m, n, d)
    x, y = x.to(dev), y.to(dev)
    pairwise_distance(x, y, metric)  # library handles / workspaces exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = pairwise_distance(x, y, metric)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    assert out.shape == (m, n)
    assert extra <= 3 * m * n * 4 + 8 * (m + n) * d * 4, extra


@pytest.mark.parametrize("metric", ["braycurtis", "jaccard"])
def test_output_index_past_2_31(dev, metric):
    """m * n > 2^31 outputs (d = 1 keeps it cheap): the tiled kernel and the
    flat float4 epilogue must index in 64 bits. The last rows sit past 2^31."""
    m = n = 46400
    assert m * n > 2 ** 31
    g = torch.Generator().manual_seed(16)
    x = torch.rand(m, 1, generator=g) + 0.5
    y = torch.rand(n, 1, generator=g) + 0.5
    got = pairwise_distance(x.to(dev), y.to(dev), metric)
    assert got.shape == (m, n)
    for rows in (slice(0, 3), slice(m - 3, m)):
        ref = pairwise_distance(x[rows].double(), y.double(), metric)
        torch.testing.assert_close(got[rows].double().cpu(), ref, rtol=1e-4, atol=1e-4)
    del got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("metric", ["jensenshannon", "braycurtis"])
def test_knn(dev, metric):
    from raft_amd.neighbors.brute_force import knn
    x, q = prob_rows(300, 33, 13), prob_rows(40, 33, 14)
    d_gpu, i_gpu = knn(x.to(dev), q.to(dev), 5, metric=metric)
    d_cpu, _ = knn(x, q, 5, metric=metric)
    true = pairwise_distance(q.double(), x.double(), metric)
    got, ref = d_gpu.double().cpu(), d_cpu.double()
    gathered = true.gather(1, i_gpu.cpu())
    if metric in SQUARED:
        got, ref, gathered = got * got, ref * ref, gathered * gathered
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)
    # tie-tolerant: the true distances at the returned indices reproduce them
    torch.testing.assert_close(gathered, got, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("metric,p", [("l1", 2.0), ("linf", 2.0), ("lp", 3.0),
                                      ("canberra", 2.0), ("hamming", 2.0)])
def test_existing_codes_not_rerouted(dev, metric, p):
    g = torch.Generator().manual_seed(15)
    x = torch.randn(65, 33, generator=g)
    y = torch.randn(63, 33, generator=g)
    if metric == "hamming":
        x, y = x.round(), y.round()
    got = pairwise_distance(x.to(dev), y.to(dev), metric, p=p).double().cpu()
    if metric in ("l1", "linf", "lp"):
        ref = torch.cdist(x.double(), y.double(),
                          p={"l1": 1.0, "linf": float("inf"), "lp": 3.0}[metric])
    else:
        ref = pairwise_distance(x.double(), y.double(), metric, p=p)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)
