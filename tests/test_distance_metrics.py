"""KL / Jensen-Shannon / Russel-Rao / Hellinger / Jaccard / Dice / Bray-Curtis /
Haversine on the CPU (fp64) path — the oracle the GPU kernels are held to.

Checked against scipy where scipy has the metric (cdist: jensenshannon,
braycurtis, jaccard, dice, russellrao; special.rel_entr for KL) and against
the written formula otherwise.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist
from scipy.special import rel_entr

from raft_amd.distance import pairwise_distance, DistanceType
from raft_amd.distance.pairwise import _metric_from_str

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 6, 5), (65, 63, 33)]
TOL = dict(rtol=1e-6, atol=1e-8)  # fp64 inputs, as the Minkowski tests


def prob_rows(m, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(m, d, generator=g, dtype=torch.float64) + 1e-3
    return x / x.sum(dim=1, keepdim=True)


def binary_rows(m, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(m, d, generator=g) < 0.3).double()
    x[:, 0] = 1.0  # no empty row
    return x


def _close(d, ref):
    torch.testing.assert_close(d, torch.as_tensor(ref, dtype=torch.float64), **TOL)


@pytest.mark.parametrize("name,member", [
    ("hellinger", "HellingerExpanded"), ("jaccard", "JaccardExpanded"),
    ("dice", "DiceExpanded"), ("braycurtis", "BrayCurtis"),
    ("haversine", "Haversine"), ("kl_divergence", "KLDivergence"),
    ("jensenshannon", "JensenShannon"), ("russelrao", "RusselRaoExpanded")])
def test_string_names_resolve(name, member):
    assert _metric_from_str(name) is getattr(DistanceType, member)
    assert _metric_from_str(member) is getattr(DistanceType, member)


@pytest.mark.parametrize("m,n,d", SHAPES)
class TestAgainstScipy:
    def test_jensenshannon(self, m, n, d):
        x, y = prob_rows(m, d, 1), prob_rows(n, d, 2)
        _close(pairwise_distance(x, y, "jensenshannon"),
               cdist(x.numpy(), y.numpy(), "jensenshannon"))

    def test_braycurtis(self, m, n, d):
        x, y = prob_rows(m, d, 3), prob_rows(n, d, 4)
        _close(pairwise_distance(x, y, "braycurtis"),
               cdist(x.numpy(), y.numpy(), "braycurtis"))

    def test_braycurtis_signed(self, m, n, d):
        g = torch.Generator().manual_seed(5)
        x = torch.randn(m, d, generator=g, dtype=torch.float64)
        y = torch.randn(n, d, generator=g, dtype=torch.float64)
        _close(pairwise_distance(x, y, "braycurtis"),
               cdist(x.numpy(), y.numpy(), "braycurtis"))

    def test_jaccard(self, m, n, d):
        x, y = binary_rows(m, d, 6), binary_rows(n, d, 7)
        _close(pairwise_distance(x, y, "jaccard"),
               cdist(x.numpy().astype(bool), y.numpy().astype(bool), "jaccard"))

    def test_dice(self, m, n, d):
        x, y = binary_rows(m, d, 8), binary_rows(n, d, 9)
        _close(pairwise_distance(x, y, "dice"),
               cdist(x.numpy().astype(bool), y.numpy().astype(bool), "dice"))

    def test_russelrao(self, m, n, d):
        x, y = binary_rows(m, d, 10), binary_rows(n, d, 11)
        _close(pairwise_distance(x, y, "russelrao"),
               cdist(x.numpy().astype(bool), y.numpy().astype(bool), "russellrao"))

    def test_kl_divergence(self, m, n, d):
        x, y = prob_rows(m, d, 12), prob_rows(n, d, 13)
        ref = rel_entr(x.numpy()[:, None, :], y.numpy()[None, :, :]).sum(-1)
        _close(pairwise_distance(x, y, "kl_divergence"), ref)

    def test_hellinger_formula(self, m, n, d):
        x, y = prob_rows(m, d, 14), prob_rows(n, d, 15)
        bc = np.sqrt(x.numpy()[:, None, :] * y.numpy()[None, :, :]).sum(-1)
        _close(pairwise_distance(x, y, "hellinger"),
               np.sqrt(np.maximum(1.0 - bc, 0.0)))

    def test_jaccard_dice_real_valued_formula(self, m, n, d):
        g = torch.Generator().manual_seed(16)
        x = torch.rand(m, d, generator=g, dtype=torch.float64)
        y = torch.rand(n, d, generator=g, dtype=torch.float64)
        dot = (x @ y.t()).numpy()
        nrm = (x * x).sum(1).numpy()[:, None] + (y * y).sum(1).numpy()[None, :]
        _close(pairwise_distance(x, y, "jaccard"), 1.0 - dot / (nrm - dot))
        _close(pairwise_distance(x, y, "dice"), 1.0 - 2.0 * dot / nrm)


def test_haversine_formula():
    g = torch.Generator().manual_seed(17)
    def pts(k):
        lat = (torch.rand(k, generator=g, dtype=torch.float64) - 0.5) * np.pi
        lon = (torch.rand(k, generator=g, dtype=torch.float64) - 0.5) * 2 * np.pi
        return torch.stack([lat, lon], dim=1)
    x, y = pts(65), pts(63)
    xn, yn = x.numpy(), y.numpy()
    dlat = xn[:, None, 0] - yn[None, :, 0]
    dlon = xn[:, None, 1] - yn[None, :, 1]
    h = np.sin(dlat / 2) ** 2 + np.cos(xn[:, None, 0]) * np.cos(yn[None, :, 0]) * np.sin(dlon / 2) ** 2
    _close(pairwise_distance(x, y, "haversine"), 2 * np.arcsin(np.sqrt(np.clip(h, 0, 1))))
    # antipodal pole pair = pi, quarter turn on the equator = pi/2
    p = torch.tensor([[np.pi / 2, 0.0], [-np.pi / 2, 0.0], [0.0, 0.0], [0.0, np.pi / 2]],
                     dtype=torch.float64)
    dd = pairwise_distance(p, p, DistanceType.Haversine)
    _close(dd[0, 1], np.pi)
    _close(dd[2, 3], np.pi / 2)
    # d(x, x) == 0 on the diagonal
    assert pairwise_distance(x, x, "haversine").diagonal().abs().max() == 0.0


def test_haversine_needs_two_columns():
    x = torch.rand(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError):
        pairwise_distance(x, x, "haversine")
    with pytest.raises(ValueError):
        pairwise_distance(x[:, :1], x[:, :1], DistanceType.Haversine)


@pytest.mark.parametrize("metric", ["jaccard", "dice", "braycurtis"])
def test_all_zero_rows_give_zero(metric):
    x = torch.zeros(3, 7, dtype=torch.float64)
    y = torch.zeros(2, 7, dtype=torch.float64)
    d = pairwise_distance(x, y, metric)
    assert d.shape == (3, 2)
    assert (d == 0).all()


def test_degenerate_terms_are_zero_not_nan():
    """KL term is 0 where x == 0; JS term is 0 where a == 0; negative
    entries are clamped to 0 for JS and Hellinger."""
    x = torch.tensor([[0.5, 0.5, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([[0.25, 0.25, 0.5]], dtype=torch.float64)
    kl = pairwise_distance(x, y, "kl_divergence")
    _close(kl, [[np.log(2.0)], [np.log(4.0)]])
    js = pairwise_distance(x, y, "jensenshannon")
    _close(js, cdist(x.numpy(), y.numpy(), "jensenshannon"))
    xneg = torch.tensor([[0.5, 0.5, -3.0]], dtype=torch.float64)
    _close(pairwise_distance(xneg, y, "jensenshannon"),
           pairwise_distance(x[:1], y, "jensenshannon"))
    _close(pairwise_distance(xneg, y, "hellinger"),
           pairwise_distance(x[:1], y, "hellinger"))


def test_self_distance_is_zero():
    x = prob_rows(9, 12, 18)
    for metric in ("kl_divergence", "jensenshannon", "braycurtis"):
        assert pairwise_distance(x, x, metric).diagonal().abs().max() < 1e-12, metric
    assert pairwise_distance(x, x, "hellinger").diagonal().abs().max() < 1e-7
    b = binary_rows(9, 12, 19)
    for metric in ("jaccard", "dice"):
        assert pairwise_distance(b, b, metric).diagonal().abs().max() < 1e-12, metric


def test_fp32_cpu_inputs_keep_dtype():
    x = prob_rows(5, 6, 20).float()
    for metric in ("hellinger", "jaccard", "dice", "braycurtis", "kl_divergence"):
        assert pairwise_distance(x, x, metric).dtype == torch.float32


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_cpp_headers_expose_new_codes(tmp_path):
    src = tmp_path / "metrics_tu.cpp"
    src.write_text(
        "#include <raft_amd/raft_amd.hpp>\n"
        "using namespace raft_amd;\n"
        "void use(device_matrix_view<const float> x, device_matrix_view<float> g,\n"
        "         device_vector_view<const float> xa, device_vector_view<const float> ya) {\n"
        "  for (auto c : {DistanceCode::kKLDivergence, DistanceCode::kJensenShannon,\n"
        "                 DistanceCode::kBrayCurtis, DistanceCode::kHaversine})\n"
        "    pairwise_distance(x, x, g, c);\n"
        "  for (auto c : {ExpandedDistanceCode::kHellinger, ExpandedDistanceCode::kRusselRao,\n"
        "                 ExpandedDistanceCode::kJaccard, ExpandedDistanceCode::kDice})\n"
        "    pairwise_expanded_epilogue(g, xa, ya, c, 8.0f);\n"
        "}\n"
        "static_assert(static_cast<int>(DistanceCode::kHaversine) == 8, \"code\");\n")
    r = subprocess.run(["hipcc", "-fsyntax-only", "--offload-arch=gfx950", "-std=c++17",
                        f"-I{os.path.join(ROOT, 'include')}", str(src)],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
