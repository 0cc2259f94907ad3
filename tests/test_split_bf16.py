"""raft_amd.linalg.split_bf16: the split recipe, its reconstruction bounds,
feature padding, and what every op's fp32 mode names resolve to."""
import pathlib
import re

import pytest
import torch

from raft_amd.linalg.split_bf16 import (MODE_NSLICE, SPLIT_BOUND, VERIFY_MODES,
                                        pad_features, row_sqnorms,
                                        split_bf16_slices)

B1, B2, B3 = (2.0 ** -7, 2.0 ** -12), (2.0 ** -13, 2.0 ** -18), (2.0 ** -21, 2.0 ** -24)


def _recipe(t, nslice):
    out, r = [], t
    for _ in range(nslice):
        s = r.to(torch.bfloat16)
        out.append(s)
        r = r - s.float()
    return out


def _inputs():
    g = torch.Generator().manual_seed(11)
    wide = torch.randn(7, 140, generator=g)
    return {"5x64": torch.randn(5, 64, generator=g),
            "3x70": torch.randn(3, 70, generator=g),
            "strided": wide[:, ::2],
            "transposed": torch.randn(64, 6, generator=g).t()}


@pytest.mark.parametrize("nslice", [1, 2, 3])
@pytest.mark.parametrize("name", ["5x64", "3x70", "strided", "transposed"])
def test_split_is_the_recipe(name, nslice):
    t = _inputs()[name]
    assert t.is_contiguous() == (name in ("5x64", "3x70"))
    got = split_bf16_slices(t, nslice)
    want = _recipe(t, nslice)
    assert len(got) == nslice
    for s, w in zip(got, want):
        assert s.dtype == torch.bfloat16 and s.is_contiguous() and s.shape == t.shape
        assert torch.equal(s, w)


def test_the_names_other_modules_keep_are_this_function():
    from raft_amd.linalg.gemm import _split_bf16
    from raft_amd.neighbors.fused_l2nn import split_bf16_slices as reexport
    assert _split_bf16 is split_bf16_slices and reexport is split_bf16_slices


def _bound_inputs():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(64, 128, generator=g)
    return [base, base * 1e-20, base * 1e20,
            torch.arange(2 ** 23, 2 ** 24).float()]   # every 24-bit significand


def test_reconstruction_bounds():
    """bf16 keeps 8 significant bits, unit roundoff 2^-8 (round to nearest):
    one slice leaves |x - s0| <= 2^-8 |x|, the second slice rounds that
    residual the same way, <= 2^-16 |x|, and three slices of 8 bits hold all
    24 bits of an fp32 significand: the sum is x."""
    for x in _bound_inputs():
        xd = x.double()
        mag = xd.abs()
        s = split_bf16_slices(x, 3)
        acc = s[0].double()
        assert bool(((xd - acc).abs() <= 2.0 ** -8 * mag).all())
        acc += s[1].double()
        assert bool(((xd - acc).abs() <= 2.0 ** -16 * mag).all())
        acc += s[2].double()
        assert torch.equal(acc, xd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pad_features(dtype):
    g = torch.Generator().manual_seed(3)
    for d in (64, 128):
        t = torch.randn(4, d, generator=g).to(dtype)
        assert pad_features(t) is t
    for d, dp in ((1, 64), (63, 64), (70, 128), (129, 192)):
        t = torch.randn(4, d, generator=g).to(dtype)
        p = pad_features(t)
        assert p.shape == (4, dp) and p.dtype == dtype and p.is_contiguous()
        assert torch.equal(p[:, :d], t)
        assert bool((p[:, d:] == 0).all())
    t = torch.randn(4, 70, generator=g).to(dtype)
    assert pad_features(t, 32).shape == (4, 96)
    assert pad_features(t, 35) is t


def test_row_sqnorms_cpu():
    x = torch.arange(12.0).reshape(3, 4)
    assert torch.equal(row_sqnorms(x), torch.tensor([14.0, 126.0, 366.0]))
    assert row_sqnorms(x.to(torch.bfloat16)).dtype == torch.float32


def test_tables():
    assert SPLIT_BOUND == {1: B1, 2: B2, 3: B3}
    assert MODE_NSLICE == {"bf16x1v": 1, "bf16x2": 2, "bf16x2v": 2, "bf16x3": 3,
                           "fused": 3, "mfma": 3}
    assert VERIFY_MODES == {"bf16x2v", "bf16x1v", "auto"}


def test_fused_l2nn_modes():
    """(slices, verified, bound of the verify pass) per fp32 mode."""
    from raft_amd.neighbors.fused_l2nn import FUSED_NSLICE
    want = {"bf16x2": (2, False, None), "bf16x3": (3, False, None),
            "fused": (3, False, None), "bf16x2v": (2, True, B2),
            "auto": (2, True, B2), "bf16x1v": (1, True, B1)}
    assert set(FUSED_NSLICE) == set(want)      # "mfma", "native": not fused modes
    for mode, (nslice, verified, bound) in want.items():
        assert FUSED_NSLICE[mode] == nslice
        assert (mode in VERIFY_MODES) == verified
        if verified:
            # fused_l2nn_presplit reads the envelope of its slice count
            assert SPLIT_BOUND[FUSED_NSLICE[mode]] == bound


def test_knn_filter_modes():
    from raft_amd.neighbors.brute_force import _slices_of
    x = torch.randn(8, 64, generator=torch.Generator().manual_seed(1))
    want = {"auto": 1, "bf16x1v": 1, "bf16x3": 3, "bf16x2": 2, "bf16x2v": 2,
            "mfma": 2, "fused": 2}
    for mode, nslice in want.items():
        got = _slices_of(x, mode)
        assert len(got) == nslice
        assert all(torch.equal(a, b) for a, b in zip(got, _recipe(x, nslice)))
    # bf16 rows are their own single slice, whatever the mode
    xb = x.to(torch.bfloat16)
    assert [s.data_ptr() for s in _slices_of(xb, "bf16x3")] == [xb.data_ptr()]


def test_eps_and_masked_modes():
    from raft_amd.neighbors import epsilon_neighborhood, masked_nn
    want = {"auto": (2, B2), "bf16x2v": (2, B2), "bf16x1v": (1, B1)}
    for mod in (epsilon_neighborhood, masked_nn):
        assert set(mod._FP32_MODES) == set(want) | {"native"}
        for mode, (nslice, bound) in want.items():
            resolved = mod._AUTO_MODE if mode == "auto" else mode
            assert resolved in VERIFY_MODES
            assert MODE_NSLICE[resolved] == nslice
            assert SPLIT_BOUND[MODE_NSLICE[resolved]] == bound


def test_pairwise_modes():
    assert [MODE_NSLICE[m] for m in ("bf16x2", "bf16x3", "mfma")] == [2, 3, 3]


def test_kmeans_auto_starts_on_one_slice():
    from raft_amd.cluster import kmeans
    assert kmeans._AUTO_START_NSLICE == 1


def test_layering():
    """distance/ and linalg/ (L3) import nothing from neighbors/ (L4), and the
    shared module only torch and the extension loader. Checked on the source:
    importing raft_amd loads every subpackage."""
    root = pathlib.Path(__file__).resolve().parent.parent / "raft_amd"
    for sub in ("distance", "linalg"):
        for path in sorted((root / sub).glob("*.py")):
            assert not re.search(r"raft_amd\.neighbors|from \.\.neighbors|from \.\. import neighbors",
                                 path.read_text()), path
    src = (root / "linalg" / "split_bf16.py").read_text()
    imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, flags=re.M)
    assert set(imports) == {"__future__", "torch", "raft_amd._ext"}
