"""bench.py command-line contract: the JSON result line, --dump-outputs
(what the last timed step returned, reproducible run to run) and --full
(the secondary measurements stay out of a plain run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1",
          "--rows", "3000", "--dim", "16", "--k", "8"]


def _bench(*extra, cuda_visible=None):
    env = dict(os.environ)
    if cuda_visible is not None:
        # hide the GPUs: the CPU tests must take the CPU path on any box
        env["HIP_VISIBLE_DEVICES"] = cuda_visible
        env["CUDA_VISIBLE_DEVICES"] = cuda_visible
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra],
                       cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    return r


def _result(r):
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def _check_line(j, steps):
    assert j["unit"] == "iters/sec" and j["higher_is_better"] is True
    assert j["dtype"] == "fp32" and j["steps"] == steps
    assert j["value"] > 0 and j["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert j["value"] * j["ms_per_step"] == pytest.approx(1000.0, rel=1e-2)


def test_plain_run_dumps_reproducible_outputs(tmp_path):
    """Two plain runs with the same arguments write identical centroids and
    inertia (seeded inputs; the CPU path is deterministic), and the plain
    result line carries none of the --full measurements."""
    outs = []
    for name in ("a", "b"):
        d = tmp_path / name
        j = _result(_bench(*_SMALL, "--dump-outputs", str(d), cuda_visible="-1"))
        _check_line(j, 2)
        assert "pairwise_l2_1Mx128_fp32_gdist_per_s" not in j["config"]
        assert "assign_agreement_vs_native_fp32" not in j["config"]
        assert sorted(os.listdir(d)) == ["centroids.npy", "inertia.npy"]
        c = np.load(d / "centroids.npy")
        i = np.load(d / "inertia.npy")
        assert c.dtype == np.float32 and c.shape == (8, 16)
        assert i.dtype == np.float64 and i.shape == ()
        assert np.isfinite(c).all() and i > 0
        # the dumped inertia is the one the result line reports
        assert float(i) == pytest.approx(j["config"]["inertia"], rel=1e-6)
        outs.append((c, i))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]


def test_check_requires_full():
    r = _bench(*_SMALL, "--check", cuda_visible="-1")
    assert r.returncode == 2
    assert "--full" in r.stderr


@pytest.mark.gpu
def test_full_run_adds_secondary_measurements(tmp_path):
    """--full on the GPU: the headline fields are unchanged and the pairwise
    Gdist/s figure and the --check agreement appear next to them; the native
    kernels' outputs are dumped as well."""
    d = tmp_path / "out"
    j = _result(_bench("--gpus", "1", "--steps", "2", "--warmup", "1",
                       "--rows", "100000", "--dim", "64", "--k", "128",
                       "--full", "--check", "--dump-outputs", str(d)))
    _check_line(j, 2)
    gd = j["config"]["pairwise_l2_1Mx128_fp32_gdist_per_s"]
    assert isinstance(gd, float) and gd > 0, gd
    # the verified engine's argmin is exact fp32 (docs/verified_engines.md);
    # the native engine's expanded form may round a near-tie the other way
    # (3 rows in 200k on tie-heavy random data = 1.5e-5), so
    # allow 1e-4 of the rows, not bitwise equality
    assert j["config"]["assign_agreement_vs_native_fp32"] > 0.9999
    c = np.load(d / "centroids.npy")
    assert c.dtype == np.float32 and c.shape == (128, 64)
    assert np.isfinite(c).all()
    assert np.load(d / "inertia.npy") > 0
