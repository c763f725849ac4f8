"""bench.py's plain run and --dump-outputs: the headline line alone, the last timed step's outputs written as .npy,
identical inputs from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--gaussians", "20000", "--width", "320", "--height", "240"]


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_last_timed_step(built, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = _bench(SMALL + ["--dump-outputs", str(a)])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 0.01 * 1e3
    for k in ("tracking", "map_update", "mapping", "slam", "knn", "sustained_fps", "value_default_engine"):
        assert k not in out, k
    assert out["roofline"] is None and out["cpu_baseline"] is None
    N, H, W = 20000, 240, 320
    shapes = {"image": (3, H, W), "depth": (1, H, W), "opacity": (1, H, W), "radii": (N,), "n_touched": (N,),
              "loss": (1,), "grad_means3D": (N, 3), "grad_scales": (N, 3), "grad_rotations": (N, 4),
              "grad_opacities": (N, 1), "grad_shs": (N, 1, 3), "grad_means2D": (N, 3), "grad_rho": (3,),
              "grad_theta": (3,)}
    got = {k: np.load(a / f"{k}.npy") for k in shapes}
    assert sorted(os.listdir(a)) == sorted(f"{k}.npy" for k in shapes)
    for k, s in shapes.items():
        assert got[k].shape == s and got[k].dtype in (np.float32, np.float64), k
        assert np.isfinite(got[k]).all(), k
    assert (got["radii"] > 0).sum() > 1000 and np.abs(got["grad_means3D"]).sum() > 0
    assert float(got["loss"][0]) > 0
    # a second run on the same arguments sees the same inputs: the forward is reproduced
    _bench(SMALL + ["--dump-outputs", str(b)])
    for k in ("image", "depth", "opacity", "radii", "n_touched"):
        assert np.allclose(np.load(b / f"{k}.npy"), got[k], rtol=0, atol=1e-6), k
