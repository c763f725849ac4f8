"""bench.py's --dump-outputs writer on the CPU: dtypes, and the fixed, seeded sample of the per-Gaussian arrays
that keeps a dump within its 64 MB."""
import os

import numpy as np
import torch

import bench


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_dump_is_written_whole(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"image": torch.rand(3, 8, 10, generator=g), "radii": torch.arange(50, dtype=torch.int32),
              "grad_means3D": torch.randn(50, 3, generator=g), "loss": torch.tensor([0.5])}
    bench.dump_outputs(str(tmp_path), arrays, 50)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in arrays)
    assert np.load(tmp_path / "image.npy").dtype == np.float32
    r = np.load(tmp_path / "radii.npy")
    assert r.dtype == np.float64 and np.array_equal(r, np.arange(50))
    assert np.array_equal(np.load(tmp_path / "grad_means3D.npy"), arrays["grad_means3D"].numpy())


def test_large_dump_keeps_a_fixed_sample_within_the_cap(tmp_path):
    N = 3_000_000
    arrays = {"image": torch.zeros(3, 480, 640), "grad_means3D": torch.arange(3 * N, dtype=torch.float32).reshape(N, 3),
              "grad_rotations": torch.zeros(N, 4), "n_touched": torch.ones(N, dtype=torch.int32)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays, N)
    bench.dump_outputs(str(b), arrays, N)
    assert _sizes(a) <= bench.DUMP_BYTES_MAX
    idx = np.load(a / "gaussian_sample_index.npy")
    assert idx.dtype == np.float64 and len(idx) > N // 10 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(b / "gaussian_sample_index.npy"))
    g = np.load(a / "grad_means3D.npy")
    assert np.array_equal(g[:, 0], (idx * 3).astype(np.float32))
    assert np.load(a / "image.npy").shape == (3, 480, 640)
