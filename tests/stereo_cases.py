"""Shared by the CPU and the GPU tests of stereo depth (no test itself): the synthetic pairs, and the NumPy mirror's result
for a pair, computed once per session and handed out read-only."""
import functools

import numpy as np

from monogs_amd import stereo_depth as SD

D = SD.NUM_DISPARITIES


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def planes_pair(H=56, W=176, seed=0, split_x=120):
    """The right image is uniform uint8 noise and left[y,x] = right[y, x - d(y,x)] with d piecewise constant: {9, 23}
    over {23, 40}, in four blocks split at x = split_x and y = H // 2.  Returns (left, right, d)."""
    canvas = noise(H, W + D, seed)                                     # the right image with D more columns to its left
    d = np.where(np.arange(W)[None, :] < split_x, 9, 23) * np.ones((H, 1), np.int64)
    d[H // 2:] = np.where(np.arange(W) < split_x, 23, 40)
    ys, xs = np.mgrid[0:H, 0:W]
    left = canvas[ys, xs - d + D]
    return np.ascontiguousarray(left), np.ascontiguousarray(canvas[:, D:]), d


def planes_interior(d):
    """Pixels with x - 11 >= 64, x + 11 <= W - 1 and a 23x23 neighbourhood (cut at the image's top and bottom) of one d."""
    H, W = d.shape
    inside = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(D + 11, W - 11):
            blk = d[max(y - 11, 0):min(y + 11, H - 1) + 1, x - 11:x + 12]
            inside[y, x] = (blk == d[y, x]).all()
    return inside


def ramp_pair(H=37, W=203, seed=5):
    """Noise (smoothed along x, so that half a pixel of shift is not a new image) seen through a slanted disparity ramp,
    linearly interpolated, with a nearer rectangle in front of it: sub-pixel disparities, occlusions at the rectangle's
    sides, and both uniqueness and left-right failures.  Returns (left, right)."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (H, W + D + 2)).astype(np.float64)
    canvas = (raw[:, :-2] + 2 * raw[:, 1:-1] + raw[:, 2:]) / 4.0
    ys, xs = np.mgrid[0:H, 0:W]
    d = 6.0 + 22.0 * xs / W + 0.15 * ys
    d[8:30, 110:150] += 17.0                                            # the nearer rectangle
    src = xs - d + D
    x0 = np.floor(src).astype(np.int64)
    a = src - x0
    left = (1 - a) * canvas[ys, x0] + a * canvas[ys, x0 + 1]
    q = lambda img: np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return q(left), q(canvas[:, D:D + W])


@functools.lru_cache(maxsize=None)
def pair(name, H=None, W=None):
    """(left, right) uint8, read-only: "planes", "ramp", or "noise" at H x W (two unrelated images)."""
    if name == "planes":
        out = planes_pair()[:2]
    elif name == "ramp":
        out = ramp_pair() if H is None else ramp_pair(H, W)
    elif name == "noise":
        out = noise(H, W, 11), noise(H, W, 12)
    else:
        raise KeyError(name)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mirror(name, H=None, W=None):
    """stereo_sgbm_numpy(..., return_flags=True) of `pair(name, H, W)`: (disp16, depth, not_unique, failed_left_right),
    computed once and read-only."""
    out = SD.stereo_sgbm_numpy(*pair(name, H, W), return_flags=True)
    for a in out:
        a.setflags(write=False)
    return out
