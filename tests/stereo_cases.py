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


def offset_pair(H, W, lift=190, span=66, seed=5):
    """The ramp pair squeezed into `span` grey levels (a * span // 256) with `lift` added to the left image only: the
    brightness offset makes every pixel cost large - the block cost at r = 14 reaches or passes 32 768, see OFFSET_LIFT -
    while the texture keeps the argmin structured.  Returns (left, right), both uint8."""
    assert 0 <= lift and lift + (255 * span) // 256 <= 255
    left, right = (a.astype(np.int64) * span // 256 for a in ramp_pair(H, W, seed))
    return np.ascontiguousarray((left + lift).astype(np.uint8)), np.ascontiguousarray(right.astype(np.uint8))


# offset_pair's lift by pair name.  At 190 EVERY valid entry of C at r = 14 is above 32 767 (37 060 .. 42 393 at the sizes
# tested): the volumes' upper half, but all 64 disparities of a pixel on one side of bit 15.  At 155 and 157 C runs from
# about 30 000 to 35 000 and most pixels have disparities on both sides: 21 % and 78 % of the entries are above at
# 37x203, 29 % and 78 % at 33x129.
OFFSET_LIFT = {"offset": 190, "straddle_low": 155, "straddle_high": 157}


@functools.lru_cache(maxsize=None)
def pair(name, H=None, W=None):
    """(left, right) uint8, read-only: "planes", "ramp", a name of OFFSET_LIFT (`offset_pair` at H x W with that lift),
    or "noise" at H x W (two unrelated images)."""
    if name not in ("planes", "ramp") and (H is None or W is None):
        raise ValueError(f'pair("{name}") needs H and W')
    if name == "planes":
        out = planes_pair()[:2]
    elif name == "ramp":
        out = ramp_pair() if H is None else ramp_pair(H, W)
    elif name in OFFSET_LIFT:
        out = offset_pair(H, W, lift=OFFSET_LIFT[name])
    elif name == "noise":
        out = noise(H, W, 11), noise(H, W, 12)
    else:
        raise KeyError(name)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mirror(name, H=None, W=None, *, blockSize=SD.BLOCK_SIZE, uniquenessRatio=SD.UNIQUENESS_RATIO):
    """stereo_sgbm_numpy(..., return_flags=True) of `pair(name, H, W)` at the block size and uniqueness ratio given:
    (disp16, depth, not_unique, failed_left_right), computed once per setting and read-only."""
    out = SD.stereo_sgbm_numpy(*pair(name, H, W), blockSize=blockSize, uniquenessRatio=uniquenessRatio,
                               return_flags=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mirror_block_cost(name, H=None, W=None, r=SD.BLOCK_SIZE // 2):
    """The mirror's C of `pair(name, H, W)` at half block r: block_cost_numpy(pixel_cost_numpy(L, R), r), int32
    [H,W,64], read-only.  For the preconditions that a test states on the reference side."""
    C_ = SD.block_cost_numpy(SD.pixel_cost_numpy(*pair(name, H, W)), r)
    C_.setflags(write=False)
    return C_
