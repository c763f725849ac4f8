"""Helpers shared by tests/test_cpu_frame_remap.py and tests/test_gpu_frame_remap.py: the test calibration (fr1_desk's
five coefficients with the intrinsics scaled to the image), tap coverage, the shift case and its hand arithmetic."""
import numpy as np
import torch

from monogs_amd import frame_prepare as FP

FR1_DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)             # configs/mono/tum/fr1_desk.yaml: k1 k2 p1 p2 k3
SHIFT = (5.25, 2.5)                                                # new_K's principal point against K's, in pixels


def calibration_for(H, W, dist=FR1_DIST, distorted=True):
    c = {"fx": 517.3 * W / 640, "fy": 516.5 * H / 480, "cx": 318.6 * W / 640, "cy": 255.3 * H / 480,
         "width": W, "height": H, "distorted": distorted}
    c.update(dict(zip(FP.DIST_KEYS, dist)))
    return c


def intrinsics(cal):
    return tuple(cal[k] for k in ("fx", "fy", "cx", "cy"))


def camera_matrix(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def distorted_map(H, W):
    """(ir, map) of the test calibration, R = I and new_K = K, asserted to have destination pixels with no tap inside
    the image and pixels with only some of them inside: the border code cannot go untested unnoticed."""
    cal = calibration_for(H, W)
    ir, m = FP.remap_build_numpy(H, W, intrinsics(cal), FR1_DIST)
    none, partly = coverage(m)
    assert partly.any(), f"{H}x{W}: no destination pixel straddles the border"
    if (H, W) != (2, 2):       # (at 2x2 every tap pair (sy, sy + 1) holds a row of the image: all four pixels straddle)
        assert none.any(), f"{H}x{W}: no destination pixel has all its taps outside"
    return ir, m


def coverage(m):
    """(no tap inside, some but not all taps inside) per destination pixel of an int32 [H,W,2] map."""
    H, W = m.shape[:2]
    sx, sy = m[..., 0].astype(np.int64) >> 5, m[..., 1].astype(np.int64) >> 5
    n = sum(((sy + dy >= 0) & (sy + dy < H) & (sx + dx >= 0) & (sx + dx < W)).astype(int)
            for dy in (0, 1) for dx in (0, 1))
    return n == 0, (n > 0) & (n < 4)


def shift_case(H=45, W=70):
    """K with fx = fy = 64 (an exact inverse), new_K's principal point moved by SHIFT: (K, new_K)."""
    K = camera_matrix(64.0, 64.0, 35.0, 22.0)
    new_K = camera_matrix(64.0, 64.0, 35.0 + SHIFT[0], 22.0 + SHIFT[1])
    return K, new_K


def shift_by_hand(image):
    """The shift case's output written out: source position (u - 5.25, v - 2.5), i.e. taps at columns u - 6, u - 5 with
    weights 8, 24 and rows v - 3, v - 2 with weights 16, 16, over a zero-padded copy of the source."""
    if image.dtype == torch.uint8:
        H, W = image.shape[:2]
        z = torch.zeros(H + 3, W + 6, 3, dtype=torch.int64)
        z[3:, 6:] = image.to(torch.int64)
        a, b, c, d = z[:H, :W], z[:H, 1:W + 1], z[1:H + 1, :W], z[1:H + 1, 1:W + 1]
        return ((8 * 16 * a + 24 * 16 * b + 8 * 16 * c + 24 * 16 * d + 512) >> 10).to(torch.uint8)
    H, W = image.shape[1:]
    z = torch.zeros(3, H + 3, W + 6)
    z[:, 3:, 6:] = image
    a, b, c, d = z[:, :H, :W], z[:, :H, 1:W + 1], z[:, 1:H + 1, :W], z[:, 1:H + 1, 1:W + 1]
    f = lambda w: torch.tensor(float(w)) / 1024
    return (f(8 * 16) * a + f(24 * 16) * b) + (f(8 * 16) * c + f(24 * 16) * d)


def shift_depth_by_hand(depth):
    """Depth mode 1 on the shift map: ix = 32u - 168 -> column (32u - 152) >> 5 = u - 5 (the .25 rounds down: the source
    x is u - 5.25); iy = 32v - 80 -> row (32v - 64) >> 5 = v - 2 (the .5 of v - 2.5 rounds up); 0 outside."""
    H, W = depth.shape
    out = torch.zeros_like(depth)
    out[2:, 5:] = depth[:H - 2, :W - 5]
    return out


def make_image(H, W, seed, quantised=False):
    """tests/test_gpu_frame_prepare.make_image's recipe: noise over a slow ramp with a corner of exact zeros and a strip
    too dark for the validity test: float [3,H,W] on the CPU, or uint8 [H,W,3]."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H)[:, None]
    img = (0.15 + 0.3 * y + 0.5 * torch.rand(3, H, W, generator=g)).clamp(0.05, 0.95)
    if H >= 16 and W >= 16:
        img[:, :H // 4, :W // 5] = 0.0
        img[:, H // 2:H // 2 + 2, W // 3:W // 3 + 5] = 1.0 / 255.0
    if quantised:
        return img.mul(255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    return img


def as_case(m, H, W, dataset_type, edge_threshold, name):
    """A mirror result in the shape of a fixture case, for test_cpu_frame_prepare.compare (as
    tests/test_gpu_frame_prepare.as_case), with the band cap asserted on the input."""
    from test_cpu_frame_prepare import BAND_CAP, BAND_REL, fixture_threshold
    u8 = lambda k: m[k].reshape(H, W).cpu().numpy().astype(np.uint8)
    c = {"name": name, "H": H, "W": W, "dataset_type": dataset_type, "edge_threshold": float(edge_threshold),
         "intensity": m["intensity"].cpu().numpy(), "median": m["median"].cpu().numpy(), "image_u8": None,
         "gt_depth": None if m["gt_depth"] is None else m["gt_depth"][0].cpu().numpy(), "grad_mask": u8("grad_mask"),
         "rgb_pixel_mask": u8("rgb_pixel_mask"), "rgb_pixel_mask_mapping": u8("rgb_pixel_mask_mapping")}
    want_i, thr = torch.from_numpy(c["intensity"]), fixture_threshold(c)
    band = torch.isfinite(thr) & (thr > 0) & ((want_i - thr).abs() <= BAND_REL * thr)
    assert int(band.sum()) <= BAND_CAP * H * W, "the test image itself puts too many pixels on the threshold"
    return c
