"""Golden vectors for frame preparation, produced by RUNNING the reference's own Python on the CPU (build container only;
the reference tree does not exist on the GPU box):

    python tests/golden/make_frame_prepare_golden.py      ->  tests/golden/frame_prepare_ref.npz

What is run (nothing of it is copied; only arrays - inputs and what the reference left behind - are stored):
  * utils/camera_utils.py: Camera.compute_grad_mask (:110-147), called unbound on a SimpleNamespace `self` holding
    original_image, depth and device, after utils.configs.cuda_device was set to "cpu";
  * utils/slam_utils.py: image_gradient / image_gradient_mask (:7-41) once more on the same grey image, for the gradient
    intensity and the median(s) compute_grad_mask does not keep.  The generator checks that thresholding that intensity
    by those medians gives back the very mask the reference left.
The quantised cases hand the reference what its dataset would (utils/dataset.py:269-276): image / 255.0 and
depth / depth_scale as NumPy computes them, cast to float32.

For every case the generator asserts what the tests' comparison rule rests on: the edge mask covers between 5 % and
95 % of the image; NO pixel has |grey| within 1e-7 of the validity test's 0.01 or a channel sum within 1e-6 of the
boundary threshold; at most 0.1 % of the pixels have an intensity within 1e-5 (relative) of their threshold
m * edge_threshold - the only place where another rounding order may flip a mask bit.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path[:0] = [REF]
import utils.configs  # noqa: E402

utils.configs.cuda_device = "cpu"
import utils.camera_utils as CU  # noqa: E402
import utils.slam_utils as SU  # noqa: E402

RGB_BOUNDARY_THRESHOLD = 0.01
BAND_REL = 1e-5
BAND_CAP = 1e-3
PATCH = 32


def waves(g, H, W):
    """Sinusoids + noise in [0.05, 0.95]: a spread of gradient strengths."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    chans = []
    for _ in range(3):
        fy, fx, ph = (torch.rand(3, generator=g) * torch.tensor([0.5, 0.5, 6.28])).tolist()
        c = 0.5 + 0.3 * torch.sin(0.15 * y * (1 + fy) + ph) * torch.cos(0.11 * x * (1 + fx)) \
            + 0.06 * torch.randn(H, W, generator=g)
        chans.append(c.clamp(0.05, 0.95))
    return torch.stack(chans)


def coarse_waves(g, H, W):
    """The same on a grid of 6 / 255: after quantisation many pixels share one intensity, the median's among them."""
    return (waves(g, H, W) * (255.0 / 6.0)).round() * (6.0 / 255.0)


def blocks(g, H, W, cell=12):
    """Flat cells with faint noise: sparse strong edges over a weak background (what a threshold of 4 medians needs)."""
    ny, nx = H // cell + 2, W // cell + 2
    chans = []
    for _ in range(3):
        coarse = 0.15 + 0.7 * torch.rand(ny, nx, generator=g)
        c = coarse.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[3:3 + H, 5:5 + W]
        chans.append((c + 0.012 * torch.randn(H, W, generator=g)).clamp(0.05, 0.95))
    return torch.stack(chans)


def darken(img, quantised):
    """A corner of exact zeros, a strip too dark for the validity test whose channel sum still passes the boundary
    threshold, and a strip below both."""
    _, H, W = img.shape
    lo = 1.0 / 255.0 if quantised else 0.004
    img[:, :H // 4, :W // 5] = 0.0
    img[:, H // 2:H // 2 + 3, W // 3:W // 3 + 9] = lo                   # sum 0.0118 / 0.012 > 0.01, grey < 0.01
    img[:, H - 6:H - 3, W // 2:W // 2 + 7] = 0.0
    img[0, H - 6:H - 3, W // 2:W // 2 + 7] = lo                         # sum 0.0039 / 0.004 < 0.01
    return img


# name: (painter, H, W, quantised, dataset type, edge_threshold, depth_scale or None)
CASES = {
    "global_48x80_float": (waves, 48, 80, False, "tum", 1.1, None),
    "global_96x72_u8": (coarse_waves, 96, 72, True, "tum", 1.1, None),
    "patch_70x100_float": (blocks, 70, 100, False, "replica", 4.0, None),
    "patch_70x100_u8": (blocks, 70, 100, True, "replica", 4.0, None),
    "patch_70x100_float_et1p1": (waves, 70, 100, False, "replica", 1.1, None),
    "patch_64x96_u8_et1p1": (waves, 64, 96, True, "replica", 1.1, None),
    "patch_64x96_float_depth": (blocks, 64, 96, False, "replica", 4.0, 6553.5),
    "rgbd_48x64_u8_u16": (waves, 48, 64, True, "tum", 1.1, 5000.0),
}


def run_case(name, spec, g):
    painter, H, W, quantised, dtype, et, depth_scale = spec
    img = darken(painter(g, H, W), quantised)
    res = {"H": np.int32(H), "W": np.int32(W), "edge_threshold": np.float32(et), "patch": np.int32(dtype == "replica")}
    if quantised:
        u8 = img.mul(255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()     # [H,W,3]
        res["image_u8"] = u8
        image = torch.from_numpy(u8 / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).to(dtype=torch.float32)
    else:
        image = img.to(torch.float32).contiguous()
        res["image"] = image.numpy()
    depth = None
    if depth_scale is not None:
        d16 = (torch.rand(H, W, generator=g) * 40000).to(torch.int32)
        d16[torch.rand(H, W, generator=g) < 0.05] = 0
        d16[0, :4] = torch.tensor([0, 1, 65535, 32768], dtype=torch.int32)
        d16 = d16.numpy().astype(np.uint16)
        depth = d16 / depth_scale                                            # float64, as the dataset hands it over
        res["depth_u16"], res["depth_scale"] = d16, np.float64(depth_scale)
    cfg = {"Training": {"edge_threshold": et, "rgb_boundary_threshold": RGB_BOUNDARY_THRESHOLD},
           "Dataset": {"type": dtype}}
    cam = types.SimpleNamespace(original_image=image.clone(), depth=depth, device="cpu")
    CU.Camera.compute_grad_mask(cam, cfg)
    grad = cam.grad_mask.reshape(H, W).to(torch.float32)
    res["grad_mask"] = grad.numpy().astype(np.uint8)
    res["rgb_pixel_mask"] = cam.rgb_pixel_mask.reshape(H, W).to(torch.float32).numpy().astype(np.uint8)
    res["rgb_pixel_mask_mapping"] = cam.rgb_pixel_mask_mapping.reshape(H, W).numpy().astype(np.uint8)
    if depth is not None:
        assert tuple(cam.gt_depth.shape) == (1, H, W) and cam.gt_depth.dtype == torch.float32
        res["gt_depth"] = cam.gt_depth[0].numpy()
    # the intensity and the median(s), through the reference's own stencils
    grey = image.mean(dim=0, keepdim=True)
    gv, gh = SU.image_gradient(grey)
    mv, mh = SU.image_gradient_mask(grey)
    inten = torch.sqrt((gv * mv) ** 2 + (gh * mh) ** 2)[0]
    thr = torch.full((H, W), float("inf"))
    if dtype == "replica":
        ny, nx = H // PATCH, W // PATCH
        rows = inten[:ny * PATCH, :nx * PATCH].reshape(ny, PATCH, nx, PATCH).permute(0, 2, 1, 3).reshape(ny * nx, -1)
        med = rows.median(dim=1).values
        thr[:ny * PATCH, :nx * PATCH] = (med * et).reshape(ny, nx).repeat_interleave(PATCH, 0).repeat_interleave(PATCH, 1)
    else:
        med = inten.median()
        thr[:] = med * et
    assert torch.equal((inten > thr).to(torch.float32), grad), name       # these ARE the reference's medians
    res["intensity"], res["median"] = inten.numpy(), med.numpy().astype(np.float32)
    # what the comparison rule rests on
    cover = float(grad.mean())
    assert 0.05 <= cover <= 0.95, (name, cover)
    near_valid = int(((grey.abs() - 0.01).abs() <= 1e-7).sum())
    near_boundary = int(((image.sum(dim=0) - RGB_BOUNDARY_THRESHOLD).abs() <= 1e-6).sum())
    assert near_valid == 0 and near_boundary == 0, (name, near_valid, near_boundary)
    band = int((((inten - thr).abs() <= BAND_REL * thr) & torch.isfinite(thr)).sum())
    assert band <= BAND_CAP * H * W, (name, band)
    ties = H * W - int(torch.unique(inten).numel())
    print(f"{name:26s} {H}x{W} {dtype:7s} edge_threshold {et}: mask covers {100 * cover:.1f} %, zero intensity "
          f"{int((inten == 0).sum())}, tied values {ties}, in the band {band}, median(s) {float(med.min()):.4g} .. "
          f"{float(med.max()):.4g}")
    return res


def main():
    g = torch.Generator().manual_seed(20261018)
    out = {"names": np.array(list(CASES)), "rgb_boundary_threshold": np.float32(RGB_BOUNDARY_THRESHOLD)}
    for name, spec in CASES.items():
        for k, v in run_case(name, spec, g).items():
            out[f"{name}_{k}"] = v
    path = os.path.join(HERE, "frame_prepare_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
