"""Pixel-sampled first-order tracking against the dense first-order iteration on the GPU box:

    python profiles/sampled_tracking_profile.py

Times native first-order tracking iterations (NativeTracker.step) with the dense gradient and with the pixel-sampled
gradient for K in {300, 4096, 16384}, in the same run, at 300 k Gaussians and 640x480 and at the Replica shape
(1200x680, 300 k), by device events after warm-up, and the kernels of the dense and the K = 4096 iteration by the
library's per-kernel timer.  The pose offset is large and the convergence threshold 0, so every timed iteration
does full work.  Prints one line per shape and, last, one JSON line with everything."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import synthetic as S  # noqa: E402
from monogs_amd.gaussian_renderer import render  # noqa: E402
from monogs_amd.pose import SE3_exp  # noqa: E402
from monogs_amd.slam_loops import GaussianParams, Pipe, ViewCamera  # noqa: E402
from monogs_amd.tracking_native import NativeTracker  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "profiles"))
from rgbd_tracking_profile import device_time_us, kernels_us  # noqa: E402

KS = (300, 4096, 16384)


def shape_profile(dev, N, W, H):
    sc = S.make_scene(N, W, H, 4)
    gauss = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev), sc.opacity_logit.to(dev),
                           sc.features_dc.to(dev))
    cam = sc.cam
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    bg = torch.zeros(3, device=dev)
    view = lambda uid, T: ViewCamera(uid, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, dev)
    with torch.no_grad():
        target = render(view(0, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.03, -0.02, 0.04, 0.006, -0.008, 0.004]))
    out = {"gaussians": N, "W": W, "H": H}
    for K in (-1,) + KS:
        v = view(1, T0)
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, H, W)
        trk = NativeTracker(v, gauss, bg, converged_threshold=0.0, num_pixels=K, sample_seed=1)
        t = device_time_us(trk.step, 20, 100)
        ok = trk.check_capacity()
        name = "dense" if K < 0 else f"K{K}"
        out[name] = {"first_order_us": round(t, 1), "capacity_ok": ok}
        if K in (-1, 4096):
            out[name]["kernels_us"] = kernels_us(trk.step, 20)
    for K in KS:
        out[f"K{K}"]["ratio_to_dense"] = round(out[f"K{K}"]["first_order_us"] / out["dense"]["first_order_us"], 3)
    print(f"{N} Gaussians @ {W}x{H}: dense {out['dense']['first_order_us']} us; " +
          ", ".join(f"K={K} {out[f'K{K}']['first_order_us']} us (x{out[f'K{K}']['ratio_to_dense']})" for K in KS))
    return out


def main():
    dev = torch.device("cuda:0")
    res = [shape_profile(dev, 300_000, 640, 480), shape_profile(dev, 300_000, 1200, 680)]
    print(json.dumps({"sampled_tracking_profile": res}))


if __name__ == "__main__":
    main()
