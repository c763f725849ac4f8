"""RGB-D tracking against monocular tracking on the GPU box:

    python profiles/rgbd_tracking_profile.py

Times native first- and second-order tracking iterations (NativeTracker.step / step_second_order) with and without
the stacked depth row, in the same run, at 300 k Gaussians and 640x480 and at the Replica shape (1200x680, 300 k), by
device events after warm-up, and the blend / residual kernels alone by the library's per-kernel timer.  The pose
offset is large enough that no iteration converges inside the timed window.  Prints one line per shape and, last,
one JSON line with everything."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import _cabi, synthetic as S  # noqa: E402
from monogs_amd.gaussian_renderer import render  # noqa: E402
from monogs_amd.pose import SE3_exp  # noqa: E402
from monogs_amd.slam_loops import GaussianParams, Pipe, ViewCamera  # noqa: E402
from monogs_amd.tracking_native import NativeTracker  # noqa: E402


def device_time_us(fn, warm, timed):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(timed):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / timed * 1e3


def kernels_us(fn, reps):
    _cabi.profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    return {k: round(v[0] / v[1] * 1e3, 2) for k, v in p.items()}


def shape_profile(dev, N, W, H):
    sc = S.make_scene(N, W, H, 4)
    gauss = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev), sc.opacity_logit.to(dev),
                           sc.features_dc.to(dev))
    cam = sc.cam
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    bg = torch.zeros(3, device=dev)
    view = lambda uid, T: ViewCamera(uid, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, dev)
    with torch.no_grad():
        pkg = render(view(0, torch.eye(4)), gauss, Pipe, bg)
    target, depth = pkg["render"].clone(), pkg["depth"].clone()
    T0 = SE3_exp(torch.tensor([0.03, -0.02, 0.04, 0.006, -0.008, 0.004]))
    out = {"gaussians": N, "W": W, "H": H}
    for mode in ("mono", "rgbd"):
        v = view(1, T0)
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, H, W)
        trk = NativeTracker(v, gauss, bg, converged_threshold=0.0,
                            **({"gt_depth": depth, "alpha": 0.95} if mode == "rgbd" else {}))
        trk.enable_second_order()
        trk.so_args.lm.converged_threshold = 0.0
        fo = device_time_us(trk.step, 20, 100)
        so = device_time_us(trk.step_second_order, 5, 30)
        ok = trk.check_capacity()
        out[mode] = {"first_order_us": round(fo, 1), "second_order_us": round(so, 1), "capacity_ok": ok,
                     "first_order_kernels_us": kernels_us(trk.step, 20),
                     "second_order_kernels_us": kernels_us(trk.step_second_order, 10)}
    out["first_order_ratio"] = round(out["rgbd"]["first_order_us"] / out["mono"]["first_order_us"], 3)
    out["second_order_ratio"] = round(out["rgbd"]["second_order_us"] / out["mono"]["second_order_us"], 3)
    print(f"{N} Gaussians @ {W}x{H}: first order mono {out['mono']['first_order_us']} us, rgbd "
          f"{out['rgbd']['first_order_us']} us (x{out['first_order_ratio']}); second order mono "
          f"{out['mono']['second_order_us']} us, rgbd {out['rgbd']['second_order_us']} us (x{out['second_order_ratio']})")
    return out


def main():
    dev = torch.device("cuda:0")
    res = [shape_profile(dev, 300_000, 640, 480), shape_profile(dev, 300_000, 1200, 680)]
    print(json.dumps({"rgbd_tracking_profile": res}))


if __name__ == "__main__":
    main()
