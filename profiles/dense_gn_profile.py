"""Dense Gauss-Newton iteration against the sketched Levenberg-Marquardt iteration on the GPU box:

    python profiles/dense_gn_profile.py [output file, default profiles/dense_gn_profile.txt]

Times NativeTracker.step_second_order in both modes (exact=False: mgs_tracking_iteration_second_order, the reference
time; exact=True: mgs_tracking_iteration_gauss_newton) in ONE run at three sizes - 300 k Gaussians / 640x480,
8 k / 640x480 and 300 k / 1200x680 - by device events after warm-up, the two modes alternating over several rounds so
that a drift of the box hits both; then the kernels of one iteration of each mode by the library's per-kernel timer
(events around every launch: their sum lacks the gaps between launches and is not the iteration time).  The pose offset
is large and the convergence threshold zero, so no iteration is a no-op.  Writes the table to the output file and
prints it, and last one JSON line with everything."""
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

ROUNDS, WARM, TIMED = 5, 5, 40


def device_time_us(fn, timed):
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
        target = render(view(0, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.03, -0.02, 0.04, 0.006, -0.008, 0.004]))
    trackers = {}
    for mode in ("sketched", "dense"):
        v = view(1, T0)
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, H, W)
        trk = NativeTracker(v, gauss, bg, converged_threshold=0.0)
        # a large lambda keeps the timed iterations near the start pose: the same render load in every round
        trk.enable_second_order(exact=mode == "dense", initial_lambda=1e4, min_lambda=1e4)
        trk.so_args.lm.converged_threshold = 0.0
        for _ in range(WARM):
            trk.step_second_order()
        trackers[mode] = trk
    times = {"sketched": [], "dense": []}
    for _ in range(ROUNDS):
        for mode, trk in trackers.items():
            times[mode].append(device_time_us(trk.step_second_order, TIMED))
    out = {"gaussians": N, "W": W, "H": H}
    for mode, trk in trackers.items():
        t = sorted(times[mode])
        out[mode] = {"iteration_us_median": round(t[len(t) // 2], 1), "iteration_us_min": round(t[0], 1),
                     "iteration_us_max": round(t[-1], 1), "capacity_ok": trk.check_capacity(), "pairs": trk.pairs(),
                     "kernels_us": kernels_us(trk.step_second_order, 10)}
    out["dense_over_sketched"] = round(out["dense"]["iteration_us_median"] / out["sketched"]["iteration_us_median"], 3)
    return out


def table(res):
    lines = ["dense Gauss-Newton iteration vs sketched LM iteration (16 x 64), NativeTracker.step_second_order, monocular",
             f"device events, {ROUNDS} alternating rounds of {TIMED} iterations per mode after {WARM} warm-up iterations; us per iteration",
             ""]
    for r in res:
        s, d = r["sketched"], r["dense"]
        lines.append(f"{r['gaussians']} Gaussians @ {r['W']}x{r['H']} ({s['pairs']} pairs, capacity ok {s['capacity_ok'] and d['capacity_ok']})")
        lines.append(f"  sketched (reference)  median {s['iteration_us_median']:8.1f}   min {s['iteration_us_min']:8.1f}   max {s['iteration_us_max']:8.1f}")
        lines.append(f"  dense                 median {d['iteration_us_median']:8.1f}   min {d['iteration_us_min']:8.1f}   max {d['iteration_us_max']:8.1f}"
                     f"   dense / sketched {r['dense_over_sketched']:.3f}")
        names = sorted(set(s["kernels_us"]) | set(d["kernels_us"]))
        lines.append("  kernel (us per launch, per-kernel timer)      sketched      dense")
        for k in names:
            a, b = s["kernels_us"].get(k), d["kernels_us"].get(k)
            lines.append(f"    {k:40s} {'-' if a is None else format(a, '10.2f'):>10s} {'-' if b is None else format(b, '10.2f'):>10s}")
        lines.append(f"    {'sum of the kernels':40s} {sum(s['kernels_us'].values()):10.2f} {sum(d['kernels_us'].values()):10.2f}")
        lines.append("")
    return "\n".join(lines)


def main():
    dev = torch.device("cuda:0")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dense_gn_profile.txt")
    res = [shape_profile(dev, 300_000, 640, 480), shape_profile(dev, 8_000, 640, 480), shape_profile(dev, 300_000, 1200, 680)]
    text = table(res)
    with open(out_path, "w") as fh:
        fh.write(text + "\n")
    print(text)
    print(json.dumps({"dense_gn_profile": res}))


if __name__ == "__main__":
    main()
