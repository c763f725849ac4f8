"""The `--eval` tail (utils/eval_utils.py:114-178) on the GPU box:

    python profiles/eval_profile.py [output file]          # default: profiles/eval_profile.txt

Per-view wall time of eval_native.NativeEvaluator (begin, score x views, finish: ONE synchronisation at the end of the
batch) against the loop body of eval_metrics.eval_rendering (render through the autograd binding under no_grad, clamp,
image[mask], psnr(...).item(), ssim(...).item(): the path before the native one), on a SYN-C-shaped map of 300 000
Gaussians at 640x480 and at 1200x680 with a depth image; the PyTorch scoring alone (the body without its render); and
the scorer's kernel time by the library's own events.  One human-readable line per measurement, then one JSON line."""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import _cabi, eval_metrics, synthetic as S  # noqa: E402


def wall_us(fn, warm, timed):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(timed):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / timed * 1e6


def profile(dev, W, H, N, with_depth, n_views=20):
    from monogs_amd.bench_legs import _model_from_scene
    from monogs_amd.eval_native import NativeEvaluator
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.parallel import view_pose
    from monogs_amd.slam_loops import Pipe, ViewCamera
    sc = S.make_scene(N, W, H, seed=0)
    cam = sc.cam
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    bg = torch.zeros(3, device=dev)
    gm = _model_from_scene(sc, dev)
    g = torch.Generator(device=dev).manual_seed(2)
    gt = sc.gt_image.to(dev).float().clamp(0, 1).contiguous()
    gt[:, : H // 8] = 0.0                                   # a masked border, as a real frame has
    depth = (0.5 + 5.0 * torch.rand(H, W, device=dev, generator=g)) if with_depth else None
    views = [ViewCamera(i, gt, view_pose(i % 5), cam.projmatrix_raw, fovx, fovy, H, W, dev) for i in range(n_views)]
    ev = NativeEvaluator(gm, bg, H, W, dev, max_views=n_views)
    last = {}

    def native():
        ev.begin()
        for v in views:
            ev.score(v, gt, gt_depth=depth)
        last["native"] = ev.finish()

    def torch_scoring(image):
        mask = gt > 0
        p = eval_metrics.psnr(image[mask].unsqueeze(0), gt[mask].unsqueeze(0)).item()
        s = eval_metrics.ssim(image.unsqueeze(0), gt.unsqueeze(0)).item()
        return p, s

    def torch_path():
        ps = []
        for v in views:
            with torch.no_grad():
                image = torch.clamp(render(v, gm, Pipe, bg)["render"], 0.0, 1.0)
            ps.append(torch_scoring(image))
        last["torch"] = ps

    with torch.no_grad():
        fixed = torch.clamp(render(views[0], gm, Pipe, bg)["render"], 0.0, 1.0)

    def torch_scoring_only():
        for _ in views:
            torch_scoring(fixed)

    t_native = wall_us(native, 2, 5) / n_views
    t_torch = wall_us(torch_path, 1, 3) / n_views
    t_score = wall_us(torch_scoring_only, 1, 3) / n_views
    _cabi.profile_enable(True)
    native()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    kernels = {n: round(v[0] / v[1] * 1e3, 1) for n, v in sorted(p.items(), key=lambda kv: -kv[1][0])}
    res = last["native"]
    d_psnr = max(abs(a - b[0]) for a, b in zip(res["psnr"].tolist(), last["torch"]))
    d_ssim = max(abs(a - b[1]) for a, b in zip(res["ssim"].tolist(), last["torch"]))
    r = {"native_us_per_view": round(t_native, 1), "torch_us_per_view": round(t_torch, 1),
         "torch_scoring_only_us_per_view": round(t_score, 1), "speedup": round(t_torch / t_native, 2),
         "eval_score_kernel_us": kernels.get("eval_score"), "kernels_us": kernels,
         "pairs": int(res["pairs"].max()), "capacity": ev.capacity, "regrows": ev.overflow_regrows,
         "max_psnr_diff_db": d_psnr, "max_ssim_diff": d_ssim}
    return (f"eval {N} Gaussians @ {W}x{H}{' + depth' if with_depth else ''}, {n_views} views: native "
            f"{t_native:.1f} us / view (one synchronisation per batch; scorer kernel {kernels.get('eval_score')} us); "
            f"eval_rendering's loop body {t_torch:.1f} us / view, of which PyTorch scoring {t_score:.1f} us; "
            f"{r['speedup']}x; largest difference {d_psnr:.1e} dB / {d_ssim:.1e} SSIM; "
            f"native kernels (us per launch): {kernels}"), r


def main():
    dev = torch.device("cuda:0")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eval_profile.txt")
    lines, out = [], {}
    for W, H, N, with_depth in ((640, 480, 300000, False), (1200, 680, 300000, True)):
        line, r = profile(dev, W, H, N, with_depth)
        print(line, flush=True)
        lines.append(line)
        out[f"{W}x{H}"] = r
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
