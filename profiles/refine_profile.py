"""Colour refinement (utils/slam_backend.py:335-368) on the GPU box:

    python profiles/refine_profile.py [gaussians ...]      # default: 300000 8000

1. The fused objective mgs_ssim_loss (value + gradient, one launch) against the PyTorch path the reference runs
   (l1 + eval_metrics.ssim, autograd forward + backward) at 640x480 and 1200x680, by device events after warm-up;
   the kernel's algorithmic bytes (12 C H W: two images in, one gradient out) and GB/s over its kernel time.
2. One refinement iteration on a SYN-C-shaped map (640x480, five keyframes): NativeMapper.color_refinement
   against slam_loops.color_refinement_step over the drop-in rasteriser (same model, same FusedGaussianAdam).
Prints one human-readable line per measurement and, last, one JSON line with everything."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import _cabi, eval_metrics, synthetic as S  # noqa: E402
from monogs_amd.tracking_fused import color_refinement_loss  # noqa: E402


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


def kernel_us(fn, name, reps):
    _cabi.profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    return p[name][0] / p[name][1] * 1e3


def loss_profile(dev, W, H):
    g = torch.Generator(device=dev).manual_seed(1)
    img = torch.rand(3, H, W, device=dev, generator=g).requires_grad_()
    gt = torch.rand(3, H, W, device=dev, generator=g)

    def fused():
        img.grad = None
        color_refinement_loss(img, gt, 0.2).backward()

    def torch_path():
        img.grad = None
        loss = 0.8 * torch.abs(img - gt).mean() + 0.2 * (1.0 - eval_metrics.ssim(img, gt))
        loss.backward()

    t_fused = device_time_us(fused, 20, 200)
    t_torch = device_time_us(torch_path, 10, 100)
    t_kernel = kernel_us(fused, "ssim_loss", 50)
    nbytes = 12 * 3 * H * W
    r = {"fused_us": round(t_fused, 1), "kernel_us": round(t_kernel, 1), "torch_us": round(t_torch, 1),
         "speedup": round(t_torch / t_fused, 1), "bytes": nbytes, "kernel_GBps": round(nbytes / t_kernel / 1e3, 1)}
    print(f"loss {W}x{H}: fused value+gradient {t_fused:.1f} us per call (kernel {t_kernel:.1f} us, "
          f"{r['kernel_GBps']} GB/s of {nbytes} algorithmic bytes); PyTorch l1 + ssim forward + backward "
          f"{t_torch:.1f} us ({r['speedup']}x)", flush=True)
    return r


def refine_profile(dev, N):
    from monogs_amd.bench_legs import _model_from_scene
    from monogs_amd.mapping_native import NativeMapper
    from monogs_amd.parallel import view_pose
    from monogs_amd.slam_loops import Pipe, ViewCamera, color_refinement_step
    sc = S.make_scene(N, 640, 480, seed=0)
    cam = sc.cam
    H, W = cam.H, cam.W
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    bg = torch.zeros(3, device=dev)

    def setup():
        gm = _model_from_scene(sc, dev)
        views = [ViewCamera(i, sc.gt_image, view_pose(i), cam.projmatrix_raw, fovx, fovy, H, W, dev) for i in range(5)]
        return gm, views

    gm, views = setup()
    mp = NativeMapper(gm, bg, concurrent_views=1)
    for i, v in enumerate(views):
        mp.add_keyframe(i, v)
    mp.color_refinement(iterations=20)
    torch.cuda.synchronize()
    iters = 200
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    mp.color_refinement(iterations=iters)
    b.record()
    torch.cuda.synchronize()
    t_native = a.elapsed_time(b) / iters * 1e3
    _cabi.profile_enable(True)
    mp.color_refinement(iterations=10)
    torch.cuda.synchronize()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    kernels = {n: round(v[0] / v[1] * 1e3, 1) for n, v in sorted(p.items(), key=lambda kv: -kv[1][0])}
    assert mp.check_capacity() and len(gm) == N

    gm, views = setup()
    draws = torch.randint(len(views), (iters + 10,), generator=torch.Generator().manual_seed(0)).tolist()
    for it, d in enumerate(draws[:10], start=1):
        color_refinement_step(views[d], gm, bg, 0.2, it, Pipe)
    torch.cuda.synchronize()
    n_py = iters // 4
    a.record()
    for it, d in enumerate(draws[10:10 + n_py], start=11):
        color_refinement_step(views[d], gm, bg, 0.2, it, Pipe)
    b.record()
    torch.cuda.synchronize()
    t_python = a.elapsed_time(b) / n_py * 1e3
    r = {"native_us": round(t_native, 1), "native_its_per_s": round(1e6 / t_native), "python_us": round(t_python, 1),
         "python_its_per_s": round(1e6 / t_python), "speedup": round(t_python / t_native, 1),
         "native_26000_s": round(26000 * t_native / 1e6, 1), "python_26000_s": round(26000 * t_python / 1e6, 1),
         "kernels_us": kernels}
    print(f"refinement {N} Gaussians @ {W}x{H}, 5 keyframes: native {t_native:.1f} us / iteration "
          f"({r['native_its_per_s']} its/s, 26000 iterations {r['native_26000_s']} s); Python body over the drop-in "
          f"{t_python:.1f} us ({r['python_its_per_s']} its/s, {r['python_26000_s']} s); {r['speedup']}x; "
          f"native kernels (us per launch): {kernels}", flush=True)
    return r


def main():
    dev = torch.device("cuda:0")
    sizes = [int(a) for a in sys.argv[1:]] or [300000, 8000]
    out = {"loss": {f"{W}x{H}": loss_profile(dev, W, H) for W, H in ((640, 480), (1200, 680))},
           "refine": {str(N): refine_profile(dev, N) for N in sizes}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
