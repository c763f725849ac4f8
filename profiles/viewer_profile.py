"""The headless viewer on the GPU box:

    python profiles/viewer_profile.py [output file]          # default: profiles/viewer_profile.txt

Wall time per viewer.NativeViewer.frame() call and mode (a host clock around a batch of calls that ends in one
synchronise) on SYN-C-shaped maps of 300 000 and 8 000 Gaussians at 640x480, with 20 keyframe frusta, the current camera
and a 200-point trajectory drawn over every frame; beside it the same frames made the way the reference's GUI makes them
- render() through the autograd binding under no_grad, then the mirror viewer.view_frame_torch on the rendered planes
(the device-tensor route) and the GUI's own host route (planes to NumPy, colour map and bytes on the host); for the two
ball modes, whose reference route is an OpenGL pass that does not exist here, the render() + host conversion of the
colour stands in.  Then the kernel times of the four new kernels (and the two reduction launches that feed them): from
the library's own events in this process, and from `rocprofv3 --kernel-trace --stats` over a child run of this script
(`--trace-run`).  One human-readable line per measurement, then one JSON line."""
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import _cabi, synthetic as S, viewer as V  # noqa: E402

NEW_KERNELS = ("view_compose", "view_max", "view_first_hit", "view_time_colors", "view_id_range", "view_overlay_project",
               "view_overlay_draw")


def wall_us(fn, warm, timed):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(timed):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / timed * 1e6


def setup(dev, W, H, N):
    from monogs_amd.bench_legs import _model_from_scene
    from monogs_amd.parallel import view_pose
    from monogs_amd.slam_loops import ViewCamera
    sc = S.make_scene(N, W, H, seed=0)
    cam = sc.cam
    gm = _model_from_scene(sc, dev)
    gm.unique_kfIDs = (torch.arange(N, dtype=torch.int32, device=dev) * 20 // N) * 5
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    view = ViewCamera(0, torch.zeros(3, H, W), view_pose(1), cam.projmatrix_raw, fovx, fovy, H, W, dev,
                      intrinsics=(cam.fx, cam.fy, cam.cx, cam.cy))
    c2w = [torch.linalg.inv(view_pose(i % 5).double()).float() for i in range(21)]
    for i, P in enumerate(c2w):
        P[:3, 3] += torch.tensor([0.05 * (i % 7) - 0.15, 0.03 * (i % 3), 0.4 + 0.1 * i])
    g = torch.Generator().manual_seed(4)
    traj = torch.cumsum(0.02 * torch.randn(200, 3, generator=g), dim=0) + torch.tensor([0.0, 0.0, 1.5])
    over = dict(keyframes=torch.stack(c2w[:20]).to(dev), current=c2w[20].to(dev), trajectory=traj.to(dev),
                frustum_size=0.05)
    return gm, view, over, torch.zeros(3, device=dev)


def host_route(pkg, mode):
    """slam_gui.py:577-653 with the colour map of this repository in the place of imgviz.depth2rgb."""
    if mode in ("depth", "opacity"):
        a = pkg[mode][0].detach().cpu().numpy()
        lo = V.DEPTH_LO if mode == "depth" else 0.0
        t = (a - lo) / (np.max(a) - lo)
        idx = np.minimum(255, (np.clip(np.nan_to_num(t), 0.0, 1.0) * 256).astype(np.int64))
        return np.ascontiguousarray(V.JET_LUT[idx])
    return (torch.clamp(pkg["render"], min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous().cpu().numpy()


def profile(dev, W, H, N):
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    gm, view, over, bg = setup(dev, W, H, N)
    vw = V.NativeViewer(gm, bg, H, W, dev)

    def render_planes(mode):
        with torch.no_grad():
            if mode != "time":
                return render(view, gm, Pipe, bg)
            keep = gm._features_dc                      # the GUI swaps the features for the tinted ones (:550-566)
            gm._features_dc = torch.nn.Parameter(V.time_colors_torch(keep.detach(), gm.unique_kfIDs))
            try:
                return render(view, gm, Pipe, bg)
            finally:
                gm._features_dc = keep

    def mirror(mode, with_overlay):
        pkg = render_planes(mode)
        kw = over if with_overlay else {}
        return V.view_frame_torch(mode, color=pkg["render"], depth=pkg["depth"], opacity=pkg["opacity"],
                                  hit_color=pkg["render"], camera=view, **kw)

    r = {}
    parts = []
    for mode in V.MODES:
        t_native = wall_us(lambda: vw.frame(view, mode, **over), 3, 30)
        t_plain = wall_us(lambda: vw.frame(view, mode), 3, 30)
        t_mirror = wall_us(lambda: mirror(mode, False), 2, 10)
        t_host = wall_us(lambda: host_route(render_planes(mode), mode), 2, 10)
        r[mode] = {"native_us": round(t_native, 1), "native_no_overlay_us": round(t_plain, 1),
                   "torch_mirror_no_overlay_us": round(t_mirror, 1), "host_numpy_no_overlay_us": round(t_host, 1)}
        parts.append(f"{mode} {t_native:.0f} (no overlay {t_plain:.0f}; render + torch mirror {t_mirror:.0f}; "
                     f"render + host NumPy {t_host:.0f})")
    r["rgb"]["torch_mirror_with_overlay_us"] = round(wall_us(lambda: mirror("rgb", True), 1, 3), 1)
    assert vw.check_capacity()
    _cabi.profile_enable(True)
    for mode in V.MODES:
        vw.frame(view, mode, **over)
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    r["kernels_us"] = {n: round(v[0] / v[1] * 1e3, 1) for n, v in sorted(p.items(), key=lambda kv: -kv[1][0])}
    r["capacity"] = vw.capacity
    new = {n: r["kernels_us"].get(n) for n in NEW_KERNELS}
    return (f"viewer {N} Gaussians @ {W}x{H}, 168 frustum lines + 199 trajectory pieces, us per frame(): "
            + "; ".join(parts) + f"; rgb through the torch mirror WITH its host-side overlay "
            f"{r['rgb']['torch_mirror_with_overlay_us']:.0f}; new kernels by the library's events (us per launch): {new}; "
            f"all kernels: {r['kernels_us']}"), r


def trace_run(dev):
    """What the rocprofv3 child runs: every mode a few times at both map sizes."""
    for N in (300000, 8000):
        gm, view, over, bg = setup(dev, 640, 480, N)
        vw = V.NativeViewer(gm, bg, 480, 640, dev)
        for _ in range(5):
            for mode in V.MODES:
                vw.frame(view, mode, **over)
        torch.cuda.synchronize()


def rocprof_kernels():
    """Average ns per launch of the k_view_* kernels from rocprofv3's kernel statistics, or a reason why not."""
    exe = "/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else "rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--trace-run"]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        except (OSError, subprocess.TimeoutExpired) as e:
            return None, f"rocprofv3 did not run: {e}"
        if p.returncode != 0:
            return None, f"rocprofv3 exit {p.returncode}: {p.stdout[-300:]}"
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    if "k_view_" in name:
                        short = name.split("k_view_")[1].split("(")[0].split("<")[0]
                        tmpl = "<" + name.split("<")[1].split(">")[0] + ">" if "<" in name.split("(")[0] else ""
                        out["k_view_" + short + tmpl] = {"calls": int(row["Calls"]),
                                                         "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                                         "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        if out:
            return out, None
        files = [os.path.relpath(f, d) for f in glob.glob(os.path.join(d, "**", "*"), recursive=True) if os.path.isfile(f)]
        return None, f"rocprofv3 wrote no kernel statistics for k_view_* (files: {files[:8]})"


def main():
    dev = torch.device("cuda:0")
    if "--trace-run" in sys.argv:
        trace_run(dev)
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "viewer_profile.txt")
    lines, out = [], {}
    for N in (300000, 8000):
        line, r = profile(dev, 640, 480, N)
        print(line, flush=True)
        lines.append(line)
        out[str(N)] = r
    stats, why = rocprof_kernels()
    out["rocprofv3"] = stats if stats is not None else {"not_measured": why}
    lines.append("rocprofv3 --kernel-trace --stats over both map sizes (5 frames per mode each; per launch): "
                 + (json.dumps(stats) if stats is not None else f"not measured ({why})"))
    print(lines[-1], flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
