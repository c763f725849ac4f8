"""The surface planes on the GPU box:

    python profiles/surface_profile.py [output file]          # default: profiles/surface_profile.txt

On SYN-C-shaped maps of 300 000 and 8 000 Gaussians at 640x480 (the scenes of profiles/viewer_profile.py):
  - the kernel times of k_surface_median, k_blend_fwd and k_view_first_hit on the SAME sorted tile lists in the same
    run, from the library's own events (mgs_profile_*): surface() and frame("flat_ball") alternate at one camera, so
    each of the three walks the lists the same project / emit / sort launches made;
  - the wall time of NativeViewer.surface() (with and without normals) and of the two surface modes of frame() against
    frame("depth") - a host clock around a batch of calls that ends in one synchronise;
  - k_depth_normal's time and its rate over the 16 bytes per pixel it has to move (4 read, 12 written) against the
    6.29 TB/s a float4 copy reaches on this chip - at 640x480, where the plane is one launch latency, and at 4096x4096,
    where the time is a rate.
One human-readable line per measurement, then one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from monogs_amd import _cabi, viewer as V  # noqa: E402
from viewer_profile import setup, wall_us  # noqa: E402

COPY_TBS = 6.29                      # float4 copy, measured (HBM3E; 8.0 TB/s spec)
WALKS = ("surface_median", "blend_fwd", "view_first_hit")
ROUNDS = 20


def profile(dev, W, H, N):
    gm, view, _, bg = setup(dev, W, H, N)
    vw = V.NativeViewer(gm, bg, H, W, dev)
    wall = {"surface": wall_us(lambda: vw.surface(view), 3, 30),
            "surface_no_normals": wall_us(lambda: vw.surface(view, normals=False), 3, 30),
            "frame_depth": wall_us(lambda: vw.frame(view, "depth"), 3, 30),
            "frame_median_depth": wall_us(lambda: vw.frame(view, "median_depth"), 3, 30),
            "frame_normal": wall_us(lambda: vw.frame(view, "normal"), 3, 30)}
    assert vw.check_capacity()
    _cabi.profile_enable(True)
    for _ in range(ROUNDS):
        vw.surface(view)
        vw.frame(view, "flat_ball")
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    assert vw.check_capacity()
    kernels = {n: round(v[0] / v[1] * 1e3, 2) for n, v in sorted(p.items(), key=lambda kv: -kv[1][0])}
    launches = {n: v[1] for n, v in p.items() if n in WALKS + ("depth_normal",)}
    crossed = float((vw.median_index >= 0).float().mean())
    t_n = kernels["depth_normal"]
    rate = 16.0 * H * W / (t_n * 1e-6) / 1e12
    r = {"wall_us": {k: round(v, 1) for k, v in wall.items()}, "kernels_us": kernels, "launches": launches,
         "capacity": vw.capacity, "pixels_with_a_median": round(crossed, 4),
         "depth_normal": {"us": t_n, "bytes": 16 * H * W, "tb_per_s": round(rate, 3), "of_copy_rate": round(rate / COPY_TBS, 3)}}
    walks = ", ".join(f"{n} {kernels[n]:.1f}" for n in WALKS)
    line = (f"surface {N} Gaussians @ {W}x{H}: kernels on the same tile lists by the library's events (us per launch, "
            f"{ROUNDS} rounds of surface() + frame('flat_ball')): {walks}; depth_normal {t_n:.2f} us = {rate:.2f} TB/s of its "
            f"16 B per pixel, {100 * rate / COPY_TBS:.0f} % of the {COPY_TBS} TB/s copy rate; wall us per call: "
            + ", ".join(f"{k} {v:.0f}" for k, v in wall.items())
            + f"; {100 * crossed:.1f} % of the pixels have a median; all kernels: {kernels}")
    return line, r


def normal_streaming(dev, W=4096, H=4096):
    """k_depth_normal on a plane large enough for its time to be a rate (a 640x480 plane is one launch latency)."""
    vw = V.NativeViewer(None, torch.zeros(3), H, W, dev)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev),
                          indexing="ij")
    depth = (2.0 + 0.3 * torch.sin(u / 90.0) * torch.cos(v / 70.0)).contiguous()        # every inner pixel has a normal
    out = torch.empty(3, H, W, device=dev)
    fn = lambda: vw.depth_normal(depth, 0.9 * W, 0.9 * W, 0.5 * W, 0.5 * H, 0.5, 0.05, out)
    t_wall = wall_us(fn, 3, 30)
    _cabi.profile_enable(True)
    for _ in range(ROUNDS):
        fn()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    t = p["depth_normal"][0] / p["depth_normal"][1] * 1e3
    rate = 16.0 * H * W / (t * 1e-6) / 1e12
    r = {"width": W, "height": H, "us": round(t, 1), "wall_us": round(t_wall, 1), "bytes": 16 * H * W,
         "tb_per_s": round(rate, 2), "of_copy_rate": round(rate / COPY_TBS, 3),
         "pixels_with_a_normal": round(float((out != 0).any(dim=0).float().mean()), 4)}
    return (f"depth_normal streaming, {W}x{H} ({16 * H * W / 1e6:.0f} MB at 16 B per pixel): {t:.1f} us by the library's "
            f"events ({t_wall:.1f} wall) = {rate:.2f} TB/s, {100 * rate / COPY_TBS:.0f} % of the {COPY_TBS} TB/s copy rate"), r


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "surface_profile.txt")
    lines, out = [], {}
    for N in (300000, 8000):
        line, r = profile(dev, 640, 480, N)
        print(line, flush=True)
        lines.append(line)
        out[str(N)] = r
    line, out["depth_normal_streaming"] = normal_streaming(dev)
    print(line, flush=True)
    lines.append(line)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
