"""Mesh export on the GPU box:

    python profiles/tsdf_profile.py [output file]          # default: profiles/tsdf_profile.txt

One integration and one extraction on a 256^3 volume around a SYN-C-shaped map of 300 000 Gaussians seen at 640x480:
wall time per TSDFVolume.integrate() / extract_mesh() call (a host clock around a batch of calls that ends in one
synchronise; the extraction synchronises itself, by its one host read), the kernels' own times from the library's
events, and the achieved traffic against the model of the issue - 20 B read + 20 B written per UPDATED point with an
image (tsdf, weight, three colour planes) for the integration, 8 B per point (tsdf, weight) for the classification.
Beside it the same integration through the mirror tsdf.integrate_torch on the device (eager fp32 torch, no culling),
and the extraction through the NumPy mirror on the host at 128^3 (at 256^3 its key table alone is 0.9 GB).  No threshold
is set anywhere: the numbers are written down.  One human-readable line per measurement, then one JSON line."""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import _cabi, synthetic as S, tsdf as T  # noqa: E402

COPY_TBS = 6.29      # MI355X float4 copy, measured (8.0 TB/s specified)


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
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.parallel import view_pose
    from monogs_amd.slam_loops import Pipe, ViewCamera
    sc = S.make_scene(N, W, H, seed=0)
    cam = sc.cam
    gm = _model_from_scene(sc, dev)
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    view = ViewCamera(0, torch.zeros(3, H, W), view_pose(1), cam.projmatrix_raw, fovx, fovy, H, W, dev,
                      intrinsics=(cam.fx, cam.fy, cam.cx, cam.cy))
    with torch.no_grad():
        pkg = render(view, gm, Pipe, torch.zeros(3, device=dev))
    return gm, view, {k: pkg[k].detach().clone() for k in ("render", "depth", "opacity")}


def volume_for(gm, n, dev):
    xyz = gm.get_xyz.detach()
    lo, hi = xyz.min(dim=0).values.cpu(), xyz.max(dim=0).values.cpu()
    vs = float((hi - lo).max()) / (n - 1)
    return T.TSDFVolume([float(v) for v in lo], vs, (n, n, n), device=dev)


def kernel_us(fn):
    _cabi.profile_enable(True)
    fn()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    return {n: round(v[0] / v[1] * 1e3, 1) for n, v in p.items()}


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "tsdf_profile.txt")
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = setup(dev, W, H, N)
    vol = volume_for(gm, n, dev)
    cam = (view.fx, view.fy, view.cx, view.cy)
    kw = dict(image=pkg["render"], opacity=pkg["opacity"], normalize=True, min_opacity=0.95)
    integ = lambda: vol.integrate(pkg["depth"], view.T, *cam, **kw)
    integ()
    torch.cuda.synchronize()
    updated = int((vol.weight > 0).sum())
    points = n ** 3
    out = {"volume": [n, n, n], "voxel_size": vol.voxel_size, "image": [W, H], "gaussians": N, "updated_points": updated}
    lines = []

    t_int = wall_us(integ, 3, 20)
    k_int = kernel_us(integ)["tsdf_integrate"]
    gbs = updated * 40 / (k_int * 1e-6) / 1e9
    out["integrate"] = {"wall_us": round(t_int, 1), "kernel_us": k_int, "model_GBs": round(gbs, 1),
                        "fraction_of_copy_rate": round(gbs / (COPY_TBS * 1e3), 3)}
    lines.append(f"integrate {n}^3 (voxel {vol.voxel_size:.4f}) from one {W}x{H} view of {N} Gaussians, depth / opacity with "
                 f"an image: {updated} of {points} points updated; {t_int:.0f} us per call (wall), k_tsdf_integrate "
                 f"{k_int:.1f} us; 40 B per updated point = {gbs:.0f} GB/s = {100 * gbs / (COPY_TBS * 1e3):.1f} % of the "
                 f"{COPY_TBS} TB/s copy rate")

    ref = (torch.ones_like(vol.tsdf), torch.zeros_like(vol.weight), torch.zeros_like(vol.color))
    mirror = lambda: T.integrate_torch(*ref, vol.origin, vol.voxel_size, vol.trunc, pkg["depth"], view.T, *cam,
                                       max_weight=vol.max_weight, **kw)
    t_mir = wall_us(mirror, 1, 3)
    out["integrate_torch_on_device_us"] = round(t_mir, 1)
    lines.append(f"the same integration through tsdf.integrate_torch on the device (eager torch, no culling): {t_mir:.0f} us "
                 f"per call = {t_mir / t_int:.0f} x the native call")
    del ref

    # the streaming rate of the kernel itself: a view that holds the whole volume, a constant depth behind it - every
    # lattice point is updated, nothing is culled
    dense = volume_for(gm, n, dev)
    e = dense.voxel_size * (n - 1)
    Td = torch.eye(4, device=dev)
    Td[:3, 3] = -torch.tensor([dense.origin[0] + 0.5 * e, dense.origin[1] + 0.5 * e, dense.origin[2] - e], device=dev)
    far = torch.full((H, W), 3.0 * e, device=dev)
    dcam = (0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5)
    for name, img in (("with an image", pkg["render"]), ("without an image", None)):
        dense.reset()
        run = lambda: dense.integrate(far, Td, *dcam, image=img, z_near=0.0)
        run()
        torch.cuda.synchronize()
        upd = int((dense.weight > 0).sum())
        t_d = wall_us(run, 2, 10)
        k_d = kernel_us(run)["tsdf_integrate"]
        per = 40 if img is not None else 16
        g = upd * per / (k_d * 1e-6) / 1e9
        out["integrate_dense_" + name.split()[0]] = {"updated_points": upd, "wall_us": round(t_d, 1), "kernel_us": k_d,
                                                      "bytes_per_point": per, "model_GBs": round(g, 1),
                                                      "fraction_of_copy_rate": round(g / (COPY_TBS * 1e3), 3)}
        lines.append(f"integrate {n}^3, a view that holds the whole volume and a constant depth behind it, {name}: {upd} of "
                     f"{points} points updated; {t_d:.0f} us per call (wall), k_tsdf_integrate {k_d:.1f} us; {per} B per "
                     f"updated point = {g:.0f} GB/s = {100 * g / (COPY_TBS * 1e3):.1f} % of the copy rate")
    del dense, far

    # (the timing loops above accumulated the same view many times: the surface is that of one view)
    ext = lambda: vol.extract_mesh(1.0)
    verts, faces, _ = ext()
    t_ext = wall_us(ext, 2, 10)
    k_ext = kernel_us(ext)
    cls_gbs = points * 8 / (k_ext["mesh_classify"] * 1e-6) / 1e9
    out["extract"] = {"wall_us": round(t_ext, 1), "kernels_us": k_ext, "verts": int(verts.shape[0]),
                      "faces": int(faces.shape[0]), "classify_model_GBs": round(cls_gbs, 1),
                      "classify_fraction_of_copy_rate": round(cls_gbs / (COPY_TBS * 1e3), 3)}
    lines.append(f"extract_mesh {n}^3: {verts.shape[0]} vertices, {faces.shape[0]} faces; {t_ext:.0f} us per call (wall, "
                 f"with its host read of (V, F) and three output allocations); kernels (us per launch): {k_ext}; "
                 f"k_mesh_classify at 8 B per point = {cls_gbs:.0f} GB/s = {100 * cls_gbs / (COPY_TBS * 1e3):.1f} % of the "
                 f"copy rate")
    del verts, faces

    # the NumPy mirror on the host, at 128^3, against the device at the same size
    small = volume_for(gm, 128, dev)
    small.integrate(pkg["depth"], view.T, *cam, **kw)
    t_small = wall_us(lambda: small.extract_mesh(1.0), 2, 10)
    planes = [t.cpu().numpy() for t in (small.tsdf, small.weight, small.color)]
    t0 = time.perf_counter()
    rv, rf, _ = T.extract_mesh_numpy(*planes, small.origin, small.voxel_size, 1.0)
    t_np = (time.perf_counter() - t0) * 1e6
    sv, sf, _ = small.extract_mesh(1.0)
    out["extract_128"] = {"native_wall_us": round(t_small, 1), "numpy_mirror_host_us": round(t_np, 1),
                          "verts": int(sv.shape[0]), "faces": int(sf.shape[0]),
                          "mirror_agrees": bool(sv.shape[0] == rv.shape[0] and sf.shape[0] == rf.shape[0])}
    lines.append(f"extract_mesh 128^3: {sv.shape[0]} vertices, {sf.shape[0]} faces; native {t_small:.0f} us per call, "
                 f"tsdf.extract_mesh_numpy on the host {t_np / 1e3:.0f} ms (planes already on the host)")
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
