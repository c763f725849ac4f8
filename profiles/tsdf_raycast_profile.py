"""The ray cast of the TSDF volumes on the GPU box:

    python profiles/tsdf_raycast_profile.py [output file]          # default: profiles/tsdf_raycast_profile.txt

The 256^3 / 640 x 480 / 300 000-Gaussian case of profiles/sparse_tsdf_profile.py - one rendered view fused into a dense
and a sparse volume of the same lattice - and its quarter-voxel variant (sparse only).  Per volume: raycast() at the
fused view's pose with and without `skip` (wall, the kernels' own times from the library's events, the samples the march
evaluated per ray), the shade launch, volume_depth_l1 over 20 views, and the route the ray cast replaces:
extract_mesh + render_mesh_depth + render_mesh_frame.  The mirror raycast_torch is timed on a 160 x 120 image of the same
camera (its planes are copied to the host first; the full image takes minutes).  integrate() and extract_mesh() of both
volumes are measured in the same run next to the values profiles/sparse_tsdf_profile.txt recorded, since the map helpers
of sparse_tsdf.hip moved into a header.  Wall times are medians of warm calls, each ended by a synchronise; kernel times
are means over five warm calls.  No threshold is set anywhere: the numbers are written down.  One human-readable line
per measurement, then one JSON line."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import mesh_clean_profile as CP  # noqa: E402
import tsdf_profile as TP  # noqa: E402
from monogs_amd import tsdf_raycast as R  # noqa: E402
from monogs_amd.mesh_render import render_mesh_depth, render_mesh_frame  # noqa: E402
from monogs_amd.sparse_tsdf import SparseTSDFVolume  # noqa: E402


def recorded_values():
    try:
        with open(os.path.join(ROOT, "profiles", "sparse_tsdf_profile.txt"), encoding="utf-8") as fh:
            rec = json.loads(fh.read().strip().splitlines()[-1])
        return {"dense_256": {"integrate_wall_us": rec["dense_256"]["integrate_wall_us_three_runs"],
                              "integrate_kernels_us": rec["dense_256"]["integrate_kernels_us"],
                              "extract_wall_us": rec["dense_256"]["extract_wall_us_three_runs"],
                              "extract_kernels_us": rec["dense_256"]["extract_kernels_us"]},
                **{n: {"integrate_again_wall_us": rec[n]["integrate_again_wall_us"], "kernels_again_us": rec[n]["kernels_again_us"],
                       "extract_wall_us": rec[n]["extract_wall_us"], "extract_kernels_us": rec[n]["extract_kernels_us"]}
                   for n in ("sparse_256", "sparse_quarter_voxel")}}
    except (OSError, ValueError, KeyError):
        return {}


def measure(name, vol, view, pkg, kw, lines, out, recorded):
    cam = (view.fx, view.fy, view.cx, view.cy)
    vt = (view.T, *cam, view.image_height, view.image_width)
    ikw = dict(image=pkg["render"], opacity=pkg["opacity"], normalize=True, min_opacity=0.95)
    integ = lambda: vol.integrate(pkg["depth"], view.T, *cam, **ikw)
    rec = {"voxel_size": vol.voxel_size, "steps_per_ray": R.march_steps(vol.voxel_size, kw["z_near"], kw["z_far"])[1]}
    rec["integrate_wall_us"] = round(CP.median_us(integ, 3, 21), 1)
    rec["integrate_kernels_us"] = CP.kernels_us(integ)
    vol.reset()
    integ()                                             # one view, as the sparse profile holds it
    ext = lambda: vol.extract_mesh(1.0)
    verts, faces, colors = ext()
    rec["extract_wall_us"] = round(CP.median_us(ext, 3, 21), 1)
    rec["extract_kernels_us"] = CP.kernels_us(ext)
    rec["recorded_by_sparse_tsdf_profile_txt"] = recorded.get(name, {})
    for skip in (True, False):
        run = lambda: R.raycast_view(vol, vt, skip=skip, **kw)
        planes = R.raycast_view(vol, vt, skip=skip, count_evaluated=True, **kw)
        torch.cuda.synchronize()
        ev = planes["evaluated"].float()
        tag = "skip" if skip else "plain"
        rec[f"raycast_{tag}_wall_us"] = round(CP.median_us(run, 3, 21), 1)
        rec[f"raycast_{tag}_kernels_us"] = CP.kernels_us(run)
        rec[f"raycast_{tag}_evaluated_per_ray"] = {"mean": round(float(ev.mean()), 1), "max": int(ev.max())}
        rec["hits"] = int((planes["hit_step"] >= 0).sum())
    planes = R.raycast_view(vol, vt, **kw)
    both = (planes["depth"] > 0) & (pkg["opacity"][0] >= 0.95)
    sensor = torch.where(pkg["opacity"] >= 0.95, pkg["depth"] / pkg["opacity"], torch.zeros_like(pkg["depth"]))[0]
    rec["depth_against_fused_view"] = {"pixels": int(both.sum()), "mean_abs": float((planes["depth"] - sensor).abs()[both].mean())}
    shade = lambda: R.shade(planes, vt, "shaded", depth_range=(kw["z_near"], kw["z_far"]))
    rec["shade_wall_us"] = round(CP.median_us(shade, 3, 21), 1)
    rec["shade_kernels_us"] = CP.kernels_us(shade)
    frame = lambda: R.raycast_frame(vol, vt, "shaded", **kw)
    rec["raycast_frame_wall_us"] = round(CP.median_us(frame, 3, 21), 1)
    l1 = lambda: R.volume_depth_l1(vol, [vt] * 20, [sensor] * 20, **kw)
    rec["volume_depth_l1_20_views"] = l1()
    rec["volume_depth_l1_20_views_wall_us"] = round(CP.median_us(l1, 2, 7), 1)

    def route():
        v, f, _ = vol.extract_mesh(1.0)
        render_mesh_depth(v, f, *vt, kw["z_near"])
        return render_mesh_frame(v, f, vt, "shaded", z_near=kw["z_near"])

    route()
    rec["mesh_route_wall_us"] = round(CP.median_us(route, 3, 21), 1)
    rec["mesh_route_kernels_us"] = CP.kernels_us(route)
    out[name] = rec
    lines.append(f"{name}: voxel {vol.voxel_size:.5f}, {rec['steps_per_ray']} samples per ray, {rec['hits']} of "
                 f"{view.image_height * view.image_width} rays hit; raycast skip {rec['raycast_skip_wall_us']:.0f} us per call "
                 f"(wall), kernels {rec['raycast_skip_kernels_us']}, evaluated per ray {rec['raycast_skip_evaluated_per_ray']}; "
                 f"plain {rec['raycast_plain_wall_us']:.0f} us, kernels {rec['raycast_plain_kernels_us']}, evaluated per ray "
                 f"{rec['raycast_plain_evaluated_per_ray']}; shade {rec['shade_wall_us']:.0f} us (wall), "
                 f"{rec['shade_kernels_us']}; raycast_frame {rec['raycast_frame_wall_us']:.0f} us; volume_depth_l1 over 20 "
                 f"views {rec['volume_depth_l1_20_views_wall_us']:.0f} us (one host read), {rec['volume_depth_l1_20_views']}; "
                 f"the mesh route extract_mesh + render_mesh_depth + render_mesh_frame {rec['mesh_route_wall_us']:.0f} us "
                 f"(wall), kernels {rec['mesh_route_kernels_us']}, {sum(rec['mesh_route_kernels_us'].values()):.1f} us in all; "
                 f"ray cast depth against the fused view's own depth: {rec['depth_against_fused_view']}")
    lines.append(f"{name}, the header move: integrate {rec['integrate_wall_us']:.0f} us (wall), {rec['integrate_kernels_us']}; "
                 f"extract_mesh {rec['extract_wall_us']:.0f} us (wall), {rec['extract_kernels_us']}; recorded before: "
                 f"{rec['recorded_by_sparse_tsdf_profile_txt']}")
    return planes


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "tsdf_raycast_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    ok = pkg["opacity"] >= 0.95
    z_far = 1.1 * float((pkg["depth"] / pkg["opacity"])[ok].max())
    kw = dict(z_near=0.2, z_far=z_far)
    recorded = recorded_values()
    dense = TP.volume_for(gm, n, dev)
    origin, vs = dense.origin, dense.voxel_size
    cam = (view.fx, view.fy, view.cx, view.cy)
    ikw = dict(image=pkg["render"], opacity=pkg["opacity"], normalize=True, min_opacity=0.95)
    dense.integrate(pkg["depth"], view.T, *cam, **ikw)
    d_planes = measure("dense_256", dense, view, pkg, kw, lines, out, recorded)
    # the mirror, on a quarter of the image's side (the dense planes go to the host once)
    t0 = time.perf_counter()
    host = [t.cpu() for t in (dense.tsdf, dense.weight, dense.color)]
    small = R.raycast_torch(*host, origin, vs, (0, 0, 0), view.T.cpu(), view.fx / 4, view.fy / 4, view.cx / 4, view.cy / 4,
                            H // 4, W // 4, **kw)
    t_mirror = time.perf_counter() - t0
    got = dense.raycast(view.T, view.fx / 4, view.fy / 4, view.cx / 4, view.cy / 4, H // 4, W // 4, **kw)
    same = all(torch.equal(small[k].view(torch.int32), got[k].cpu().view(torch.int32)) for k in small)
    out["mirror_160x120"] = {"seconds": round(t_mirror, 2), "equals_device_bit_for_bit": same}
    lines.append(f"the mirror raycast_torch at 160 x 120 on the dense 256^3 planes: {t_mirror:.2f} s with the copy to the host; "
                 f"equals the device bit for bit: {same}")
    del host, dense
    sparse = SparseTSDFVolume(origin, vs, 65536, device=dev)
    sparse.integrate(pkg["depth"], view.T, *cam, **ikw)
    s_planes = measure("sparse_256", sparse, view, pkg, kw, lines, out, recorded)
    same = all(torch.equal(d_planes[k].view(torch.int32), s_planes[k].view(torch.int32)) for k in d_planes)
    out["sparse_256"]["equals_dense_bit_for_bit"] = same
    lines.append(f"sparse_256 against dense_256: the same bits in every plane: {same}")
    del sparse
    fine = SparseTSDFVolume(origin, vs / 4.0, 262144, device=dev)
    fine.integrate(pkg["depth"], view.T, *cam, **ikw)
    measure("sparse_quarter_voxel", fine, view, pkg, kw, lines, out, recorded)
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
