"""The frame-to-model ICP on the GPU box:

    python profiles/icp_profile.py [output file]          # default: profiles/icp_profile.txt

The 256^3 / 640 x 480 / 300 000-Gaussian case of profiles/tsdf_raycast_profile.py: one rendered view fused into a dense and
a sparse volume of the same lattice.  The frame is that view's own normalised depth; the start pose is the view's pose
moved by 1.3 cm / 0.2 degrees.  That scene is a cloud of random Gaussians, not a surface: few pixels have a sensor
normal, and the run says what status the alignment ends with there.  So the same measurements are repeated at the same
image size on the wavy surface of tests/icp_cases.py (a 208 x 144 x 96 lattice at voxel 0.0125, three views fused), where
the alignment converges.  Measured: one iteration of every level of the default
schedule (both kernels from the library's events, and the wall time of a one-iteration schedule), the whole default schedule
enqueued at once (wall, with one synchronise at the end and no host read), track_against_volume on the dense and the sparse
volume, and for scale one first-order NativeTracker iteration of the same build on the same map.  raycast(), integrate()
and the tracking iteration are printed next to what profiles/tsdf_raycast_profile.txt and the README recorded before this
kernel existed: nothing in their code changed.  The RGB-D legs (icp.align(image=, photo_weight=): k_icp_intensity twice per
call, k_icp_rows_rgbd and k_icp_solve_rgbd per iteration) follow on the wavy scene, re-fused with the texture of
tests/icp_rgbd_cases.py AFTER its geometric legs were measured as before: the rows kernel per stride, the default schedule,
and track_against_volume dense and sparse, to be read against the geometric legs of the same run.  Wall times are medians of warm calls, each ended by a synchronise; kernel
times are means over five warm calls.  No threshold is set anywhere: the numbers are written down.  One human-readable line
per measurement, then one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import mesh_clean_profile as CP  # noqa: E402
import tsdf_profile as TP  # noqa: E402
from monogs_amd import icp  # noqa: E402
from monogs_amd.pose import SE3_exp  # noqa: E402
from monogs_amd.sparse_tsdf import SparseTSDFVolume  # noqa: E402
from monogs_amd.tracking_native import NativeTracker  # noqa: E402


def recorded_values():
    try:
        with open(os.path.join(ROOT, "profiles", "tsdf_raycast_profile.txt"), encoding="utf-8") as fh:
            rec = json.loads(fh.read().strip().splitlines()[-1])
        return {n: {k: rec[n][k] for k in ("integrate_wall_us", "integrate_kernels_us", "raycast_skip_wall_us", "raycast_skip_kernels_us")}
                for n in ("dense_256", "sparse_256")}
    except (OSError, ValueError, KeyError):
        return {}


def measure(name, vol, sensor, T_prev, vt, z_far, akw, levels, rec, lines):
    """track_against_volume on `vol`, and with `levels` one iteration of every level and the whole schedule on its ray cast."""
    cam, (H, W) = vt[1:5], vt[5:7]
    planes = vol.raycast(T_prev, *cam, H, W, z_far=z_far)
    track = lambda: icp.track_against_volume(vol, sensor, T_prev, vt, z_far=z_far, **akw)
    res = icp.track_against_volume(vol, sensor, T_prev, vt, z_far=z_far, **dict(akw, read=True))
    info = res["info"]
    rec["track_against_volume_wall_us"] = round(CP.median_us(track, 3, 21), 1)
    rec["track_against_volume_kernels_us"] = CP.kernels_us(track)
    rec["result"] = {"status": info["status_name"], "iterations_run": info["iterations_run"], "counts": info["counts"],
                     "ran": [int(v) for v in info["history"]["ran"]]}
    if "photo" in info:
        rec["result"]["photo"] = info["photo"]
    lines.append(f"{name}: track_against_volume (ray cast at the previous pose, sensor normals, the default schedule enqueued at once, "
                 f"no host read) {rec['track_against_volume_wall_us']:.0f} us (wall), kernels (means per launch, idle launches "
                 f"included) {rec['track_against_volume_kernels_us']}; {rec['result']}")
    if not levels:
        return res
    for stride, iters in icp.LEVELS:
        one = lambda: icp.align(planes, sensor, cam, T_prev, levels=((stride, 1),), **akw)
        k = CP.kernels_us(one)
        rec[f"stride_{stride}"] = {"one_iteration_schedule_wall_us": round(CP.median_us(one, 3, 21), 1), "kernels_us": k,
                                   "stride_grid_pixels": -(-W // stride) * -(-H // stride)}
        lines.append(f"{name}: one iteration at stride {stride} ({rec[f'stride_{stride}']['stride_grid_pixels']} pixels): "
                     f"kernels {k}; a one-iteration schedule (depth_normal, start, rows, solve) "
                     f"{rec[f'stride_{stride}']['one_iteration_schedule_wall_us']:.0f} us (wall)")
    full = lambda: icp.align(planes, sensor, cam, T_prev, **akw)
    rec["default_schedule_wall_us"] = round(CP.median_us(full, 3, 21), 1)
    rec["default_schedule_kernels_us"] = CP.kernels_us(full)
    fixed = lambda: icp.align(planes, sensor, cam, T_prev, converged=0.0, **akw)          # never converges: all 19 run
    rec["all_19_iterations_wall_us"] = round(CP.median_us(fixed, 3, 21), 1)
    rec["all_19_iterations_kernels_us"] = CP.kernels_us(fixed)
    lines.append(f"{name}: the default schedule {icp.LEVELS} enqueued at once: {rec['default_schedule_wall_us']:.0f} us (wall), "
                 f"kernels (means per launch, idle launches included) {rec['default_schedule_kernels_us']}; with converged = 0, all "
                 f"19 iterations running: {rec['all_19_iterations_wall_us']:.0f} us (wall), {rec['all_19_iterations_kernels_us']}")
    return res


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "icp_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    ok = pkg["opacity"] >= 0.95
    sensor = torch.where(ok, pkg["depth"] / pkg["opacity"], torch.zeros_like(pkg["depth"]))[0].contiguous()
    z_far = 1.1 * float(sensor.max())
    cam = (view.fx, view.fy, view.cx, view.cy)
    vt = (view.T, *cam, H, W)
    ikw = dict(image=pkg["render"], opacity=pkg["opacity"], normalize=True, min_opacity=0.95)
    T_prev = (SE3_exp(torch.tensor([0.01, -0.008, 0.002, 0.002, -0.003, 0.001])).to(dev) @ view.T).contiguous()
    akw = dict(depth_max=min(16.0, z_far), read=False)
    recorded = recorded_values()
    dense = TP.volume_for(gm, n, dev)
    sparse = SparseTSDFVolume(dense.origin, dense.voxel_size, 65536, device=dev)
    for name, vol in (("dense_256", dense), ("sparse_256", sparse)):
        integ = lambda: vol.integrate(pkg["depth"], view.T, *cam, **ikw)
        integ()
        cast = lambda: vol.raycast(T_prev, *cam, H, W, z_far=z_far)
        cast()
        rec = {"integrate_wall_us": round(CP.median_us(integ, 3, 21), 1), "integrate_kernels_us": CP.kernels_us(integ),
               "raycast_skip_wall_us": round(CP.median_us(cast, 3, 21), 1), "raycast_skip_kernels_us": CP.kernels_us(cast),
               "recorded_by_tsdf_raycast_profile_txt": recorded.get(name, {})}
        lines.append(f"{name}: integrate {rec['integrate_wall_us']:.0f} us (wall) {rec['integrate_kernels_us']}, raycast "
                     f"{rec['raycast_skip_wall_us']:.0f} us (wall) {rec['raycast_skip_kernels_us']}; recorded before this change: "
                     f"{rec['recorded_by_tsdf_raycast_profile_txt']}")
        vol.reset()
        integ()
        measure(name, vol, sensor, T_prev, vt, z_far, akw, name == "dense_256", rec, lines)
        out[name] = rec
    del dense, sparse
    # the same sizes on a scene the alignment converges on: the wavy surface of tests/icp_cases.py on a 208 x 144 x 96 lattice
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import icp_cases as IC
    from monogs_amd.tsdf import TSDFVolume
    intr = (548.0, 548.0, 319.5, 239.5)
    frame = IC.surface_depth(IC.true_pose(), H, W, intr).to(dev)
    eye = torch.eye(4, device=dev)
    volumes = (("wavy_dense", TSDFVolume(IC.ORIGIN, IC.VS / 4, tuple(4 * d for d in IC.DIMS), device=dev)),
               ("wavy_sparse", SparseTSDFVolume(IC.ORIGIN, IC.VS / 4, 16384, device=dev)))
    for name, vol in volumes:
        for T in IC.fusion_poses():
            vol.integrate(IC.surface_depth(T, H, W, intr).to(dev), torch.from_numpy(T).float().to(dev), *intr)
        rec = {}
        res = measure(name, vol, frame, eye, (eye, *intr, H, W), IC.Z_FAR, dict(read=False), name == "wavy_dense", rec, lines)
        et, er = IC.pose_error(res["info"]["T_w2c"], IC.true_pose())
        rec["pose_error"] = {"start_m_deg": IC.pose_error(torch.eye(4).numpy(), IC.true_pose()), "end_m_deg": (et, er)}
        lines.append(f"{name}: the frame starts {rec['pose_error']['start_m_deg']} (m, degrees) off and ends {rec['pose_error']['end_m_deg']} off")
        out[name] = rec
    # RGB-D: the same volumes fused again with colour, the same frame with its image, photo_weight 1
    import icp_rgbd_cases as RC
    image = RC.painted(frame.cpu(), IC.true_pose(), intr).to(dev)
    # fused from wider views (880 x 660, the same f), so that the border of the fused region, where a ray cast's colour
    # darkens, lies outside the tracked view - as tests/icp_rgbd_cases.py does at its size
    wide, views = (548.0, 548.0, 439.5, 329.5), []
    for T in IC.fusion_poses():
        depth = IC.surface_depth(T, 660, 880, wide)
        views.append((torch.from_numpy(T).float().to(dev), depth.to(dev), RC.painted(depth, T, wide).to(dev)))
    for name, vol in volumes:
        vol.reset()
        for T, depth, img in views:
            vol.integrate(depth, T, *wide, image=img)
        rec = {}
        res = measure(name + "_rgbd", vol, frame, eye, (eye, *intr, H, W), IC.Z_FAR, dict(read=False, image=image, photo_weight=1.0),
                      name == "wavy_dense", rec, lines)
        et, er = IC.pose_error(res["info"]["T_w2c"], IC.true_pose())
        rec["pose_error"] = {"end_m_deg": (et, er)}
        lines.append(f"{name}_rgbd: with the photometric rows the frame ends {rec['pose_error']['end_m_deg']} (m, degrees) off")
        out[name + "_rgbd"] = rec
    # for scale: one first-order tracking iteration of the same build on the same map
    from monogs_amd.slam_loops import ViewCamera
    vp = ViewCamera(1, pkg["render"], T_prev, view.projection_matrix, view.FoVx, view.FoVy, H, W, dev, intrinsics=cam)
    trk = NativeTracker(vp, gm, torch.zeros(3, device=dev))
    trk.args.adam.sticky_converged = 0
    out["tracking_first_order"] = {"wall_us": round(CP.median_us(trk.step, 20, 200), 1), "kernels_us": CP.kernels_us(trk.step),
                                   "recorded_in_README": "see the tracking rows of README.md"}
    lines.append(f"for scale, one first-order NativeTracker iteration on the same map: {out['tracking_first_order']['wall_us']:.0f} us "
                 f"(wall), kernels {sum(out['tracking_first_order']['kernels_us'].values()):.1f} us: {out['tracking_first_order']['kernels_us']}")
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
