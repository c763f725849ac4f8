"""The scene, views and mirror runs shared by test_cpu_icp.py and test_gpu_icp.py.

The wavy scene: the surface z = 1.45 + 0.12 sin 3x cos 4y in a 52 x 36 x 24 volume at voxel 0.05, seen on 70 x 45 images
at f = 60 (neither side a multiple of 8, of 64 or of stride 4).  The depth of the surface from any pose is a per-ray
fp64 root solve.  For the CPU tests the model planes are ANALYTIC - the exact depth at the model pose and
depth_normal_torch of it - so the CPU suite pays for no ray cast; the GPU tests ray cast the fused volume on the device
and feed the device's own planes to the mirror.  Mirror results are computed once (lru_cache) and handed out read-only by
convention."""
import functools

import numpy as np
import torch

H, W = 45, 70
FX, FY, CX, CY = 60.0, 60.0, 34.5, 22.0
INTR = (FX, FY, CX, CY)
VS = 0.05
ORIGIN = (-1.3, -0.9, 0.9)
DIMS = (52, 36, 24)
Z_FAR = 2.4
MAX_BRICKS = 400

# the start of the recovery case: the frame is 0.0439 m and 2.24 degrees away from the model pose
TAU_TRUE = (0.03, -0.02, 0.025, 0.025, -0.02, 0.0225)
CAP_T, CAP_R_DEG = 0.5 * VS, 0.5            # half a voxel, half a degree


def surface(x, y):
    return 1.45 + 0.12 * np.sin(3.0 * x) * np.cos(4.0 * y)


def pose(tau):
    """Exp(tau) as a float64 [4,4] world -> camera matrix."""
    from monogs_amd.pose import SE3_exp
    return SE3_exp(torch.tensor(tau, dtype=torch.float64)).numpy()


def look_from(centre, yaw):
    """A camera at `centre` turned by `yaw` about the y axis."""
    T = pose((0.0, 0.0, 0.0, 0.0, yaw, 0.0))
    T[:3, 3] = -T[:3, :3] @ np.asarray(centre, np.float64)
    return T


def fusion_poses():
    """The three views the volume is fused from: I, and two about 0.15 m to the sides, turned about 0.1 rad inwards."""
    return [np.eye(4), look_from((0.15, 0.01, 0.0), 0.1), look_from((-0.15, -0.01, 0.0), -0.1)]


def true_pose():
    return pose(TAU_TRUE)


def pose_error(T, T_ref):
    """(distance of the camera centres in m, angle between the rotations in degrees)."""
    T, T_ref = np.asarray(T, np.float64), np.asarray(T_ref, np.float64)
    c = lambda M: -M[:3, :3].T @ M[:3, 3]
    cos = (np.trace(T[:3, :3] @ T_ref[:3, :3].T) - 1.0) / 2.0
    return float(np.linalg.norm(c(T) - c(T_ref))), float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))))


def surface_depth(T_w2c, h=H, w=W, intr=INTR):
    """The camera-z depth [h,w] fp32 of the surface along every pixel's ray (pixel centre 0): bisection in fp64 on
    g(z) = w_z - surface(w_x, w_y), which is negative in front of the surface and positive behind it."""
    T = np.asarray(T_w2c, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)          # camera frame, z = 1
    centre, dirs = -R.T @ t, ray @ R                                             # R^T ray, row-wise
    g = lambda z: (centre[2] + z * dirs[..., 2]) - surface(centre[0] + z * dirs[..., 0], centre[1] + z * dirs[..., 1])
    lo, hi = np.full((h, w), 0.5), np.full((h, w), 3.0)
    assert bool((g(lo) < 0).all() and (g(hi) > 0).all())
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        behind = g(mid) > 0
        lo, hi = np.where(behind, lo, mid), np.where(behind, mid, hi)
    return torch.from_numpy((0.5 * (lo + hi)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def model_planes(h=H, w=W, intr=INTR):
    """The analytic model at T_model = I: dict(depth [h,w], normal [3,h,w]) - the layout of mgs_depth_normal."""
    from monogs_amd.surface import depth_normal_torch
    depth = surface_depth(np.eye(4), h, w, intr)
    return {"depth": depth, "normal": depth_normal_torch(depth, *intr, pixel_center=0.0)}


@functools.lru_cache(maxsize=None)
def frame_depth(h=H, w=W, intr=INTR):
    """The sensor frame of the recovery case: the surface from true_pose()."""
    return surface_depth(true_pose(), h, w, intr)


@functools.lru_cache(maxsize=None)
def sensor_normal(h=H, w=W, intr=INTR):
    from monogs_amd.surface import depth_normal_torch
    return depth_normal_torch(frame_depth(h, w, intr), *intr, pixel_center=0.0)


def patched_depth():
    """frame_depth() with 0, NaN, inf and over-depth_max patches, where sparse_tsdf_cases.view_planes has them."""
    d = frame_depth().clone()
    d[3:6, 10:20] = 0.0
    d[20:23, 30:40] = float("nan")
    d[30:34, 5:15] = float("inf")
    d[10:14, 50:60] = 3.0
    return d


@functools.lru_cache(maxsize=None)
def recovery_mirror(levels):
    from monogs_amd import icp
    return icp.align_numpy(model_planes(), frame_depth(), INTR, np.eye(4, dtype=np.float32), levels=levels,
                           sensor_normal=sensor_normal())


# ---- the status cases ------------------------------------------------------------------------------------------------
def plane_model(depth=1.5):
    n = torch.zeros(H, W, 3)
    n[..., 2] = -1.0
    return {"depth": torch.full((H, W), depth), "normal": n}


def plane_sensor_normal():
    n = torch.zeros(3, H, W)
    n[2] = -1.0
    return n


def tilted_depth(tan_alpha=0.68):
    """The plane z = 1.5 + x tan(alpha) along every ray: z = 1.5 / (1 - rx tan(alpha))."""
    rx = (torch.arange(W, dtype=torch.float64) - CX) / FX
    return (1.5 / (1.0 - rx * tan_alpha)).float()[None, :].repeat(H, 1)


def status_cases():
    """name -> (model, depth, kwargs of align / align_numpy, the status expected)."""
    from monogs_amd import icp
    return {
        "degenerate": (plane_model(), torch.full((H, W), 1.5), dict(sensor_normal=plane_sensor_normal()), icp.DEGENERATE),
        "too_few": (model_planes(), torch.zeros(H, W), {}, icp.TOO_FEW),
        # Against the fronto-parallel model plane the residual of the tilted plane is -x tan(alpha) and the row of theta_y is
        # x, so the linearised step is theta_y = tan(alpha) = 0.68 > 0.5; damping makes the three free directions solvable.
        "step_too_large": (plane_model(), tilted_depth(), dict(dist=2.0, cos_min=0.0, damping=1e-3, min_pivot_ratio=0.0),
                           icp.STEP_TOO_LARGE),
    }


def same_result(got, want):
    """A device result of icp.align against align_numpy's: record, history, D and T_w2c bit for bit."""
    rec, hist = got["record"].cpu().numpy(), got["history"].cpu().numpy()
    D, T = got["D"].cpu().numpy(), got["T_w2c"].cpu().numpy()
    ok = True
    for name, a, b in (("record", rec, want["record"]), ("history", hist, want["history"]),
                       ("D", D.view(np.int64), want["D"].view(np.int64)), ("T_w2c", T.view(np.int32), want["T_w2c"].view(np.int32))):
        if not np.array_equal(a, b):
            print(f"{name} differs:\n{a}\n{b}")
            ok = False
    return ok
