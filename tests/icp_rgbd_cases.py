"""The textured scenes and mirror runs shared by test_cpu_icp_rgbd.py and test_gpu_icp_rgbd.py.

The textured plane: the fronto-parallel plane z = 1.5 of icp_cases.plane_model, 70 x 45 at f = 60, painted in WORLD
coordinates with texture(x, y), per channel 0.5 + 0.2 sin(a x + phi) cos(b y).  A pixel is 1.5 / 60 = 0.025 m on the plane,
so the periods 2 pi / a = 0.9 .. 1.3 m are 36 .. 52 pixels and 2 pi / b = 1.4 .. 2.1 m are 56 .. 84 pixels: the start offset
(TAU_PLANE: 0.036 m in the plane and 2 degrees about the optical axis, 1.4 pixels and, at the image corner, 1.5 pixels more)
stays well inside a quarter period, where Gauss-Newton on the intensity converges.  The frame is the plane seen from
pose(TAU_PLANE): an in-plane translation and a rotation about the optical axis keep every depth at exactly 1.5 - these are
the three directions [n ; p x n] cannot see.  Colours are analytic; nothing is rendered.

The textured wavy scene: icp_cases' surface painted with the same texture of the world point every ray meets."""
import functools

import numpy as np
import torch

import icp_cases as IC

H, W, INTR = IC.H, IC.W, IC.INTR
PLANE_Z = 1.5
# in-plane translation and rotation about the optical axis, of the size of icp_cases.TAU_TRUE
TAU_PLANE = (0.03, -0.02, 0.0, 0.0, 0.0, 0.035)
A = (6.9, 5.6, 4.8)          # rad / m along x, per channel
B = (4.4, 3.0, 3.7)          # rad / m along y
PHI = (0.3, 1.7, 2.9)
PHOTO_WEIGHT = 1.0


def texture(x, y):
    """[..., 3] fp64 in [0.3, 0.7]."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([0.5 + 0.2 * np.sin(A[c] * x + PHI[c]) * np.cos(B[c] * y) for c in range(3)], -1)


def plane_pose():
    return IC.pose(TAU_PLANE)


def world_points(depth, T_w2c, intr=INTR):
    """[h,w,3] fp64: the world point of every pixel of the camera-z depth plane seen from T_w2c (pixel centre 0)."""
    d = np.asarray(depth, np.float64)
    h, w = d.shape
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    X = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], -1)
    T = np.asarray(T_w2c, np.float64)
    return (X - T[:3, 3]) @ T[:3, :3]          # R^T (X - t), row-wise


def painted(depth, T_w2c, intr=INTR, chw=True):
    """The texture of the world point behind every pixel: fp32 [3,h,w] (a camera's image) or [h,w,3] (a ray cast's colour)."""
    P = world_points(depth, T_w2c, intr)
    rgb = torch.from_numpy(texture(P[..., 0], P[..., 1]).astype(np.float32))
    return rgb.permute(2, 0, 1).contiguous() if chw else rgb


@functools.lru_cache(maxsize=None)
def plane_model(h=H, w=W, intr=INTR):
    """The analytic model at T_model = I: icp_cases.plane_model with the texture as "color" [h,w,3]."""
    n = torch.zeros(h, w, 3)
    n[..., 2] = -1.0
    depth = torch.full((h, w), PLANE_Z)
    return {"depth": depth, "normal": n, "color": painted(depth, np.eye(4), intr, chw=False)}


@functools.lru_cache(maxsize=None)
def plane_frame(h=H, w=W, intr=INTR):
    """(depth [h,w], image [3,h,w], sensor normal [3,h,w]) of the plane seen from plane_pose(): every depth is exactly 1.5."""
    depth = torch.full((h, w), PLANE_Z)
    n = torch.zeros(3, h, w)
    n[2] = -1.0
    return depth, painted(depth, plane_pose(), intr), n


def plane_depth(T_w2c, h=H, w=W, intr=INTR):
    """The camera-z depth [h,w] fp32 of the plane z = 1.5 from any pose: the ray centre + s R^T (rx, ry, 1) meets it at
    s = (1.5 - centre_z) / (R^T ray)_z, and s is the camera-z depth because the ray has z = 1 in the camera frame."""
    T = np.asarray(T_w2c, np.float64)
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    centre, dirs = -T[:3, :3].T @ T[:3, 3], ray @ T[:3, :3]
    return torch.from_numpy(((PLANE_Z - centre[2]) / dirs[..., 2]).astype(np.float32))


# The fusion views are wider than the tracked view (110 x 75 at the same f: 2.75 m x 1.9 m on the plane, the whole volume):
# a ray cast darkens the colour where it interpolates into voxels no view has weighted, so the border of the fused region
# must lie outside the 70 x 45 model view.
FUSE_H, FUSE_W, FUSE_INTR = 75, 110, (60.0, 60.0, 54.5, 37.0)


def fusion_views(scene):
    """[(T fp64 [4,4], depth, image [3,.,.], intrinsics)] of icp_cases.fusion_poses(): three coloured 110 x 75 views of the
    textured plane ("plane") or of the textured wavy surface ("wavy")."""
    out = []
    for T in IC.fusion_poses():
        depth = plane_depth(T, FUSE_H, FUSE_W, FUSE_INTR) if scene == "plane" else IC.surface_depth(T, FUSE_H, FUSE_W, FUSE_INTR)
        out.append((T, depth, painted(depth, T, FUSE_INTR), FUSE_INTR))
    return out


@functools.lru_cache(maxsize=None)
def plane_mirror(photo_weight, levels):
    from monogs_amd import icp
    depth, image, sn = plane_frame()
    return icp.align_numpy(plane_model(), depth, INTR, np.eye(4, dtype=np.float32), levels=levels, sensor_normal=sn,
                           image=image, photo_weight=photo_weight)


@functools.lru_cache(maxsize=None)
def wavy_model():
    """icp_cases.model_planes() with the texture as "color" [3,H,W] (the other colour layout)."""
    m = IC.model_planes()
    return {"depth": m["depth"], "normal": m["normal"], "color": painted(m["depth"], np.eye(4))}


@functools.lru_cache(maxsize=None)
def wavy_image():
    return painted(IC.frame_depth(), IC.true_pose())


@functools.lru_cache(maxsize=None)
def wavy_mirror(photo_weight, levels):
    from monogs_amd import icp
    return icp.align_numpy(wavy_model(), IC.frame_depth(), INTR, np.eye(4, dtype=np.float32), levels=levels,
                           sensor_normal=IC.sensor_normal(), image=wavy_image(), photo_weight=photo_weight)


def same_result(got, want):
    """icp_cases.same_result, and the intensity planes bit for bit."""
    ok = IC.same_result(got, want)
    for name in ("intensity", "model_intensity"):
        a, b = got[name].cpu().numpy().view(np.int32), want[name].numpy().view(np.int32)
        if not np.array_equal(a, b):
            print(f"{name} differs at {int((a != b).sum())} of {a.size} values")
            ok = False
    return ok
