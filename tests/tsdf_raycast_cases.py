"""Volumes, poses and mirror runs shared by test_cpu_tsdf_raycast.py and test_gpu_tsdf_raycast.py, built with the
existing mirrors.  Every image is 70 x 45 at f = 60 (neither a multiple of the 8 x 8 tile); every mirror result is
computed once (lru_cache) and handed out read-only by convention."""
import functools

import numpy as np
import torch

import sparse_tsdf_cases as SC
import tsdf_cases as K

H, W = SC.H, SC.W
FX, FY, CX, CY = SC.FX, SC.FY, SC.CX, SC.CY
INTR = (FX, FY, CX, CY)


def pose(rotvec=(0.0, 0.0, 0.0), centre=(0.0, 0.0, 0.0)):
    """T_w2c of a camera at `centre` turned by exp(rotvec)."""
    from monogs_amd.pose import SE3_exp
    T = SE3_exp(torch.tensor([0.0, 0.0, 0.0] + [float(v) for v in rotvec]))
    T[:3, 3] = -T[:3, :3] @ torch.tensor([float(v) for v in centre])
    return T


# ---- the four views of sparse_tsdf_cases at voxel 0.05: about 240 bricks ---------------------------------------------
VIEWS_KW = dict(z_near=0.05, z_far=2.5)            # 99 samples of half a voxel


def views_bricks(step=-1):
    """(bricks, tsdf, weight, color rows) after view `step` of the four."""
    bricks, _, _, t, w, c = SC.mirror_run(SC.MAX_BRICKS, False, True)[step]
    return bricks, t, w, c


def views_poses():
    """The integration's four poses, then two no view had: a generic one, and one whose centre lies ON a brick face
    (y = origin_y, the principal row cy = 22 is an integer) looking along the lattice's z: the rays of that row run inside
    the plane between two layers of bricks, l_y = 0 up to rounding, and their neighbours graze it."""
    ps = [T for T, _, _ in SC.views()]
    ps.append(pose((0.1, 0.25, -0.07), (0.35, 0.1, 0.1)))
    ps.append(pose((0.0, 0.0, 0.0), (SC.ORIGIN[0], SC.ORIGIN[1], 0.1)))
    return ps


@functools.lru_cache(maxsize=None)
def views_mirror(p, frame="camera", step=-1):
    from monogs_amd.tsdf_raycast import raycast_bricks_torch
    bricks, t, w, c = views_bricks(step)
    return raycast_bricks_torch(bricks, t.numpy(), w.numpy(), c.numpy(), SC.ORIGIN, SC.VS, views_poses()[p], *INTR, H, W,
                                frame=frame, **VIEWS_KW)


# ---- the 24^3 sphere of tsdf_cases -----------------------------------------------------------------------------------
SPHERE_DIMS = (24, 24, 24)
SPHERE_KW = dict(z_near=0.2, z_far=2.0)            # 73 samples
SPHERE_WORLD = tuple(K.ORIGIN[a] + K.SPHERE_C[a] * K.VOXEL for a in range(3))


@functools.lru_cache(maxsize=None)
def sphere():
    return K.sphere_volume(SPHERE_DIMS)


def sphere_poses():
    """From outside (1.1 in front, a little off the axis and turned: rays enter and leave the box, some miss it), and from
    inside the sphere (every ray ends on a back face)."""
    c = SPHERE_WORLD
    return [pose((0.03, -0.05, 0.2), (c[0] + 0.07, c[1] - 0.05, c[2] - 1.1)), pose((0.2, 0.1, 0.0), (c[0] + 0.02, c[1], c[2] - 0.03))]


@functools.lru_cache(maxsize=None)
def sphere_mirror(p, frame="camera"):
    from monogs_amd.tsdf_raycast import raycast_torch
    return raycast_torch(*sphere(), K.ORIGIN, K.VOXEL, (0, 0, 0), sphere_poses()[p], *INTR, H, W, frame=frame, **SPHERE_KW)


# ---- the far sphere around lattice (-1500, 900, 1700) ----------------------------------------------------------------
FAR_KW = dict(z_near=0.2, z_far=2.6)
FAR_WORLD = tuple(K.ORIGIN[a] + SC.FAR_CENTRE[a] * K.VOXEL for a in range(3))


@functools.lru_cache(maxsize=None)
def far_sphere():
    return SC.far_sphere()


def far_poses():
    c = FAR_WORLD
    return [pose((0.0, 0.0, 0.0), (c[0], c[1], c[2] - 1.5)), pose((-0.4, 0.3, 0.1), (c[0] + 0.5, c[1] + 0.6, c[2] - 1.2))]


@functools.lru_cache(maxsize=None)
def far_mirror(p):
    from monogs_amd.tsdf_raycast import raycast_torch
    return raycast_torch(*far_sphere(), K.ORIGIN, K.VOXEL, SC.FAR_LO, far_poses()[p], *INTR, H, W, **FAR_KW)


# ---- a fronto-parallel plane -----------------------------------------------------------------------------------------
PLANE_VS, PLANE_D0 = 0.05, 1.0
PLANE_ORIGIN = (-1.0, -0.7, 0.6)
PLANE_DIMS = (40, 28, 16)                          # x in [-1, 0.95], y in [-0.7, 0.65], z in [0.6, 1.35]
PLANE_KW = dict(z_near=0.2, z_far=1.5)


@functools.lru_cache(maxsize=None)
def plane_volume():
    """(tsdf, weight, color) of ONE view of constant depth d0 at T = I through tsdf.integrate_torch, trunc = 4 vs."""
    from monogs_amd.tsdf import integrate_torch
    nx, ny, nz = PLANE_DIMS
    t, w, c = torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx)
    integrate_torch(t, w, c, PLANE_ORIGIN, PLANE_VS, 4.0 * PLANE_VS, torch.full((H, W), PLANE_D0), torch.eye(4), *INTR)
    return t, w, c


def bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def same_planes(a, b, show=True):
    """Every plane of two ray casts: the floats as int32 bits, hit_step exactly.  A mismatch is printed."""
    same = True
    for k in ("depth", "normal", "color", "hit_step"):
        x, y = torch.as_tensor(a[k]).detach().cpu(), torch.as_tensor(b[k]).detach().cpu()
        if k != "hit_step":
            x, y = bits(x), bits(y)
        if not torch.equal(x, y):
            bad = (x != y).reshape(H * W, -1).any(1).nonzero().reshape(-1)
            show and print(f"{k}: {len(bad)} pixels differ, first {bad[:6].tolist()}: "
                  f"{torch.as_tensor(a[k]).detach().cpu().reshape(H * W, -1)[bad[:3]].tolist()} against "
                  f"{torch.as_tensor(b[k]).detach().cpu().reshape(H * W, -1)[bad[:3]].tolist()}")
            same = False
    return same
