"""Scenes, views and mirror runs shared by test_cpu_sparse_tsdf.py and test_gpu_sparse_tsdf.py.

Images are 70 x 45 at f = 60.  Voxel sizes are chosen so that a case holds few bricks: at 0.05 a brick is 0.4 wide, and
the surface a view sees 1.2 - 1.7 in front of it spans about 5 x 3 bricks, two or three deep.  Every mirror result is
computed once (lru_cache) and handed out read-only by convention: callers clone what they change."""
import functools

import numpy as np
import torch

import tsdf_cases as K

H, W = 45, 70
FX, FY, CX, CY = 60.0, 60.0, 34.5, 22.0

# ---- the view sequence of the allocation / capacity / integration tests ---------------------------------------------
VS = 0.05
ORIGIN = (0.013, -0.02, 1.5)          # the surface lies around z = 1.2 .. 1.7 and x = -0.9 .. 0.9: both signs on x, y, z
ORIGIN_POSITIVE = (0.013 - 3.2, -0.02 - 1.6, 1.5 - 1.2)      # 8, 4 and 3 bricks lower: every brick coordinate is >= 0
MAX_BRICKS = 400                      # the four views hold about 240
MAX_WEIGHT = 2.0
VIEW_KW = dict(depth_max=2.5, z_near=0.05)


def view_planes():
    """(depth, opacity, image) with 0, NaN, inf, over-depth_max and low-opacity patches (test_gpu_tsdf.make_planes)."""
    g = torch.Generator().manual_seed(3)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 1.45 + 0.12 * torch.sin(u / 9.0) * torch.cos(v / 7.0)
    depth[3:6, 10:20] = 0.0
    depth[20:23, 30:40] = float("nan")
    depth[30:34, 5:15] = float("inf")
    depth[10:14, 50:60] = 3.0                       # over depth_max
    opacity = 0.93 + 0.07 * torch.rand(H, W, generator=g)
    opacity[40:43, 20:30] = 0.0
    opacity[25:27, 60:66] = float("nan")
    image = torch.rand(3, H, W, generator=g)
    return depth, opacity, image


def views():
    """(T_w2c, weight, allocate): from outside, from inside the band of the first view's surface, facing away, the first
    again (with max_weight 2 the clamp of the stored weight is live).  The view facing away is integrated into the
    existing bricks only (allocate=False): it sees none of them, so every brick is culled and nothing may change.  (A
    sparse volume has no box to face away from: ALLOCATING from that pose with the same depth plane would simply map what
    lies behind the first camera.)"""
    from monogs_amd.pose import SE3_exp
    T0 = SE3_exp(torch.tensor([0.04, -0.03, 0.0, 0.08, -0.12, 0.05]))
    T0[:3, 3] = -T0[:3, :3] @ torch.tensor([0.1, -0.05, 0.0])
    T1 = SE3_exp(torch.tensor([0.0, 0.0, 0.0, -0.05, 0.6, 0.02]))
    T1[:3, 3] = -T1[:3, :3] @ torch.tensor([-0.6, 0.05, 1.42])            # on the first surface, looking along it
    T2 = torch.eye(4)
    T2[0, 0] = T2[2, 2] = -1.0
    T2[:3, 3] = -T2[:3, :3] @ torch.tensor([0.0, 0.0, -0.5])              # looks away from everything
    return [(T0, 1.0, True), (T1, 1.0, True), (T2, 1.0, False), (T0, 1.5, True)]


def view_inputs(with_opacity, with_image):
    depth, opacity, image = view_planes()
    kw = dict(VIEW_KW)
    if with_opacity:
        kw.update(opacity=opacity, normalize=True, min_opacity=0.95)
        depth = depth * opacity                     # the forward's depth is the unnormalised blend
    return depth, kw, (image if with_image else None)


@functools.lru_cache(maxsize=None)
def mirror_run(max_bricks, with_opacity, with_image, origin=ORIGIN, vs=VS):
    """The four views through the mirrors: a list of steps (bricks int32 [B,3], dropped, out_of_range, tsdf, weight,
    color) - the state AFTER each view, dropped / out_of_range summed as the device sums them."""
    from monogs_amd import sparse_tsdf as ST
    depth, kw, image = view_inputs(with_opacity, with_image)
    trunc = 4.0 * vs
    bricks = np.zeros((0, 3), np.int32)
    t = torch.ones(max_bricks, 512)
    w = torch.zeros(max_bricks, 512)
    c = torch.zeros(3, max_bricks, 512)
    dropped = out = 0
    steps = []
    for T, vw, allocate in views():
        if allocate:
            bricks, d, o = ST.allocate_bricks_torch(bricks, max_bricks, origin, vs, trunc, depth, T, FX, FY, CX, CY, **kw)
            dropped, out = dropped + d, out + o
        ST.integrate_bricks_torch(bricks, t, w, c, origin, vs, trunc, depth, T, FX, FY, CX, CY, image=image,
                                  view_weight=vw, max_weight=MAX_WEIGHT, **kw)
        steps.append((bricks.copy(), dropped, out, t.clone(), w.clone(), c.clone()))
    return steps


# ---- extraction: a sphere centred on a brick corner -----------------------------------------------------------------
CORNER_LO = (-8, -16, 8)                      # brick-aligned: bricks bx in {-1, 0}, by in {-2, -1}, bz in {1, 2}
CORNER_DIMS = (16, 16, 16)
CORNER_C, CORNER_R = (8.13, 7.91, 8.2), 6.3   # in the box's own lattice units: the corner shared by its eight bricks


def corner_sphere():
    return K.sphere_volume(CORNER_DIMS, c=CORNER_C, r=CORNER_R)


def box_bricks(lo, dims):
    """The bricks a box touches, x fastest: SparseTSDFVolume.from_dense's default list."""
    blo = [l // 8 for l in lo]
    nb = [(l + d - 1) // 8 + 1 - b for l, d, b in zip(lo, dims, blo)]
    bz, by, bx = np.meshgrid(*(np.arange(nb[a]) + blo[a] for a in (2, 1, 0)), indexing="ij")
    return np.stack([bx, by, bz], -1).reshape(-1, 3)


def brick_rows(planes, lo, bricks):
    """(tsdf [B,512], weight [B,512], color [3,B,512]) of `bricks` cut out of dense planes whose first point is `lo`
    (NumPy; outside the box: tsdf 1, weight 0, colour 0)."""
    t, w, c = planes
    nz, ny, nx = t.shape
    out_t = np.ones((len(bricks), 8, 8, 8), np.float32)
    out_w = np.zeros((len(bricks), 8, 8, 8), np.float32)
    out_c = np.zeros((3, len(bricks), 8, 8, 8), np.float32)
    for n, (bx, by, bz) in enumerate(np.asarray(bricks)):
        for lk in range(8):
            k = 8 * bz + lk - lo[2]
            if not 0 <= k < nz:
                continue
            for lj in range(8):
                j = 8 * by + lj - lo[1]
                if not 0 <= j < ny:
                    continue
                i0 = 8 * bx - lo[0]
                a, b = max(i0, 0), min(i0 + 8, nx)
                if a >= b:
                    continue
                out_t[n, lk, lj, a - i0:b - i0] = t[k, j, a:b]
                out_w[n, lk, lj, a - i0:b - i0] = w[k, j, a:b]
                out_c[:, n, lk, lj, a - i0:b - i0] = c[:, k, j, a:b]
    B = len(bricks)
    return out_t.reshape(B, 512), out_w.reshape(B, 512), out_c.reshape(3, B, 512)


# ---- more than 512 bricks: two trips of the one-workgroup scan -------------------------------------------------------
TRIP_DIMS = (72, 64, 72)                      # 9 x 8 x 9 = 648 bricks, 1296 block totals
TRIP_LO = (-24, 0, -40)
TRIP_C, TRIP_R = (35.37, 31.61, 38.13), 24.3  # brick 512 lies in the layer k in [56, 64): the surface reaches k = 62


def trip_sphere():
    return K.sphere_volume(TRIP_DIMS, c=TRIP_C, r=TRIP_R)


# ---- beyond the dense limit ------------------------------------------------------------------------------------------
FAR_CENTRE = (-1500.37, 900.61, 1700.13)      # lattice units
FAR_R = 12.2
FAR_LO = (-1517, 884, 1683)                   # not brick-aligned
FAR_DIMS = (34, 34, 35)


def far_sphere():
    c = tuple(FAR_CENTRE[a] - FAR_LO[a] for a in range(3))
    return K.sphere_volume(FAR_DIMS, c=c, r=FAR_R)


# ---- a sphere seen from six views: sparse against dense --------------------------------------------------------------
SIX_VS = 0.05
SIX_ORIGIN = (0.0, 0.0, 0.0)
SIX_DIMS = (80, 80, 80)                       # the dense box: 4 m around the "map"
SIX_CENTRE = (2.013, 1.987, 2.021)
SIX_RADIUS = 0.5                              # 10 voxels
SIX_DISTANCE = 1.5                            # camera centre to sphere centre


def six_views():
    """[(T_w2c, depth [H,W])]: cameras on the six axis directions looking at the sphere's centre; the depth is the
    analytic z-depth of the first hit of the pixel's ray, 0 where the ray misses."""
    out = []
    c = torch.tensor(SIX_CENTRE, dtype=torch.float64)
    for axis in range(3):
        for sign in (-1.0, 1.0):
            fwd = torch.zeros(3, dtype=torch.float64)
            fwd[axis] = -sign                                   # from the camera to the centre
            up = torch.zeros(3, dtype=torch.float64)
            up[(axis + 1) % 3] = 1.0
            right = torch.linalg.cross(up, fwd)
            R = torch.stack([right, torch.linalg.cross(fwd, right), fwd])      # rows: the camera's axes in the world
            pos = c - SIX_DISTANCE * fwd
            T = torch.eye(4, dtype=torch.float64)
            T[:3, :3] = R
            T[:3, 3] = -R @ pos
            v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
            d = torch.stack([(u - CX) / FX, (v - CY) / FY, torch.ones_like(u)], -1)      # z-normalised ray
            oc = torch.tensor([0.0, 0.0, SIX_DISTANCE], dtype=torch.float64)             # the centre in the camera
            a = (d * d).sum(-1)
            b = d @ oc
            disc = b * b - a * (SIX_DISTANCE ** 2 - SIX_RADIUS ** 2)
            z = torch.where(disc > 0, (b - torch.sqrt(disc.clamp_min(0))) / a, torch.zeros_like(a))
            out.append((T.float(), z.float()))
    return out


@functools.lru_cache(maxsize=None)
def six_views_mirror():
    """(dense planes, bricks, brick planes) of the six views through integrate_torch and through the brick mirrors."""
    from monogs_amd import sparse_tsdf as ST
    from monogs_amd.tsdf import integrate_torch
    nx, ny, nz = SIX_DIMS
    dense = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    cap = 400
    rows = (torch.ones(cap, 512), torch.zeros(cap, 512), torch.zeros(3, cap, 512))
    bricks = np.zeros((0, 3), np.int32)
    trunc = 4.0 * SIX_VS
    for T, depth in six_views():
        integrate_torch(*dense, SIX_ORIGIN, SIX_VS, trunc, depth, T, FX, FY, CX, CY)
        bricks, dropped, out = ST.allocate_bricks_torch(bricks, cap, SIX_ORIGIN, SIX_VS, trunc, depth, T, FX, FY, CX, CY)
        assert dropped == 0 and out == 0
        ST.integrate_bricks_torch(bricks, *rows, SIX_ORIGIN, SIX_VS, trunc, depth, T, FX, FY, CX, CY)
    return dense, bricks, rows


# ---- comparisons -----------------------------------------------------------------------------------------------------
def vertex_set(verts, colors):
    """The rows (x, y, z, r, g, b) as bit patterns, sorted."""
    a = np.concatenate([np.asarray(verts, np.float32), np.asarray(colors, np.float32)], 1).view(np.uint32)
    return a[np.lexsort(a.T[::-1])]


def face_position_set(verts, faces):
    """Every face as the bit patterns of its three positions, rotated to start at the smallest, rows sorted."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return np.zeros((0, 9), np.uint32)
    key = np.unique(np.asarray(verts, np.float32).view(np.uint32), axis=0, return_inverse=True)[1].reshape(-1)   # rank of a position
    s = np.argmin(key[f], axis=1)
    r = np.arange(f.shape[0])
    g = np.stack([f[r, s], f[r, (s + 1) % 3], f[r, (s + 2) % 3]], 1)
    rows = np.asarray(verts, np.float32).view(np.uint32)[g].reshape(-1, 9)
    return rows[np.lexsort(rows.T[::-1])]
