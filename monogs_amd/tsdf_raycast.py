"""Ray cast of the TSDF volumes: depth, normal and colour of the fused surface at a pose, straight from the planes of a
tsdf.TSDFVolume or a sparse_tsdf.SparseTSDFVolume (csrc/tsdf_raycast.hip; the contract is in include/monogs_raster.h and
DESIGN.md "Ray cast of the volumes").

    planes = vol.raycast_view(camera, z_far=4.0)             # dict(depth, normal, color, hit_step) on the device
    frame = raycast_frame(vol, camera, "shaded", z_far=4.0)  # uint8 [H,W,3]: a picture of the volume without a mesh
    err = volume_depth_l1(vol, views, sensor_depths, z_far=4.0)

No mesh, no host read, two launches at most (the neighbour table of a sparse volume, then the march), so it can run
while `run_sequence(mesh_volume=vol)` is still filling the volume.

The mirror `raycast_torch` IS the contract: brute force over every sample of every ray, every product, sum, difference,
quotient and root one torch operation, i.e. one fp32 rounding.  The device equals it bit for bit.  It needs no GPU.
There is no CPU fall-back behind `raycast`: off the GPU the volumes raise."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _cabi
from ._device import stream_ptr
from .mesh_render import _quantise, view_tuple
from .tsdf import _f32

FRAMES = ("camera", "world")
FRAME_MODES = ("shaded", "normal", "color", "depth")
MAX_STEPS = _cabi.RAYCAST_MAX_STEPS
INDEX_LIMIT = float(2 ** 23)


def march_steps(voxel_size, z_near, z_far, step=0.5, frame="camera"):
    """(dz, N) of a ray cast, or ValueError: dz = f32(step) * f32(voxel_size), one rounding; N = floor((z_far - z_near)
    / dz) + 1 in fp64 from the fp32 values; 2 <= N <= 2^20."""
    if frame not in FRAMES:
        raise ValueError(f"raycast: frame must be one of {FRAMES}, got {frame!r}")
    if z_far is None:
        raise ValueError("raycast: z_far is required")
    if not float(step) > 0:
        raise ValueError(f"raycast: step {step} must be positive (it is in voxels)")
    if not float(voxel_size) > 0:
        raise ValueError("raycast: voxel_size must be positive")
    zn, zf = np.float32(z_near), np.float32(z_far)
    if not zf > zn:
        raise ValueError(f"raycast: z_far {z_far} must exceed z_near {z_near}")
    dz = np.float32(step) * np.float32(voxel_size)
    if not (dz > 0 and np.isfinite(dz) and np.isfinite(zf) and np.isfinite(zn)):
        raise ValueError("raycast: step * voxel_size, z_near and z_far must be finite, the step positive in fp32")
    N = math.floor((float(zf) - float(zn)) / float(dz)) + 1
    if N < 2:
        raise ValueError(f"raycast: {N} sample along a ray: z_far - z_near must hold one step of {float(dz)}")
    if N > MAX_STEPS:
        raise ValueError(f"raycast: {N} samples along a ray exceed 2^20: raise step or bring z_far closer")
    return float(dz), int(N)


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def raycast_torch(tsdf, weight, color, origin, voxel_size, lo, T_w2c, fx, fy, cx, cy, H, W, z_near=0.2, z_far=None,
                  step=0.5, min_weight=1.0, frame="camera"):
    """mgs_tsdf_raycast / mgs_sparse_tsdf_raycast in fp32 torch on the CPU: dict(depth [H,W], normal [H,W,3], color
    [H,W,3], hit_step int32 [H,W]).  The planes tsdf / weight [nz,ny,nx] and color [3,nz,ny,nx] (or None) are dense, their
    first point has the lattice index `lo` of the lattice at `origin`: what SparseTSDFVolume.to_dense and
    sparse_tsdf.bricks_to_box give (with origin the VOLUME's), and with lo = (0,0,0) a TSDFVolume's own planes.  A point
    outside the planes has weight 0.  Brute force over all n, vectorised over the pixels."""
    dz_, N = march_steps(voxel_size, z_near, z_far, step, frame)
    if tsdf is None or weight is None:
        raise ValueError("raycast_torch: tsdf and weight planes are required")
    f = _f32
    t = torch.as_tensor(tsdf).detach().to("cpu", torch.float32)
    nz, ny, nx = (int(v) for v in t.shape)
    tf = t.reshape(-1)
    wf = torch.as_tensor(weight).detach().to("cpu", torch.float32).reshape(-1)
    cf = None if color is None else torch.as_tensor(color).detach().to("cpu", torch.float32).reshape(3, -1)
    T = torch.as_tensor(T_w2c).detach().to("cpu", torch.float32)
    H, W = int(H), int(W)
    lo = [int(v) for v in lo]
    vs, dz, zn, mw = f(voxel_size), f(dz_), f(z_near), f(min_weight)
    pix = torch.arange(H * W)
    xn = ((pix % W).float() - f(cx)) / f(fx)
    yn = ((pix // W).float() - f(cy)) / f(fy)
    dims = (nx, ny, nz)

    def lattice(z):
        q = (xn * z - T[0, 3], yn * z - T[1, 3], z - T[2, 3])
        out = []
        for a in range(3):
            p = (T[0, a] * q[0] + T[1, a] * q[1]) + T[2, a] * q[2]
            out.append((p - f(origin[a])) / vs)
        return out

    def corners(l):
        bf = [torch.floor(v) for v in l]
        valid = torch.ones(H * W, dtype=torch.bool)
        for v in bf:
            valid = valid & (v.abs() < INDEX_LIMIT)                 # in float: false for a NaN
        b = [torch.where(valid, v, torch.zeros(())).long() - lo[a] for a, v in enumerate(bf)]
        fr = [l[a] - bf[a] for a in range(3)]
        idx = []
        for c in range(8):
            p = [b[a] + ((c >> a) & 1) for a in range(3)]
            inside = valid
            for a in range(3):
                inside = inside & (p[a] >= 0) & (p[a] < dims[a])
            lin = torch.where(inside, (p[2] * ny + p[1]) * nx + p[0], torch.zeros((), dtype=torch.long))
            valid = inside & (wf[lin] >= mw)                        # false for a NaN weight
            idx.append(lin)
        return valid, idx, fr

    def interp(plane, idx, fr):
        v = [plane[i] for i in idx]
        x = [v[2 * e] + fr[0] * (v[2 * e + 1] - v[2 * e]) for e in range(4)]
        y = [x[2 * e] + fr[1] * (x[2 * e + 1] - x[2 * e]) for e in range(2)]
        return y[0] + fr[2] * (y[1] - y[0])

    def sample(l):
        valid, idx, fr = corners(l)
        return valid, interp(tf, idx, fr)

    hit_step = torch.full((H * W,), -1, dtype=torch.int32)
    f_prev, f_hit = torch.zeros(H * W), torch.zeros(H * W)
    done = torch.zeros(H * W, dtype=torch.bool)
    prev_ok, prev = torch.zeros(H * W, dtype=torch.bool), torch.zeros(H * W)
    for n in range(N):
        ok, val = sample(lattice(zn + f(n) * dz))
        both = ok & prev_ok & ~done
        hit = both & (prev > 0) & (val <= 0)
        back = both & (prev < 0) & (val > 0)
        hit_step[hit] = n
        hit_step[back] = -2
        f_prev = torch.where(hit, prev, f_prev)
        f_hit = torch.where(hit, val, f_hit)
        done = done | hit | back
        prev_ok, prev = ok, val
        if bool(done.all()):
            break
    hit = hit_step >= 0
    zero = torch.zeros(())
    tt = f_prev / (f_prev - f_hit)
    depth = (zn + (hit_step - 1).float() * dz) + tt * dz
    l = lattice(depth)
    good, idx, fr = corners(l)
    good = good & hit
    col = [interp(cf[ch], idx, fr) if cf is not None else torch.zeros(H * W) for ch in range(3)]
    g = []
    for a in range(3):
        lp, lm = list(l), list(l)
        lp[a], lm[a] = l[a] + f(1.0), l[a] - f(1.0)
        okp, vp = sample(lp)
        okm, vm = sample(lm)
        good = good & okp & okm
        g.append(vp - vm)
    # the correctly rounded fp32 root (surface.depth_normal_torch)
    length = torch.sqrt(((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).double()).float()
    good = good & (length > 0) & torch.isfinite(length)
    nw = [c / length for c in g]
    if frame == "camera":
        nw = [(T[r, 0] * nw[0] + T[r, 1] * nw[1]) + T[r, 2] * nw[2] for r in range(3)]
    return {"depth": torch.where(hit, depth, zero).reshape(H, W),
            "normal": torch.stack([torch.where(good, c, zero) for c in nw], -1).reshape(H, W, 3),
            "color": torch.stack([torch.where(good, c, zero) for c in col], -1).reshape(H, W, 3),
            "hit_step": hit_step.reshape(H, W)}


def raycast_bricks_torch(bricks, tsdf, weight, color, origin, voxel_size, T_w2c, fx, fy, cx, cy, H, W, **kw):
    """raycast_torch for the brick list `bricks` [B,3] and the first B rows of the pool planes tsdf / weight [cap,512],
    color [3,cap,512]: the ray cast of the dense planes of the list's bounding box (it materialises that box)."""
    from .sparse_tsdf import bricks_to_box
    lo, t, w, col, _ = bricks_to_box(bricks, np.asarray(tsdf), np.asarray(weight), None if color is None else np.asarray(color))
    return raycast_torch(t, w, col, origin, voxel_size, lo, T_w2c, fx, fy, cx, cy, H, W, **kw)


def _background(what, mode, background):
    if mode not in FRAME_MODES:
        raise ValueError(f"{what}: mode must be one of {FRAME_MODES}, got {mode!r}")
    bg = _quantise(np.asarray(background, np.float32).reshape(-1))
    if bg.shape != (3,):
        raise ValueError(f"{what}: background is (r, g, b) in [0, 1]")
    return bg


def raycast_frame_numpy(planes, view, mode: str = "shaded", background=(0.0, 0.0, 0.0), depth_range=(0.2, 4.0)):
    """mgs_raycast_shade in NumPy: uint8 [H,W,3] from the planes of a ray cast in the CAMERA frame.  A miss gets
    `background`; the channels are quantised as the viewer's rgb frames are.  "shaded" and "normal" are
    mesh_render.render_mesh_frame's rules on the ray cast's normal, "color" is the colour plane, "depth" is the viewer's
    jet with t = (d - lo) / (hi - lo) over `depth_range` = the ray cast's (z_near, z_far)."""
    bg = _background("raycast_frame_numpy", mode, background)
    _, fx, fy, cx, cy, H, W = view_tuple(view)
    to_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    hit = to_np(planes["hit_step"]).reshape(H, W) >= 0
    out = np.empty((H, W, 3), np.uint8)
    out[:] = bg
    with np.errstate(all="ignore"):
        if mode == "color":
            rgb = _quantise(to_np(planes["color"]).astype(np.float32).reshape(H, W, 3))
        elif mode == "depth":
            from .viewer import JET_LUT
            lo, hi = np.float32(depth_range[0]), np.float32(depth_range[1])
            t = (to_np(planes["depth"]).astype(np.float32).reshape(H, W) - lo) / (hi - lo)
            at = np.minimum(255, (np.clip(np.where(np.isnan(t), np.float32(0), t), np.float32(0), np.float32(1))
                                  * np.float32(256.0)).astype(np.int64))
            rgb = np.where(np.isnan(t)[..., None], np.uint8(0), JET_LUT.reshape(256, 3)[at])
        else:
            n = to_np(planes["normal"]).astype(np.float32).reshape(H, W, 3)
            nc = [n[..., 0], n[..., 1], n[..., 2]]
            if mode == "shaded":
                grey = _quantise(np.float32(0.25) + np.float32(0.75) * np.abs(nc[2]))
                rgb = np.stack([grey, grey, grey], -1)
            else:
                rx = ((np.arange(W, dtype=np.float32) - np.float32(cx)) / np.float32(fx))[None, :]
                ry = ((np.arange(H, dtype=np.float32) - np.float32(cy)) / np.float32(fy))[:, None]
                away = ((nc[0] * rx + nc[1] * ry) + nc[2]) > 0
                rgb = np.stack([_quantise(np.float32(0.5) * np.where(away, -c, c) + np.float32(0.5)) for c in nc], -1)
    return np.where(hit[:, :, None], rgb, out).astype(np.uint8)


# ---- the device ------------------------------------------------------------------------------------------------------
def _is_sparse(vol) -> bool:
    return hasattr(vol, "brick_coords")


def _fill_view(v, T, fx, fy, cx, cy, H, W, z_near, dz, N, min_weight, frame, skip, out):
    v.width, v.height, v.num_steps = W, H, N
    v.frame = _cabi.RAYCAST_FRAME_CAMERA if frame == "camera" else _cabi.RAYCAST_FRAME_WORLD
    v.skip = 1 if skip else 0
    v.fx, v.fy, v.cx, v.cy = float(fx), float(fy), float(cx), float(cy)
    v.z_near, v.dz, v.min_weight = float(z_near), dz, float(min_weight)
    v.T = T.data_ptr()
    v.depth, v.normal, v.color, v.hit_step = (out[k].data_ptr() for k in ("depth", "normal", "color", "hit_step"))
    if "evaluated" in out:
        v.evaluated = out["evaluated"].data_ptr()


def neighbor_table(vol, rebuild=None):
    """(table, build): the [max_bricks,27] neighbour table the sparse ray cast keeps on the volume, and whether the next
    ray cast must write it.  The rule: the volume counts the calls that can add bricks (`brick_epoch`: an allocating
    integrate, from_dense, reset); the table is written again when that count differs from the one it was written at.
    `rebuild=True` forces it - for a caller who filled brick_coords and the map by hand."""
    table = getattr(vol, "_raycast_table", None)
    if table is None or table.numel() != 27 * vol.max_bricks or table.device != vol.dev:
        nbytes = int(_cabi.lib().mgs_sparse_tsdf_raycast_scratch_bytes(vol.max_bricks))
        if nbytes == 0:
            raise ValueError("raycast: unsupported max_bricks")
        table = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=vol.dev)
        vol._raycast_table, vol._raycast_epoch = table, None
    build = bool(rebuild) or vol._raycast_epoch != vol.brick_epoch
    return table, build


def raycast(vol, T_w2c, fx, fy, cx, cy, H, W, z_near=0.2, z_far=None, step=0.5, min_weight=1.0, frame="camera",
            skip=True, rebuild_table=None, out=None, count_evaluated=False):
    """dict(depth [H,W], normal [H,W,3], color [H,W,3], hit_step int32 [H,W]) on the device of `vol` (a TSDFVolume or a
    SparseTSDFVolume): the fused surface seen from T_w2c.  One launch for a dense volume; for a sparse one a launch over
    the pool writes the neighbour table first when bricks were added since the last ray cast (neighbor_table).  No host
    read.  `step` is in voxels, `z_far` is required; depth 0 and hit_step -1 (ran out) / -2 (back face) mark a miss.
    `frame`: "camera" turns the normal into the camera frame, "world" leaves it.  `skip=False` evaluates every sample:
    the same bits, slower.  `out`: a dict of the four planes to write into (contiguous, of these shapes, on the device)
    instead of new ones.  `count_evaluated=True` adds the plane `evaluated` int32 [H,W], the samples the march evaluated
    on each ray: a diagnostic for profiles, the one output that depends on `skip`."""
    dz, N = march_steps(vol.voxel_size, z_near, z_far, step, frame)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or 3 * H * W > 2 ** 31 - 1:
        raise ValueError(f"raycast: {H} x {W} pixels: positive, and 3 H W must stay below 2^31")
    dev = vol.dev
    T = torch.as_tensor(T_w2c).detach().to(dev, torch.float32).contiguous()
    if tuple(T.shape) != (4, 4):
        raise ValueError("T_w2c must be [4,4]")
    shapes = {"depth": ((H, W), torch.float32), "normal": ((H, W, 3), torch.float32), "color": ((H, W, 3), torch.float32),
              "hit_step": ((H, W), torch.int32)}
    if count_evaluated:
        shapes["evaluated"] = ((H, W), torch.int32)
    if out is None:
        out = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items()}
    for k, (s, d) in shapes.items():
        t = out[k]
        if t.device != dev or t.dtype != d or tuple(t.shape) != s or not t.is_contiguous():
            raise ValueError(f"raycast: out[{k!r}] must be a contiguous {d} tensor {s} on {dev}")
    L = _cabi.lib()
    if _is_sparse(vol):
        a = _cabi.SparseTsdfRaycastArgs()
        vol._volume(a.vol)
        table, build = neighbor_table(vol, rebuild_table)
        a.scratch, a.build_table = table.data_ptr(), 1 if build else 0
        _fill_view(a.view, T, fx, fy, cx, cy, H, W, z_near, dz, N, min_weight, frame, skip, out)
        _cabi.check(L.mgs_sparse_tsdf_raycast(C.byref(a), stream_ptr(dev)), "mgs_sparse_tsdf_raycast")
        vol._raycast_epoch = vol.brick_epoch
    else:
        a = _cabi.TsdfRaycastArgs()
        a.nx, a.ny, a.nz = vol.nx, vol.ny, vol.nz
        a.origin[0], a.origin[1], a.origin[2] = vol.origin
        a.voxel_size = vol.voxel_size
        shape = (vol.nz, vol.ny, vol.nx)
        a.tsdf, a.weight = vol._plane(vol.tsdf, shape, "tsdf"), vol._plane(vol.weight, shape, "weight")
        a.color = vol._plane(vol.color, (3,) + shape, "color")
        _fill_view(a.view, T, fx, fy, cx, cy, H, W, z_near, dz, N, min_weight, frame, skip, out)
        _cabi.check(L.mgs_tsdf_raycast(C.byref(a), stream_ptr(dev)), "mgs_tsdf_raycast")
    del T      # held until the launches were enqueued; the allocator orders its reuse on this stream
    return out


def raycast_view(vol, camera, **kw):
    """raycast at a view: (T_w2c, fx, fy, cx, cy, H, W) or a camera object (mesh_render.view_tuple)."""
    T, fx, fy, cx, cy, H, W = view_tuple(camera)
    return raycast(vol, T, fx, fy, cx, cy, H, W, **kw)


def shade(planes, view, mode: str = "shaded", background=(0.0, 0.0, 0.0), depth_range=(0.2, 4.0)):
    """uint8 [H,W,3] on the device from the planes of a CAMERA-frame ray cast: one launch (raycast_frame_numpy is the
    mirror)."""
    bg = _background("raycast_frame", mode, background)
    _, fx, fy, cx, cy, H, W = view_tuple(view)
    dev = planes["depth"].device
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    a = _cabi.RaycastShadeArgs()
    a.width, a.height = W, H
    a.mode = FRAME_MODES.index(mode)       # MGS_RAYCAST_SHADE_* in this order
    a.fx, a.fy, a.cx, a.cy = fx, fy, cx, cy
    a.depth_lo, a.depth_hi = float(depth_range[0]), float(depth_range[1])
    a.background[0], a.background[1], a.background[2] = (int(b) for b in bg)
    a.depth, a.normal, a.color, a.hit_step = (planes[k].data_ptr() for k in ("depth", "normal", "color", "hit_step"))
    lut = None
    if mode == "depth":
        from .viewer import _lut
        lut = _lut(dev).contiguous()
        a.lut = lut.data_ptr()
    a.out = out.data_ptr()
    _cabi.check(_cabi.lib().mgs_raycast_shade(C.byref(a), stream_ptr(dev)), "mgs_raycast_shade")
    del lut
    return out


def raycast_frame(vol, view, mode: str = "shaded", background=(0.0, 0.0, 0.0), z_near=0.2, z_far=None, **kw):
    """uint8 [H,W,3] on the device: a picture of the volume at `view` without a mesh - the ray cast, then ONE launch.
    The modes are render_mesh_frame's: "shaded" (headlight on the normal), "normal", "color" (the fused colour) and
    "depth" (jet between z_near and z_far).  A ray that misses gets `background`."""
    _background("raycast_frame", mode, background)
    if kw.get("frame", "camera") != "camera":
        raise ValueError('raycast_frame: the frame is shaded from camera-frame normals; frame must be "camera"')
    planes = raycast_view(vol, view, z_near=z_near, z_far=z_far, **kw)
    return shade(planes, view, mode, background, (z_near, z_far))


def volume_depth_l1(vol, views, depths, **kw):
    """The mean |ray cast - sensor| depth over the pixels where both are positive, over all `views` (what view_tuple
    accepts) and their depth planes `depths` [H,W]: the sensor-against-model depth error.  The sums stay on the device;
    ONE host read at the end.  Returns dict(l1, pixels); l1 is nan when no pixel has both."""
    views, depths = list(views), list(depths)
    if len(views) != len(depths):
        raise ValueError("volume_depth_l1: one depth plane per view")
    dev = vol.dev
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    for view, d in zip(views, depths):
        T, fx, fy, cx, cy, H, W = view_tuple(view)
        d = torch.as_tensor(d).detach().to(dev, torch.float32).reshape(H, W)
        z = raycast(vol, T, fx, fy, cx, cy, H, W, **kw)["depth"]
        both = (z > 0) & (d > 0)
        acc += torch.stack([torch.where(both, (z - d).abs(), torch.zeros((), device=dev)).sum(dtype=torch.float64),
                            both.sum().double()])
    s, n = (float(v) for v in acc.cpu())
    return {"l1": s / n if n > 0 else float("nan"), "pixels": int(n)}
