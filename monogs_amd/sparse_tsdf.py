"""Sparse TSDF volume: the lattice of tsdf.TSDFVolume without its box (csrc/sparse_tsdf.hip; the contract is in
include/monogs_raster.h and DESIGN.md "Sparse TSDF volume").

    vol = SparseTSDFVolume(origin=(0, 0, 0), voxel_size=0.005, max_bricks=200_000)
    for cam in keyframes:
        vol.integrate_view(gaussians, cam, background)       # allocates the bricks the view needs, then integrates
    verts, faces, colors = vol.extract_mesh()                # TWO host reads: the brick count, then (V, F)

The lattice is unbounded: point (i,j,k), any sign, lies at origin + (i,j,k) * voxel_size.  A brick is 8 x 8 x 8 points;
brick (bx,by,bz) holds i in [8 bx, 8 bx + 8) and likewise j and k, its coordinates lie in [-2^20, 2^20).  Storage is a
pool of `max_bricks` bricks: tsdf [cap,512] (initial 1), weight [cap,512] (initial 0), color [3,cap,512] (initial 0) -
the local index of a point is (lk * 8 + lj) * 8 + li - brick_coords int32 [cap,3], and a hash map brick key -> brick id.
Memory goes with the surface seen, not with the bounding box of the map, and the volume grows while a run goes on.

The contract in one sentence: a sparse volume is the dense volume with the same origin and voxel size in which every
point of an unallocated brick has weight 0.  The mirrors `allocate_bricks_torch`, `integrate_bricks_torch` and
`extract_mesh_bricks_numpy` restate that on brick lists with the roundings of tsdf.integrate_torch /
tsdf.extract_mesh_numpy; the device equals them bit for bit - brick list, planes, vertices and colours exactly, faces as
a set.  They need no GPU.  There is no CPU fall-back behind SparseTSDFVolume: off the GPU it raises."""
from __future__ import annotations

import ctypes as C
import itertools
import math
from typing import Optional

import numpy as np
import torch

from . import _cabi
from ._device import stream_ptr
from .tsdf import (SLOT_OF_CODE, SLOT_OFFSETS, TET_CORNERS, TET_EDGES, TET_FLIP, TET_TABLE, TSDFVolume, _f32)

BRICK = _cabi.SPARSE_TSDF_BRICK
BRICK_POINTS = BRICK ** 3
MAX_BRICKS = _cabi.SPARSE_TSDF_MAX_BRICKS
COORD_RANGE = _cabi.SPARSE_TSDF_COORD_RANGE


def check_max_bricks(max_bricks) -> int:
    n = int(max_bricks)
    if n < 1:
        raise ValueError(f"sparse TSDF volume: max_bricks {max_bricks} must be positive")
    if n > MAX_BRICKS:
        raise ValueError(f"sparse TSDF volume: {n} bricks: 7 * 512 * max_bricks must stay below 2^31 "
                         f"(32-bit edge keys), i.e. max_bricks <= {MAX_BRICKS}")
    return n


def samples_of(trunc: float, voxel_size: float) -> int:
    """Samples along a pixel's ray, 4 voxels apart, that cover the band [d - trunc, d + trunc]."""
    return int(math.ceil(2.0 * float(trunc) / (4.0 * float(voxel_size)))) + 1


def brick_keys(bricks) -> np.ndarray:
    """The 64-bit key of brick coordinates [B,3] (int64)."""
    b = np.asarray(bricks, np.int64).reshape(-1, 3) + COORD_RANGE
    return b[:, 0] | (b[:, 1] << 21) | (b[:, 2] << 42)


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def allocate_bricks_torch(bricks, max_bricks, origin, voxel_size, trunc, depth, T_w2c, fx, fy, cx, cy, opacity=None,
                          min_opacity=0.95, normalize=False, depth_min=0.0, depth_max=math.inf, z_near=0.2):
    """mgs_sparse_tsdf_allocate in fp32 torch: (bricks' int32 [B',3] - the list `bricks` [B,3] with the view's new
    bricks appended in the order of their first candidate, cut at max_bricks -, dropped, out_of_range).  Every
    product, sum, difference and quotient is one torch operation, i.e. one rounding."""
    f = _f32
    old = np.asarray(bricks, np.int64).reshape(-1, 3)
    T = torch.as_tensor(T_w2c).detach().to("cpu", torch.float32)
    depth = torch.as_tensor(depth).detach().to("cpu", torch.float32)
    H, W = depth.shape[-2:]
    d = depth.reshape(-1)
    ok = torch.ones(H * W, dtype=torch.bool)
    if opacity is not None:
        o = torch.as_tensor(opacity).detach().to("cpu", torch.float32).reshape(-1)
        ok = ok & ~(o < f(min_opacity))
        if normalize:
            d = d / o
    ok = ok & (d > f(depth_min)) & (d <= f(depth_max))
    S = samples_of(trunc, voxel_size)
    vs = f(voxel_size)
    step = f(4.0) * vs
    z = (d - f(trunc))[:, None] + torch.arange(S, dtype=torch.float32)[None, :] * step          # [HW,S]
    ok = ok[:, None] & (z > f(z_near))
    pix = torch.arange(H * W)
    xn = ((pix % W).float() - f(cx)) / f(fx)
    yn = ((pix // W).float() - f(cy)) / f(fy)
    q = (xn[:, None] * z - T[0, 3], yn[:, None] * z - T[1, 3], z - T[2, 3])
    lo, hi = [], []
    for a in range(3):
        p = (T[0, a] * q[0] + T[1, a] * q[1]) + T[2, a] * q[2]
        l = (p - f(origin[a])) / vs
        lo.append(torch.floor((l - f(4.0)) * f(0.125)))
        hi.append(torch.floor((l + f(4.0)) * f(0.125)))
    b = torch.stack([torch.stack([(hi[a] if (c >> a) & 1 else lo[a]) for a in range(3)], -1) for c in range(8)], -2)
    in_range = ((b >= float(-COORD_RANGE)) & (b < float(COORD_RANGE))).all(-1)                  # [HW,S,8]; NaN: outside
    out_of_range = int((ok[..., None] & ~in_range).sum())
    valid = (ok[..., None] & in_range).reshape(-1).numpy()
    coords = torch.where(in_range[..., None], b, torch.zeros(())).long().reshape(-1, 3).numpy()
    keys = brick_keys(coords)
    valid &= ~np.isin(keys, brick_keys(old))
    cand = np.flatnonzero(valid)
    _, first = np.unique(keys[cand], return_index=True)
    new = coords[cand[np.sort(first)]]
    room = max(0, int(max_bricks) - len(old))
    dropped = max(0, len(new) - room)
    return np.concatenate([old, new[:room]]).astype(np.int32), dropped, out_of_range


def integrate_bricks_torch(bricks, tsdf, weight, color, origin, voxel_size, trunc, depth, T_w2c, fx, fy, cx, cy, image=None,
                           opacity=None, min_opacity=0.95, normalize=False, view_weight=1.0, depth_min=0.0,
                           depth_max=math.inf, z_near=0.2, max_weight=64.0):
    """mgs_sparse_tsdf_integrate in fp32 torch, in place on the first B rows of tsdf / weight [cap,512] and color
    [3,cap,512] for the brick list `bricks` [B,3]: tsdf.integrate_torch's operations on the lattice points
    origin + (8 b + l) * voxel_size of every listed brick (no culling)."""
    dev = tsdf.device
    f = lambda x: _f32(x, dev)
    bricks = torch.as_tensor(np.asarray(bricks, np.int64).reshape(-1, 3), device=dev)
    B = bricks.shape[0]
    if B == 0:
        return
    T = torch.as_tensor(T_w2c).detach().to(dev, torch.float32)
    depth = torch.as_tensor(depth).detach().to(dev, torch.float32)
    H, W = depth.shape[-2:]
    depth = depth.reshape(-1)
    vs = f(voxel_size)
    loc = torch.arange(BRICK, device=dev)
    ax = [f(origin[a]) + (BRICK * bricks[:, a, None] + loc[None, :]).float() * vs for a in range(3)]       # [B,8] each
    px, py, pz = ax[0][:, None, None, :], ax[1][:, None, :, None], ax[2][:, :, None, None]
    row = lambda r: ((T[r, 0] * px + T[r, 1] * py) + T[r, 2] * pz) + T[r, 3]
    xc, yc, zc = row(0), row(1), row(2)
    ok = zc > f(z_near)
    u = f(fx) * (xc / zc) + f(cx)
    v = f(fy) * (yc / zc) + f(cy)
    uf, vf = torch.floor(u + f(0.5)), torch.floor(v + f(0.5))
    ok = ok & (uf >= 0) & (uf < float(W)) & (vf >= 0) & (vf < float(H))
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    pix = torch.where(ok, vf, zero).long() * W + torch.where(ok, uf, zero).long()
    d = depth[pix]
    if opacity is not None:
        o = torch.as_tensor(opacity).detach().to(dev, torch.float32).reshape(-1)[pix]
        ok = ok & ~(o < f(min_opacity))
        if normalize:
            d = d / o
    ok = ok & (d > f(depth_min)) & (d <= f(depth_max))
    sdf = d - zc
    tr = f(trunc)
    ok = ok & ~(sdf < -tr)
    tn = torch.minimum(torch.ones((), dtype=torch.float32, device=dev), sdf / tr)
    w = f(view_weight)
    shape = (B, BRICK, BRICK, BRICK)
    D, Wt = tsdf[:B].view(shape), weight[:B].view(shape)
    W0 = Wt.clone()
    W1 = W0 + w
    if image is not None:
        img = torch.as_tensor(image).detach().to(dev, torch.float32).reshape(3, -1)
        for c in range(3):
            Cc = color[c, :B].view(shape)
            Cc.copy_(torch.where(ok, (W0 * Cc + w * img[c][pix]) / W1, Cc))
    D.copy_(torch.where(ok, (W0 * D + w * tn) / W1, D))
    Wt.copy_(torch.where(ok, torch.minimum(W1, f(max_weight)), W0))


def bricks_to_box(bricks, tsdf, weight, color=None):
    """The dense planes of the bounding box of a brick list (NumPy): (lo - the lattice index (i,j,k) of the box's first
    point -, tsdf, weight [nz,ny,nx], color [3,nz,ny,nx] or None, grid - the brick id of every brick of the box
    [nbz,nby,nbx], -1 where absent).  A point of an absent brick has tsdf 1, weight 0, colour 0."""
    b = np.asarray(bricks, np.int64).reshape(-1, 3)
    B = b.shape[0]
    blo = b.min(0)
    nb = b.max(0) + 1 - blo
    nbx, nby, nbz = (int(v) for v in nb)
    rx, ry, rz = (b - blo).T
    grid = np.full((nbz, nby, nbx), -1, np.int64)
    grid[rz, ry, rx] = np.arange(B)
    shape6 = (nbz, BRICK, nby, BRICK, nbx, BRICK)
    shape3 = (nbz * BRICK, nby * BRICK, nbx * BRICK)

    def box(rows, init):
        out = np.full(shape3, init, np.float32)
        out.reshape(shape6).transpose(0, 2, 4, 1, 3, 5)[rz, ry, rx] = np.asarray(rows, np.float32)[:B].reshape(B, BRICK, BRICK, BRICK)
        return out

    col = None if color is None else np.stack([box(np.asarray(color, np.float32)[c], 0.0) for c in range(3)])
    return BRICK * blo, box(tsdf, 1.0), box(weight, 0.0), col, grid


def _extract_box(t, w, col, origin, voxel_size, min_weight, lo):
    """tsdf.extract_mesh_numpy on dense planes whose first point has the lattice index `lo`: the same decisions, the
    positions formed from the GLOBAL index.  Returns verts, colors (in the box's key order), lin, slot of every vertex,
    and the face rows (cell, tetrahedron, triangle, three vertex ids), unsorted."""
    nz, ny, nx = t.shape
    n = nx * ny * nz
    inside = t < 0
    with np.errstate(invalid="ignore"):
        wok = w >= np.float32(min_weight)
    cv = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    c = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        c &= wok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    cv[1:nz, 1:ny, 1:nx] = c
    cell = lambda dx, dy, dz: cv[1 - dz:nz + 1 - dz, 1 - dy:ny + 1 - dy, 1 - dx:nx + 1 - dx]   # cell with base a - d
    bits = np.zeros((7, nz, ny, nx), bool)
    for s, (ox, oy, oz) in enumerate(SLOT_OFFSETS):
        differ = np.zeros((nz, ny, nx), bool)
        differ[:nz - oz, :ny - oy, :nx - ox] = inside[:nz - oz, :ny - oy, :nx - ox] != inside[oz:, oy:, ox:]
        anyv = np.zeros((nz, ny, nx), bool)
        for dx, dy, dz in itertools.product(*[((0,) if o else (0, 1)) for o in (ox, oy, oz)]):
            anyv |= cell(dx, dy, dz)
        bits[s] = differ & anyv
    keys = np.flatnonzero(bits.reshape(7, n).T.reshape(-1))
    V = keys.size
    vid = np.full(7 * n, -1, np.int64)
    vid[keys] = np.arange(V)
    lin, slot = keys // 7, keys % 7
    idx = np.stack([lin % nx, (lin // nx) % ny, lin // (nx * ny)], 1)
    off = np.asarray(SLOT_OFFSETS, np.int64)[slot]
    vs = np.float32(voxel_size)
    org = np.asarray(origin, np.float32)
    glo = np.asarray(lo, np.int64)[None, :]
    pa = org[None, :] + (idx + glo).astype(np.float32) * vs
    pb = org[None, :] + (idx + off + glo).astype(np.float32) * vs
    lb = lin + off[:, 0] + off[:, 1] * nx + off[:, 2] * nx * ny
    tf = t.reshape(-1)
    ta, tb = tf[lin], tf[lb]
    with np.errstate(all="ignore"):
        f = ta / (ta - tb)
        verts = (pa + f[:, None] * (pb - pa)).astype(np.float32)
        if col is None:
            colors = np.zeros((V, 3), np.float32)
        else:
            cf = col.reshape(3, n)
            ca, cb = cf[:, lin].T, cf[:, lb].T
            colors = (ca + f[:, None] * (cb - ca)).astype(np.float32)
    cz, cy, cx = np.nonzero(cv[1:, 1:, 1:][:nz, :ny, :nx])
    cl = (cz * ny + cy) * nx + cx
    rows = []
    code_off = lambda code: (code & 1) + ((code >> 1) & 1) * nx + (code >> 2) * nx * ny
    for ti, corners in enumerate(TET_CORNERS):
        case = np.zeros(cl.shape, np.int64)
        for p, code in enumerate(corners):
            case |= inside.reshape(-1)[cl + code_off(code)].astype(np.int64) << p
        for cs in range(1, 15):
            sel = cl[case == cs]
            if sel.size == 0:
                continue
            for ri, tri in enumerate(TET_TABLE[cs]):
                ids = []
                for le in tri:
                    p, q = TET_EDGES[le]
                    ca_, cb_ = corners[p], corners[q]
                    ids.append(vid[(sel + code_off(ca_)) * 7 + SLOT_OF_CODE[ca_ ^ cb_]])
                if TET_FLIP[ti]:
                    ids[1], ids[2] = ids[2], ids[1]
                rows.append(np.stack([sel, np.full_like(sel, ti), np.full_like(sel, ri)] + ids, 1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 6), np.int64)
    return verts.reshape(V, 3), colors.reshape(V, 3), lin, slot, rows


def extract_mesh_bricks_numpy(bricks, tsdf, weight, color, origin, voxel_size, min_weight=1.0):
    """mgs_sparse_tsdf_mesh_count + _emit in NumPy for the brick list `bricks` [B,3] and the first B rows of the
    planes: the dense extraction of the masked dense planes of the list's bounding box (every decision is
    tsdf.extract_mesh_numpy's; the positions come from the global lattice index), then the sparse order - vertices
    ascending in (brick * 512 + local) * 7 + slot, faces by brick, cell, tetrahedron, triangle.  For tests and small
    volumes: it materialises the bounding box."""
    b = np.asarray(bricks, np.int64).reshape(-1, 3)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    if b.shape[0] == 0:
        return empty
    lo, t, w, col, grid = bricks_to_box(b, tsdf, weight, color)
    verts, colors, lin, slot, rows = _extract_box(t, w, col, origin, voxel_size, min_weight, lo)
    if verts.shape[0] == 0:
        return empty
    nz, ny, nx = t.shape

    def virtual(l):
        i, j, k = l % nx, (l // nx) % ny, l // (nx * ny)
        return grid[k // BRICK, j // BRICK, i // BRICK] * BRICK_POINTS + ((k % BRICK) * BRICK + j % BRICK) * BRICK + i % BRICK

    order = np.argsort(virtual(lin) * 7 + slot, kind="stable")
    new_id = np.empty(order.size, np.int64)
    new_id[order] = np.arange(order.size)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], virtual(rows[:, 0])))]
    return verts[order], new_id[rows[:, 3:]].astype(np.int32).reshape(-1, 3), colors[order]


# ---- the volume ------------------------------------------------------------------------------------------------------
class SparseTSDFVolume:
    """A brick-hashed TSDF lattice on the device.  The planes are plain tensors (`tsdf`, `weight`, `color`,
    `brick_coords`, the map's `map_keys` / `map_vals`, the counters `state`) the caller may read or replace by views of
    its own storage (contiguous, of the same shapes and types); the native library keeps no state.  `state` is int32
    [4]: bricks allocated, bricks not allocated for want of capacity (summed over the views), candidates outside the
    coordinate range (summed), new bricks the last view asked for."""

    def __init__(self, origin=(0.0, 0.0, 0.0), voxel_size: float = 0.02, max_bricks: int = 65536,
                 trunc: Optional[float] = None, device="cuda", max_weight: float = 64.0):
        self.max_bricks = check_max_bricks(max_bricks)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("SparseTSDFVolume runs on the GPU only (HIP kernels, gfx950); the mirrors "
                               "allocate_bricks_torch / integrate_bricks_torch / extract_mesh_bricks_numpy run anywhere")
        if not voxel_size > 0:
            raise ValueError("SparseTSDFVolume: voxel_size must be positive")
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        cap = self.max_bricks
        self.table_size = int(_cabi.lib().mgs_sparse_tsdf_table_size(cap))
        self.tsdf = torch.ones((cap, BRICK_POINTS), device=self.dev)
        self.weight = torch.zeros((cap, BRICK_POINTS), device=self.dev)
        self.color = torch.zeros((3, cap, BRICK_POINTS), device=self.dev)
        self.has_color = False          # whether a view was integrated with an image (host-side: no read of the planes)
        self.brick_coords = torch.zeros((cap, 3), dtype=torch.int32, device=self.dev)
        self.map_keys = torch.full((self.table_size,), -1, dtype=torch.int64, device=self.dev)
        self.map_vals = torch.zeros(self.table_size, dtype=torch.int32, device=self.dev)
        self.state = torch.zeros(4, dtype=torch.int32, device=self.dev)
        self._alloc_scratch, self._alloc_key = None, None
        self._mesh_scratch, self._mesh_bricks = None, 0
        self._counts = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.brick_epoch = 0      # calls that can change the brick list: tsdf_raycast.neighbor_table rebuilds on a change

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.color.zero_()
        self.has_color = False
        self.map_keys.fill_(-1)
        self.state.zero_()
        self.brick_epoch += 1

    def stats(self) -> dict:
        """One host read: the counters, and the bytes the volume holds."""
        n, dropped, out_of_range, last = (int(v) for v in self.state.cpu())
        held = sum(t.numel() * t.element_size() for t in (self.tsdf, self.weight, self.color, self.brick_coords,
                                                          self.map_keys, self.map_vals))
        return {"bricks": n, "dropped": dropped, "out_of_range": out_of_range, "last_view_new": last,
                "max_bricks": self.max_bricks, "bytes": held, "bytes_in_use": n * BRICK_POINTS * 20}

    @property
    def num_bricks(self) -> int:
        return int(self.state[0])

    @property
    def dropped(self) -> int:
        return int(self.state[1])

    def bricks(self) -> torch.Tensor:
        """int32 [B,3]: the coordinates of the allocated bricks, by id (one host read, of B)."""
        return self.brick_coords[:self.num_bricks]

    def _tensor(self, t, shape, dtype, what):
        if t.device != self.dev or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"SparseTSDFVolume.{what} must be a contiguous {dtype} tensor {shape} on {self.dev}")
        return t.data_ptr()

    def _volume(self, v):
        cap = self.max_bricks
        v.max_bricks = cap
        v.origin[0], v.origin[1], v.origin[2] = self.origin
        v.voxel_size = self.voxel_size
        v.tsdf = self._tensor(self.tsdf, (cap, BRICK_POINTS), torch.float32, "tsdf")
        v.weight = self._tensor(self.weight, (cap, BRICK_POINTS), torch.float32, "weight")
        v.color = self._tensor(self.color, (3, cap, BRICK_POINTS), torch.float32, "color")
        v.brick_coords = self._tensor(self.brick_coords, (cap, 3), torch.int32, "brick_coords")
        v.map_keys = self._tensor(self.map_keys, (self.table_size,), torch.int64, "map_keys")
        v.map_vals = self._tensor(self.map_vals, (self.table_size,), torch.int32, "map_vals")
        v.state = self._tensor(self.state, (4,), torch.int32, "state")

    def integrate(self, depth, T_w2c, fx, fy, cx, cy, image=None, opacity=None, min_opacity=0.95, normalize=False,
                  weight=1.0, depth_min=0.0, depth_max=math.inf, z_near=0.2, allocate=True):
        """One view into the volume, TSDFVolume.integrate's arguments: the bricks the view needs are allocated (five
        launches behind one fill of the view's candidate set), then every allocated brick is updated (one launch over the
        pool, workgroups past the brick count leave at once) - all on the current stream, no host read.
        `allocate=False` integrates into the existing bricks only."""
        f32 = lambda t: torch.as_tensor(t).detach().to(self.dev, torch.float32).contiguous()
        depth = f32(depth)
        H, W = (int(v) for v in depth.shape[-2:])
        if depth.numel() != H * W:
            raise ValueError(f"depth must be [H,W] or [1,H,W], got {tuple(depth.shape)}")
        T = f32(T_w2c)
        if tuple(T.shape) != (4, 4):
            raise ValueError("T_w2c must be [4,4]")
        a = _cabi.SparseTsdfViewArgs()
        self._volume(a.vol)
        a.width, a.height, a.normalize = W, H, 1 if normalize else 0
        a.samples = samples_of(self.trunc, self.voxel_size)
        a.trunc = self.trunc
        a.fx, a.fy, a.cx, a.cy = float(fx), float(fy), float(cx), float(cy)
        a.z_near, a.depth_min, a.depth_max = float(z_near), float(depth_min), float(depth_max)
        a.min_opacity, a.view_weight, a.max_weight = float(min_opacity), float(weight), self.max_weight
        a.T, a.depth = T.data_ptr(), depth.data_ptr()
        keep = [T, depth]
        if opacity is not None:
            opacity = f32(opacity)
            if opacity.numel() != H * W:
                raise ValueError("opacity must have the depth's size")
            a.opacity = opacity.data_ptr()
            keep.append(opacity)
        if image is not None:
            image = f32(image)
            if tuple(image.shape) != (3, H, W):
                raise ValueError(f"image must be [3,{H},{W}], got {tuple(image.shape)}")
            a.image = image.data_ptr()
            keep.append(image)
            self.has_color = True
        L = _cabi.lib()
        if allocate:
            key = (W, H, a.samples)
            if self._alloc_key != key:
                nbytes = int(L.mgs_sparse_tsdf_allocate_scratch_bytes(W, H, a.samples))
                if nbytes == 0:
                    raise ValueError(f"SparseTSDFVolume.integrate: {W} x {H} pixels x {a.samples} samples x 8 corners "
                                     "must stay below 2^31")
                self._alloc_scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
                self._alloc_key = key
            a.scratch = self._alloc_scratch.data_ptr()
            _cabi.check(L.mgs_sparse_tsdf_allocate(C.byref(a), stream_ptr(self.dev)), "mgs_sparse_tsdf_allocate")
            self.brick_epoch += 1
        # `keep` holds the converted inputs until the launches are enqueued; the allocator orders their reuse on this stream
        _cabi.check(L.mgs_sparse_tsdf_integrate(C.byref(a), stream_ptr(self.dev)), "mgs_sparse_tsdf_integrate")
        del keep

    # the render of a view and its hand-over to integrate(): TSDFVolume's, which reads self.dev and calls self.integrate
    _surface_viewer = TSDFVolume._surface_viewer
    integrate_view = TSDFVolume.integrate_view

    def extract_mesh(self, min_weight: float = 1.0, clean=None, simplify=None, smooth=None, allow_dropped: bool = False):
        """(verts [V,3] f32, faces [F,3] i32, colors [V,3] f32) on the device; empty tensors when nothing crosses.
        TWO host reads - one more than TSDFVolume.extract_mesh: the counters (brick count, dropped) before the first
        launch, then (V, F) between the scan and the emission.  Raises when bricks were dropped for want of capacity
        (the surface then has holes the caller did not ask for) unless `allow_dropped`.  `clean`, `smooth` and
        `simplify` are TSDFVolume.extract_mesh's, applied in that order (one more host read each);
        simplify=dict(factor=) counts its cells from the volume's origin."""
        L = _cabi.lib()
        n, dropped = (int(v) for v in self.state[:2].cpu())
        if dropped and not allow_dropped:
            raise RuntimeError(f"SparseTSDFVolume.extract_mesh: {dropped} bricks were not allocated (max_bricks = "
                               f"{self.max_bricks}); pass allow_dropped=True to extract what there is")
        V = F = 0
        if n > 0:
            a = _cabi.SparseTsdfMeshArgs()
            self._volume(a.vol)
            a.num_bricks, a.min_weight = n, float(min_weight)
            if self._mesh_bricks < n:
                self._mesh_scratch = torch.empty(int(L.mgs_sparse_tsdf_mesh_scratch_bytes(n)), dtype=torch.uint8,
                                                 device=self.dev)
                self._mesh_bricks = n
            a.scratch, a.counts = self._mesh_scratch.data_ptr(), self._counts.data_ptr()
            _cabi.check(L.mgs_sparse_tsdf_mesh_count(C.byref(a), stream_ptr(self.dev)), "mgs_sparse_tsdf_mesh_count")
            V, F = (int(v) for v in self._counts.cpu())
            if V == 2 ** 31 - 1 or F > (2 ** 31 - 1) // 3:
                raise ValueError("SparseTSDFVolume.extract_mesh: the mesh exceeds 32-bit indices")
        verts = torch.empty(V, 3, device=self.dev)
        colors = torch.empty(V, 3, device=self.dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=self.dev)
        if V or F:
            a.num_verts, a.num_faces = V, F
            if V:
                a.verts, a.colors = verts.data_ptr(), colors.data_ptr()
            if F:
                a.faces = faces.data_ptr()
            _cabi.check(L.mgs_sparse_tsdf_mesh_emit(C.byref(a), stream_ptr(self.dev)), "mgs_sparse_tsdf_mesh_emit")
        if clean is not None:
            from .mesh_clean import clean_mesh
            verts, faces, colors, _ = clean_mesh(verts, faces, colors, **clean)
        if smooth is not None:
            from .mesh_smooth import smooth_mesh
            verts, _ = smooth_mesh(verts, faces, **smooth)
        if simplify is not None:
            from .mesh_simplify import simplify_keywords, simplify_mesh
            verts, faces, colors, _ = simplify_mesh(verts, faces, colors,
                                                    **simplify_keywords(simplify, self.voxel_size, self.origin))
        return verts, faces, colors

    def raycast(self, T_w2c, fx, fy, cx, cy, H, W, **kw):
        """tsdf_raycast.raycast of this volume: dict(depth, normal, color, hit_step) on the device, no host read."""
        from .tsdf_raycast import raycast
        return raycast(self, T_w2c, fx, fy, cx, cy, H, W, **kw)

    def raycast_view(self, camera, **kw):
        """tsdf_raycast.raycast_view of this volume at a camera object or a view tuple."""
        from .tsdf_raycast import raycast_view
        return raycast_view(self, camera, **kw)

    def track(self, depth, T_prev, view, image=None, photo_weight=0.0, **kw):
        """icp.track_against_volume: ray cast this volume at T_prev and align the sensor plane `depth` to it - with `image`
        [3,H,W] and photo_weight > 0 also its colour (a volume fused without colour then raises ValueError)."""
        from .icp import track_against_volume
        return track_against_volume(self, depth, T_prev, view, image=image, photo_weight=photo_weight, **kw)

    # ---- to and from dense planes (torch indexing; for tests and users, not on a hot path) ---------------------------
    def to_dense(self, lo=None, dims=None):
        """(origin, tsdf, weight [nz,ny,nx], color [3,nz,ny,nx]) of the box of `dims` = (nx, ny, nz) points whose first
        point has the lattice index `lo` = (i, j, k); by default the bounding box of the allocated bricks.  `origin` is
        the position of that first point (origin + lo * voxel_size, formed in fp32 as the kernels form it); a point of
        an unallocated brick has tsdf 1, weight 0, colour 0."""
        n = self.num_bricks
        coords = self.brick_coords[:n].long()
        if lo is None or dims is None:
            if n == 0:
                raise ValueError("SparseTSDFVolume.to_dense: no brick is allocated; give lo and dims")
            cmin, cmax = coords.min(0).values.cpu(), coords.max(0).values.cpu()
            if lo is None:
                lo = [BRICK * int(v) for v in cmin]
            if dims is None:
                dims = [BRICK * (int(v) + 1) - int(l) for v, l in zip(cmax, lo)]
        lo = [int(v) for v in lo]
        nx, ny, nz = (int(v) for v in dims)
        if min(nx, ny, nz) < 1:
            raise ValueError("SparseTSDFVolume.to_dense: dims must be positive")
        blo = [l // BRICK for l in lo]
        nb = [(l + d - 1) // BRICK + 1 - b for l, d, b in zip(lo, (nx, ny, nz), blo)]
        rel = coords - torch.tensor(blo, device=self.dev)
        sel = ((rel >= 0) & (rel < torch.tensor(nb, device=self.dev))).all(1)
        rx, ry, rz = rel[sel].T
        shape6 = (nb[2], BRICK, nb[1], BRICK, nb[0], BRICK)
        shape3 = (nb[2] * BRICK, nb[1] * BRICK, nb[0] * BRICK)
        off = [l - BRICK * b for l, b in zip(lo, blo)]

        def box(rows, init):
            out = torch.full(shape3, init, device=self.dev)
            out.view(shape6).permute(0, 2, 4, 1, 3, 5)[rz, ry, rx] = rows[:n][sel].view(-1, BRICK, BRICK, BRICK)
            return out[off[2]:off[2] + nz, off[1]:off[1] + ny, off[0]:off[0] + nx].contiguous()

        o32 = np.asarray(self.origin, np.float32) + np.asarray(lo, np.float32) * np.float32(self.voxel_size)
        color = torch.stack([box(self.color[c], 0.0) for c in range(3)])
        return tuple(float(v) for v in o32), box(self.tsdf, 1.0), box(self.weight, 0.0), color

    @classmethod
    def from_dense(cls, origin, voxel_size, tsdf, weight, color=None, lo=(0, 0, 0), bricks=None, max_bricks=None,
                   trunc=None, device="cuda", max_weight: float = 64.0):
        """A sparse volume that holds the dense planes tsdf / weight [nz,ny,nx] (color [3,nz,ny,nx]) whose first point
        has the lattice index `lo` of the lattice at `origin`.  `bricks` - int [B,3], distinct - lists the bricks to
        allocate, in id order; by default every brick the box touches, x fastest.  Points of a listed brick outside the
        box get tsdf 1, weight 0; points of the box in no listed brick are left out."""
        dev = torch.device(device)
        t = torch.as_tensor(tsdf, dtype=torch.float32)
        nz, ny, nx = (int(v) for v in t.shape)
        lo = [int(v) for v in lo]
        blo = [l // BRICK for l in lo]
        nb = [(l + d - 1) // BRICK + 1 - b for l, d, b in zip(lo, (nx, ny, nz), blo)]
        if bricks is None:
            bz, by, bx = np.meshgrid(*(np.arange(nb[a]) + blo[a] for a in (2, 1, 0)), indexing="ij")
            bricks = np.stack([bx, by, bz], -1).reshape(-1, 3)
        bricks = np.asarray(bricks, np.int64).reshape(-1, 3)
        B = bricks.shape[0]
        if len(np.unique(brick_keys(bricks))) != B or np.abs(bricks + 0.5).max(initial=0) > COORD_RANGE:
            raise ValueError("SparseTSDFVolume.from_dense: bricks must be distinct and lie in [-2^20, 2^20)")
        rel = bricks - np.asarray(blo)
        if B and (rel.min() < 0 or (rel >= np.asarray(nb)).any()):
            raise ValueError("SparseTSDFVolume.from_dense: a listed brick lies outside the box")
        vol = cls(origin, voxel_size, max(B, 1) if max_bricks is None else max_bricks, trunc=trunc, device=dev,
                  max_weight=max_weight)
        if B > vol.max_bricks:
            raise ValueError(f"SparseTSDFVolume.from_dense: {B} bricks exceed max_bricks = {vol.max_bricks}")
        if B == 0:
            return vol
        rx, ry, rz = (torch.as_tensor(rel[:, a], device=dev) for a in range(3))
        shape6 = (nb[2], BRICK, nb[1], BRICK, nb[0], BRICK)
        shape3 = (nb[2] * BRICK, nb[1] * BRICK, nb[0] * BRICK)
        off = [l - BRICK * b for l, b in zip(lo, blo)]

        def rows(plane, init):
            box = torch.full(shape3, init, device=dev)
            box[off[2]:off[2] + nz, off[1]:off[1] + ny, off[0]:off[0] + nx] = torch.as_tensor(plane, dtype=torch.float32).to(dev)
            return box.view(shape6).permute(0, 2, 4, 1, 3, 5)[rz, ry, rx].reshape(B, BRICK_POINTS)

        vol.tsdf[:B] = rows(t, 1.0)
        vol.weight[:B] = rows(weight, 0.0)
        if color is not None:
            for c in range(3):
                vol.color[c, :B] = rows(torch.as_tensor(color, dtype=torch.float32)[c], 0.0)
            vol.has_color = True
        vol.brick_coords[:B] = torch.as_tensor(bricks, dtype=torch.int32).to(dev)
        v = _cabi.SparseTsdfVolume()
        vol._volume(v)
        _cabi.check(_cabi.lib().mgs_sparse_tsdf_register(C.byref(v), 0, B, stream_ptr(dev)), "mgs_sparse_tsdf_register")
        vol.brick_epoch += 1
        return vol
