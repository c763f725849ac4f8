"""Mesh export: projective TSDF fusion of depth planes and marching tetrahedra over the Kuhn decomposition, on the
device (csrc/tsdf.hip; the contract is in include/monogs_raster.h and DESIGN.md "Mesh export").

    vol = TSDFVolume.for_map(gaussians, voxel_size=0.02, margin=0.1)
    for cam in keyframes:
        vol.integrate_view(gaussians, cam, background)       # renders depth / opacity / colour through the forward
    verts, faces, colors = vol.extract_mesh()                # device tensors; ONE host read, of (V, F)
    ply_io.write_mesh_ply("mesh.ply", verts, faces, colors)

`integrate` takes any depth plane: sensor depth, stereo depth or a rendered one.  The lattice point (i,j,k) lies at
origin + (i,j,k) * voxel_size; the planes are tsdf [nz,ny,nx] (initial 1), weight [nz,ny,nx] (initial 0) and
color [3,nz,ny,nx] (initial 0).

The mirrors `integrate_torch` and `extract_mesh_numpy` ARE the contract: the same single fp32 roundings in the same
order, so the device's planes, vertices and colours equal theirs bit for bit and the faces equal theirs as a set.  They
need no GPU.  There is no CPU fall-back behind TSDFVolume: off the GPU it raises."""
from __future__ import annotations

import ctypes as C
import itertools
import math
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import _cabi
from ._device import stream_ptr

# the 7 edges a lattice point owns, as offsets (dx, dy, dz) in slot order, and the same as corner codes (bit 0 x ...)
SLOT_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
SLOT_CODES = tuple(dx | (dy << 1) | (dz << 2) for dx, dy, dz in SLOT_OFFSETS)
SLOT_OF_CODE = {c: s for s, c in enumerate(SLOT_CODES)}
# the six Kuhn tetrahedra: one per permutation (a, b, c) of the axes, corner codes v0, v1 = e_a, v2 = e_a + e_b, v3
TET_PERMS = tuple(itertools.permutations(range(3)))
TET_CORNERS = tuple((0, 1 << a, (1 << a) | (1 << b), 7) for a, b, c in TET_PERMS)
# det[v1 - v0, v2 - v0, v3 - v0] = det[e_a, e_b, e_c]: the odd permutations are mirror images
TET_FLIP = tuple(int(round(float(np.linalg.det(np.eye(3)[list(p)])))) < 0 for p in TET_PERMS)
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _tet_table():
    """The 16 sign cases of a positively oriented tetrahedron (bit p = corner v_p inside): a list of triangles, each
    three local edge numbers (TET_EDGES), wound so that the normal points to the outside corners.  Derived from the
    geometry of the reference tetrahedron (0,0,0) (1,0,0) (1,1,0) (1,1,1) with every crossing at the edge's middle: one
    or three inside corners cut off a corner (one triangle), two give a quad (p,r) (p,s) (q,s) (q,r) split along its
    first diagonal; a triple whose normal points to the inside corners is reversed."""
    V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], np.float64)
    eid = {e: n for n, e in enumerate(TET_EDGES)}
    key = lambda p, q: (min(p, q), max(p, q))
    table = []
    for case in range(16):
        ins = [p for p in range(4) if (case >> p) & 1]
        out = [p for p in range(4) if not (case >> p) & 1]
        tris = []
        if len(ins) in (1, 3):
            p = ins[0] if len(ins) == 1 else out[0]
            tris = [[key(p, q) for q in range(4) if q != p]]
        elif len(ins) == 2:
            (p, q), (r, s) = ins, out
            quad = [key(p, r), key(p, s), key(q, s), key(q, r)]
            tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        fixed = []
        for t in tris:
            P = [0.5 * (V[a] + V[b]) for a, b in t]
            nrm = np.cross(P[1] - P[0], P[2] - P[0])
            if float(nrm @ (V[out].mean(0) - V[ins].mean(0))) < 0:
                t = [t[0], t[2], t[1]]
            fixed.append([eid[e] for e in t])
        table.append(fixed)
    return table


TET_TABLE = _tet_table()


def _f32(x, device=None):
    return torch.tensor(float(x), dtype=torch.float32, device=device)


def check_dims(dims) -> Tuple[int, int, int]:
    nx, ny, nz = (int(v) for v in dims)
    if min(nx, ny, nz) < 1:
        raise ValueError(f"TSDF volume: dims {tuple(dims)} must be positive")
    if nx * ny * nz > _cabi.TSDF_MAX_POINTS:
        raise ValueError(f"TSDF volume: {nx} x {ny} x {nz} points: 7 nx ny nz must stay below 2^31 (32-bit edge keys)")
    return nx, ny, nz


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def integrate_torch(tsdf, weight, color, origin, voxel_size, trunc, depth, T_w2c, fx, fy, cx, cy, image=None,
                    opacity=None, min_opacity=0.95, normalize=False, view_weight=1.0, depth_min=0.0,
                    depth_max=math.inf, z_near=0.2, max_weight=64.0):
    """mgs_tsdf_integrate in fp32 torch, in place on tsdf / weight [nz,ny,nx] and color [3,nz,ny,nx] (any device, no
    culling): every product, sum, difference and quotient is one torch operation, i.e. one rounding."""
    dev = tsdf.device
    nz, ny, nx = tsdf.shape
    f = lambda x: _f32(x, dev)
    T = torch.as_tensor(T_w2c).detach().to(dev, torch.float32)
    depth = torch.as_tensor(depth).detach().to(dev, torch.float32)
    H, W = depth.shape[-2:]
    depth = depth.reshape(-1)
    vs = f(voxel_size)
    ax = [f(origin[a]) + torch.arange(n, dtype=torch.float32, device=dev) * vs for a, n in enumerate((nx, ny, nz))]
    px, py, pz = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
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
    W0 = weight.clone()
    W1 = W0 + w
    if image is not None:
        img = torch.as_tensor(image).detach().to(dev, torch.float32).reshape(3, -1)
        for c in range(3):
            color[c].copy_(torch.where(ok, (W0 * color[c] + w * img[c][pix]) / W1, color[c]))
    tsdf.copy_(torch.where(ok, (W0 * tsdf + w * tn) / W1, tsdf))
    weight.copy_(torch.where(ok, torch.minimum(W1, f(max_weight)), W0))


def extract_mesh_numpy(tsdf, weight, color, origin, voxel_size, min_weight=1.0):
    """mgs_tsdf_mesh_count + mgs_tsdf_mesh_emit in vectorised NumPy: (verts [V,3] f32 in ascending key order,
    faces [F,3] i32 ordered by cell, tetrahedron, triangle, colors [V,3] f32).  color may be None (zeros)."""
    t = np.ascontiguousarray(np.asarray(tsdf, np.float32))
    w = np.asarray(weight, np.float32)
    nz, ny, nx = t.shape
    n = nx * ny * nz
    col = None if color is None else np.asarray(color, np.float32).reshape(3, n)
    inside = t < 0
    with np.errstate(invalid="ignore"):
        wok = w >= np.float32(min_weight)
    # cell validity on the full lattice (False where the cell leaves it), padded by one at the low side
    cv = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    if min(nx, ny, nz) >= 2:
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
    keys = np.flatnonzero(bits.reshape(7, n).T.reshape(-1))        # ascending 7 * linear + slot
    V = keys.size
    vid = np.full(7 * n, -1, np.int64)
    vid[keys] = np.arange(V)
    lin, slot = keys // 7, keys % 7
    idx = np.stack([lin % nx, (lin // nx) % ny, lin // (nx * ny)], 1)
    off = np.asarray(SLOT_OFFSETS, np.int64)[slot]
    vs = np.float32(voxel_size)
    org = np.asarray(origin, np.float32)
    pa = org[None, :] + idx.astype(np.float32) * vs
    pb = org[None, :] + (idx + off).astype(np.float32) * vs
    lb = lin + off[:, 0] + off[:, 1] * nx + off[:, 2] * nx * ny
    tf = t.reshape(-1)
    ta, tb = tf[lin], tf[lb]
    with np.errstate(all="ignore"):
        f = ta / (ta - tb)
        verts = (pa + f[:, None] * (pb - pa)).astype(np.float32)
        if col is None:
            colors = np.zeros((V, 3), np.float32)
        else:
            ca, cb = col[:, lin].T, col[:, lb].T
            colors = (ca + f[:, None] * (cb - ca)).astype(np.float32)
    # faces
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
    if rows:
        r = np.concatenate(rows)
        r = r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]
        faces = r[:, 3:].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    return verts.reshape(V, 3), faces, colors.reshape(V, 3)


# ---- the volume ------------------------------------------------------------------------------------------------------
class TSDFVolume:
    """A dense TSDF lattice on the device.  The planes are plain tensors (`tsdf`, `weight`, `color`) the caller may
    read or replace by views of its own storage (contiguous fp32 of the same shapes); the native library keeps no
    state."""

    def __init__(self, origin, voxel_size: float, dims, trunc: Optional[float] = None, device="cuda",
                 max_weight: float = 64.0):
        self.nx, self.ny, self.nz = check_dims(dims)
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("TSDFVolume runs on the GPU only (HIP kernels, gfx950); the mirrors integrate_torch / "
                               "extract_mesh_numpy run anywhere")
        if not voxel_size > 0:
            raise ValueError("TSDFVolume: voxel_size must be positive")
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size = float(voxel_size)
        self.trunc = 4.0 * self.voxel_size if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        shape = (self.nz, self.ny, self.nx)
        self.tsdf = torch.ones(shape, device=self.dev)
        self.weight = torch.zeros(shape, device=self.dev)
        self.color = torch.zeros((3,) + shape, device=self.dev)
        self.has_color = False          # whether a view was integrated with an image (host-side: no read of the planes)
        self._scratch = None
        self._counts = torch.zeros(2, dtype=torch.int32, device=self.dev)

    @classmethod
    def for_map(cls, gaussians, voxel_size: float, margin: float = 0.1, **kw):
        """A volume around the bounds of the Gaussians' means, grown by `margin` on every side."""
        xyz = gaussians.get_xyz.detach()
        lo, hi = xyz.min(dim=0).values.cpu(), xyz.max(dim=0).values.cpu()
        origin = [float(v) - margin for v in lo]
        dims = [int(math.ceil((float(h) - float(l) + 2 * margin) / voxel_size)) + 1 for l, h in zip(lo, hi)]
        kw.setdefault("device", xyz.device)
        return cls(origin, voxel_size, dims, **kw)

    @property
    def dims(self):
        return self.nx, self.ny, self.nz

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.color.zero_()
        self.has_color = False

    def _plane(self, t, shape, what):
        if t.device != self.dev or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"TSDFVolume.{what} must be a contiguous fp32 tensor {shape} on {self.dev}")
        return t.data_ptr()

    def integrate(self, depth, T_w2c, fx, fy, cx, cy, image=None, opacity=None, min_opacity=0.95, normalize=False,
                  weight=1.0, depth_min=0.0, depth_max=math.inf, z_near=0.2):
        """One view into the volume: one launch on the current stream, no host read.  depth [H,W] (or [1,H,W]) in the
        units of the map, T_w2c [4,4] world -> camera, image [3,H,W], opacity [H,W]."""
        f32 = lambda t: torch.as_tensor(t).detach().to(self.dev, torch.float32).contiguous()
        depth = f32(depth)
        H, W = (int(v) for v in depth.shape[-2:])
        if depth.numel() != H * W:
            raise ValueError(f"depth must be [H,W] or [1,H,W], got {tuple(depth.shape)}")
        T = f32(T_w2c)
        if tuple(T.shape) != (4, 4):
            raise ValueError("T_w2c must be [4,4]")
        a = _cabi.TsdfIntegrateArgs()
        a.nx, a.ny, a.nz, a.width, a.height, a.normalize = self.nx, self.ny, self.nz, W, H, 1 if normalize else 0
        a.origin[0], a.origin[1], a.origin[2] = self.origin
        a.voxel_size, a.trunc = self.voxel_size, self.trunc
        a.fx, a.fy, a.cx, a.cy = float(fx), float(fy), float(cx), float(cy)
        a.z_near, a.depth_min, a.depth_max = float(z_near), float(depth_min), float(depth_max)
        a.min_opacity, a.weight, a.max_weight = float(min_opacity), float(weight), self.max_weight
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
        shape = (self.nz, self.ny, self.nx)
        a.tsdf, a.wsum = self._plane(self.tsdf, shape, "tsdf"), self._plane(self.weight, shape, "weight")
        a.color = self._plane(self.color, (3,) + shape, "color")
        # `keep` holds the converted inputs until the launch is enqueued; the allocator orders their reuse on this stream
        _cabi.check(_cabi.lib().mgs_tsdf_integrate(C.byref(a), stream_ptr(self.dev)), "mgs_tsdf_integrate")
        del keep

    def _surface_viewer(self, gaussians, background, H, W):
        """The NativeViewer of the median mode, kept on the volume per (H, W, map)."""
        from .viewer import NativeViewer
        key = (int(H), int(W), id(gaussians))
        if getattr(self, "_viewer_key", None) != key:
            self._viewer = NativeViewer(gaussians, background, H, W, self.dev)
            self._viewer_key = key
        self._viewer.bg = background.detach().to(self.dev, torch.float32).reshape(-1).contiguous()
        return self._viewer

    def integrate_view(self, gaussians, camera, background, image=None, min_opacity=0.95, weight=1.0,
                       depth_min=0.0, depth_max=math.inf, z_near=0.2, depth_mode="mean"):
        """Renders the map at `camera` (ViewCamera: T, fx, fy, cx, cy) through the forward and integrates it where
        opacity >= min_opacity.  depth_mode "mean" fuses depth / opacity, the expected depth of the blend, and returns
        the render package.  "median" fuses the median depth (viewer.NativeViewer.surface: the depth of the splat at
        which the transmittance falls through one half), which does not bleed at silhouettes, and returns the
        surface planes; the pair capacity is confirmed BEFORE the view is integrated (one host read per view, as
        render() has; a view that exceeded it is rendered again, never integrated twice).  The colour is the rendered
        one unless `image` is given."""
        if depth_mode not in ("mean", "median"):
            raise ValueError(f"depth_mode must be 'mean' or 'median', got {depth_mode!r}")
        if depth_mode == "median":
            vw = self._surface_viewer(gaussians, background, camera.image_height, camera.image_width)
            with torch.no_grad():
                planes = vw.surface(camera, normals=False)
                if not vw.check_capacity():         # grown to 1.5 x the pairs this view holds: the second render is whole
                    planes = vw.surface(camera, normals=False)
                    if not vw.check_capacity():
                        raise RuntimeError("TSDFVolume.integrate_view: the view exceeded the grown pair capacity")
            self.integrate(planes["median_depth"], camera.T, camera.fx, camera.fy, camera.cx, camera.cy,
                           image=planes["color"] if image is None else image, opacity=planes["opacity"],
                           min_opacity=min_opacity, normalize=False, weight=weight, depth_min=depth_min,
                           depth_max=depth_max, z_near=z_near)
            return planes
        from .gaussian_renderer import render
        from .slam_loops import Pipe
        with torch.no_grad():
            pkg = render(camera, gaussians, Pipe, background)
        if pkg is None:
            raise RuntimeError("TSDFVolume.integrate_view: the map is empty")
        self.integrate(pkg["depth"], camera.T, camera.fx, camera.fy, camera.cx, camera.cy,
                       image=pkg["render"].detach() if image is None else image, opacity=pkg["opacity"],
                       min_opacity=min_opacity, normalize=True, weight=weight, depth_min=depth_min, depth_max=depth_max,
                       z_near=z_near)
        return pkg

    def _mesh_args(self, min_weight):
        a = _cabi.TsdfMeshArgs()
        a.nx, a.ny, a.nz = self.nx, self.ny, self.nz
        a.origin[0], a.origin[1], a.origin[2] = self.origin
        a.voxel_size, a.min_weight = self.voxel_size, float(min_weight)
        shape = (self.nz, self.ny, self.nx)
        a.tsdf, a.weight = self._plane(self.tsdf, shape, "tsdf"), self._plane(self.weight, shape, "weight")
        a.color = self._plane(self.color, (3,) + shape, "color")
        if self._scratch is None:
            nbytes = int(_cabi.lib().mgs_tsdf_mesh_scratch_bytes(self.nx, self.ny, self.nz))
            if nbytes == 0:
                raise ValueError("TSDFVolume: unsupported size")
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        a.scratch, a.counts = self._scratch.data_ptr(), self._counts.data_ptr()
        return a

    def extract_mesh(self, min_weight: float = 1.0, clean=None, simplify=None, smooth=None):
        """(verts [V,3] f32, faces [F,3] i32, colors [V,3] f32) on the device; empty tensors when nothing crosses.
        One host read, of (V, F), between the scan and the emission.  `clean` - a dict of mesh_clean.clean_mesh keyword
        arguments, e.g. dict(keep_largest=1) or dict(min_faces=50) - drops the floaters from the extracted mesh (one
        more host read); None leaves it as extracted.  `simplify` - a dict of mesh_simplify.simplify_mesh keyword
        arguments, applied after `clean` (one more host read) - merges the vertices of every cell of edge `cell`, or of
        `factor` voxels (dict(factor=2); not both), counted from `origin`, which defaults to the volume's; None leaves
        the mesh as it is.  `smooth` - a dict of mesh_smooth.smooth_mesh keyword arguments, e.g. dict(iterations=10) -
        moves the vertices after `clean` and before `simplify` (one more host read): denoise, then decimate; None leaves
        them where they were extracted."""
        L = _cabi.lib()
        a = self._mesh_args(min_weight)
        _cabi.check(L.mgs_tsdf_mesh_count(C.byref(a), stream_ptr(self.dev)), "mgs_tsdf_mesh_count")
        V, F = (int(v) for v in self._counts.cpu())
        if V == 2 ** 31 - 1 or F > (2 ** 31 - 1) // 3:
            raise ValueError("TSDFVolume.extract_mesh: the mesh exceeds 32-bit indices")
        verts = torch.empty(V, 3, device=self.dev)
        colors = torch.empty(V, 3, device=self.dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=self.dev)
        a.num_verts, a.num_faces = V, F
        if V:
            a.verts, a.colors = verts.data_ptr(), colors.data_ptr()
        if F:
            a.faces = faces.data_ptr()
        _cabi.check(L.mgs_tsdf_mesh_emit(C.byref(a), stream_ptr(self.dev)), "mgs_tsdf_mesh_emit")
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


    # the methods of SparseTSDFVolume, one signature for both volumes
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


def sparse_volume(sparse, voxel_size: float, device, trunc=None, max_weight: float = 64.0):
    """The sparse_tsdf.SparseTSDFVolume that `sparse` - True, or dict(max_bricks=, origin=) - asks for."""
    from .sparse_tsdf import SparseTSDFVolume
    kw = {} if sparse is True else dict(sparse)
    unknown = set(kw) - {"max_bricks", "origin"}
    if unknown:
        raise ValueError(f"sparse: unknown keys {sorted(unknown)} (max_bricks, origin)")
    return SparseTSDFVolume(kw.get("origin", (0.0, 0.0, 0.0)), voxel_size, kw.get("max_bricks", 65536), trunc=trunc,
                            device=device, max_weight=max_weight)


def fuse_map(gaussians, cameras: Iterable, background, voxel_size: float, margin: float = 0.1, trunc=None,
             max_weight: float = 64.0, min_opacity: float = 0.95, depth_max: float = math.inf,
             volume=None, depth_mode: str = "mean", sparse=None):
    """Fuses the map's own rendered depth at `cameras` into a volume sized from the map (or into `volume`, a TSDFVolume
    or a sparse_tsdf.SparseTSDFVolume): depth / opacity with depth_mode "mean", the median depth with "median"
    (TSDFVolume.integrate_view).  `sparse` - True, or dict(max_bricks=, origin=) - fuses into a new SparseTSDFVolume
    instead: no bounds pass over the map, `margin` is not used, and the bricks come with the views."""
    vol = volume
    if vol is None and sparse is not None and sparse is not False:
        vol = sparse_volume(sparse, voxel_size, gaussians.get_xyz.device, trunc=trunc, max_weight=max_weight)
    if vol is None:
        vol = TSDFVolume.for_map(gaussians, voxel_size, margin, trunc=trunc, max_weight=max_weight)
    for cam in cameras:
        vol.integrate_view(gaussians, cam, background, min_opacity=min_opacity, depth_max=depth_max,
                           depth_mode=depth_mode)
    return vol
