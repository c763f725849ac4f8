"""Mesh rendering and culling: the depth image of a triangle mesh at a pose, the visibility of vertices against such an
image, and the cull of what too few views saw - what Replica / ScanNet evaluation protocols apply to both meshes before
scoring - on the device (csrc/mesh_render.hip; the contract is in include/monogs_raster.h and DESIGN.md "Mesh rendering
and culling").

    depth, face_id, record = render_mesh_depth(verts, faces, T_w2c, fx, fy, cx, cy, H, W)       # no host read
    seen = vertex_visibility(verts, T_w2c, fx, fy, cx, cy, H, W, depth=depth, out=seen)         # no host read
    verts, faces, colors, info = cull_mesh(verts, faces, colors, seen_count=seen)               # ONE host read
    verts, faces, colors, info = cull_by_visibility((verts, faces), views, occluder="self")     # the three together
    l1, pixels = mesh_depth_l1(pred, gt, views)                                                 # the "Depth L1" column

The mirrors ARE the contract:

  * `render_mesh_depth_numpy` - tsdf.integrate_torch's projection in fp32 (one rounding per operation), vertices snapped
    to 1/256 pixel (round-half-even), int64 edge functions at the pixel centre (256 x, 256 y) multiplied by the sign of
    the doubled area, coverage iff all three are >= 0 (inclusive, two-sided, no top-left rule), perspective-correct depth
    as a chain of single fp64 roundings and one conversion to fp32, the winner of a pixel the minimum of the key
    (bits(z) << 32) | face.  Faces with a vertex at !(zc > z_near), a non-finite one, or one snapped beyond 2^24 are
    skipped for the view (there is NO near-plane clipping - that only makes the visibility test more permissive);
  * `vertex_visibility_torch` - zc > z_near, the rounded pixel inside the image and, with a depth plane d, not
    (zc - d) > eps; a pixel with !(d > 0) passes iff `empty_visible`; runs on CPU or GPU tensors;
  * `cull_mesh_numpy` - a face stays iff all / any of its vertices have seen_count >= min_views, a vertex iff a kept face
    names it, everything in its order.

Nothing in them depends on an execution order, so the device equals them bit for bit.  There is no CPU fall-back behind
render_mesh_depth / vertex_visibility / cull_mesh / cull_by_visibility / mesh_depth_l1: off the GPU they raise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _cabi
from ._device import compact_numpy, device_colors, device_rows, emit_compacted, ptr as _ptr, stream_ptr, workspace

RULES = ("all", "any")
SNAP_LIMIT = float(2 ** 24)          # |X|, |Y| of a snapped vertex, in 1/256 pixel
INFO_KEYS = ("verts_in", "faces_in", "verts_out", "faces_out", "bad_faces")
_F32_MAX = np.float32(np.finfo(np.float32).max)


def _check_image(what, H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{what}: H and W must be >= 1, got {H} x {W}")
    if H * W > _cabi.MESH_RENDER_MAX_PIXELS:
        raise ValueError(f"{what}: {H} x {W} pixels: H W must stay below 2^31")
    return H, W


def _check_rule(what, rule, min_views):
    if rule not in RULES:
        raise ValueError(f"{what}: rule must be one of {RULES}, got {rule!r}")
    return RULES.index(rule), int(min_views)


def _check_counts(what, V, F):
    if V > _cabi.MESH_EVAL_MAX_ITEMS or F > _cabi.MESH_EVAL_MAX_ITEMS:
        raise ValueError(f"{what}: {V} vertices / {F} faces: 3 V and 3 F must stay below 2^31")


def _as_numpy(x, dtype=None):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x if dtype is None else x.astype(dtype, copy=False)


def view_tuple(view):
    """(T_w2c, fx, fy, cx, cy, H, W) of a view given as that tuple or as a camera object that carries T, fx, fy, cx, cy
    and image_height / image_width."""
    if isinstance(view, (tuple, list)):
        if len(view) != 7:
            raise ValueError("a view is (T_w2c, fx, fy, cx, cy, H, W) or a camera object")
        T, fx, fy, cx, cy, H, W = view
    else:
        T, fx, fy, cx, cy = view.T, view.fx, view.fy, view.cx, view.cy
        H, W = view.image_height, view.image_width
    return T, float(fx), float(fy), float(cx), float(cy), int(H), int(W)


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def project_numpy(verts, T_w2c, fx, fy, cx, cy):
    """(u, v, zc) [V] f32 of tsdf.integrate_torch's projection, one fp32 rounding per operation."""
    v = np.ascontiguousarray(_as_numpy(verts, np.float32)).reshape(-1, 3)
    T = _as_numpy(T_w2c).astype(np.float32).reshape(4, 4)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        row = lambda r: ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
        xc, yc, zc = row(0), row(1), row(2)
        u = np.float32(fx) * (xc / zc) + np.float32(cx)
        w = np.float32(fy) * (yc / zc) + np.float32(cy)
    assert u.dtype == w.dtype == zc.dtype == np.float32
    return u, w, zc


def render_mesh_depth_numpy(verts, faces, T_w2c, fx, fy, cx, cy, H, W, z_near: float = 0.2,
                            large_threshold: int = _cabi.MESH_RENDER_LARGE_BOX):
    """(depth [H,W] f32, face_id [H,W] i32, record [4] i32) in plain NumPy, brute force over each face's clamped box: the
    contract of render_mesh_depth.  record = {bad faces, skipped faces, faces whose box holds more than
    `large_threshold` pixels, 0}."""
    H, W = _check_image("render_mesh_depth", H, W)
    v = np.ascontiguousarray(_as_numpy(verts, np.float32)).reshape(-1, 3)
    f = _as_numpy(faces).reshape(-1, 3).astype(np.int64)
    V, F = v.shape[0], f.shape[0]
    empty = np.uint64(2 ** 64 - 1)
    keys = np.full((H, W), empty, np.uint64)
    record = np.zeros(_cabi.MESH_RENDER_RECORD_INTS, np.int32)
    valid = ((f >= 0) & (f < V)).all(axis=1) if F else np.zeros(0, bool)
    record[0] = int((~valid).sum())
    if V and valid.any():
        u, w, zc = project_numpy(v, T_w2c, fx, fy, cx, cy)
        with np.errstate(all="ignore"):
            xs, ys = np.rint(u * np.float32(256.0)), np.rint(w * np.float32(256.0))       # round-half-even
            vok = (zc > np.float32(z_near)) & (zc <= _F32_MAX) & (np.abs(xs) <= SNAP_LIMIT) & (np.abs(ys) <= SNAP_LIMIT)
            X, Y = np.where(vok, xs, 0).astype(np.int64), np.where(vok, ys, 0).astype(np.int64)
            iz = np.where(vok, 1.0 / np.where(vok, zc, 1).astype(np.float64), 0.0)
        fs = np.where(valid[:, None], f, 0)
        fok = valid & vok[fs].all(axis=1)
        record[1] = int((valid & ~fok).sum())
        x, y = X[fs], Y[fs]
        a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        bx0, bx1 = np.maximum((x.min(axis=1) + 255) >> 8, 0), np.minimum(x.max(axis=1) >> 8, W - 1)
        by0, by1 = np.maximum((y.min(axis=1) + 255) >> 8, 0), np.minimum(y.max(axis=1) >> 8, H - 1)
        bw, bh = bx1 - bx0 + 1, by1 - by0 + 1
        draw = fok & (a2 != 0) & (bw >= 1) & (bh >= 1)
        record[2] = int((draw & (bw * bh > int(large_threshold))).sum())
        edge = lambda ax, ay, bx, by, px, py: (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        for i in np.flatnonzero(draw):
            s = 1 if a2[i] > 0 else -1
            px = (256 * np.arange(bx0[i], bx1[i] + 1, dtype=np.int64))[None, :]
            py = (256 * np.arange(by0[i], by1[i] + 1, dtype=np.int64))[:, None]
            (x0, x1, x2), (y0, y1, y2), (i0, i1, i2) = x[i], y[i], iz[fs[i]]
            w0, w1, w2 = s * edge(x1, y1, x2, y2, px, py), s * edge(x2, y2, x0, y0, px, py), s * edge(x0, y0, x1, y1, px, py)
            cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
            with np.errstate(all="ignore"):
                den = (w0.astype(np.float64) * i0 + w1.astype(np.float64) * i1) + w2.astype(np.float64) * i2
                z = (np.float64(abs(int(a2[i]))) / den).astype(np.float32)
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(i)
            sub = keys[by0[i]:by1[i] + 1, bx0[i]:bx1[i] + 1]
            np.minimum(sub, np.where(cov, key, empty), out=sub)
    hit = keys != empty
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0.0)).astype(np.float32)
    face_id = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth, face_id, record


def vertex_visibility_torch(verts, T_w2c, fx, fy, cx, cy, H, W, depth=None, eps: float = 0.05,
                            empty_visible: bool = True, z_near: float = 0.2, out=None):
    """seen_count [V] i32 (zeros when `out` is None, else `out` incremented in place) in eager fp32 torch, on the device
    of `verts`: the contract of vertex_visibility."""
    H, W = _check_image("vertex_visibility", H, W)
    v = torch.as_tensor(verts).detach().to(torch.float32).reshape(-1, 3)
    dev = v.device
    f = lambda s: torch.tensor(float(s), dtype=torch.float32, device=dev)
    T = torch.as_tensor(T_w2c).detach().to(dev, torch.float32).reshape(4, 4)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    row = lambda r: ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    xc, yc, zc = row(0), row(1), row(2)
    ok = zc > f(z_near)
    u = f(fx) * (xc / zc) + f(cx)
    w = f(fy) * (yc / zc) + f(cy)
    uf, wf = torch.floor(u + f(0.5)), torch.floor(w + f(0.5))
    ok = ok & (uf >= 0) & (uf < float(W)) & (wf >= 0) & (wf < float(H))
    if depth is not None:
        d = torch.as_tensor(depth).detach().to(dev, torch.float32).reshape(-1)
        if d.numel() != H * W:
            raise ValueError(f"vertex_visibility: depth must be [{H},{W}]")
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        pix = torch.where(ok, wf, zero).long() * W + torch.where(ok, uf, zero).long()
        dv = d[pix]
        empty = torch.full_like(ok, bool(empty_visible))
        ok = ok & torch.where(dv > 0, ~((zc - dv) > f(eps)), empty)
    if out is None:
        out = torch.zeros(v.shape[0], dtype=torch.int32, device=dev)
    out += ok.to(torch.int32)
    return out


def cull_mesh_numpy(verts, faces, colors=None, seen_count=None, min_views: int = 1, rule: str = "all"):
    """(verts, faces, colors | None, info) in plain NumPy: the contract of cull_mesh."""
    any_rule, min_views = _check_rule("cull_mesh", rule, min_views)
    v = np.ascontiguousarray(_as_numpy(verts, np.float32)).reshape(-1, 3)
    f = _as_numpy(faces).reshape(-1, 3).astype(np.int64)
    V, F = v.shape[0], f.shape[0]
    if seen_count is None:
        raise ValueError("cull_mesh: seen_count [V] is required")
    seen = _as_numpy(seen_count).reshape(-1).astype(np.int64)
    if seen.shape[0] != V:
        raise ValueError(f"cull_mesh: seen_count must be [{V}]")
    col = None if colors is None else np.ascontiguousarray(_as_numpy(colors, np.float32)).reshape(V, 3)
    valid = ((f >= 0) & (f < V)).all(axis=1) if F else np.zeros(0, bool)
    fs = np.where(valid[:, None], f, 0)
    ok = (seen >= min_views)[fs] if V else np.zeros((F, 3), bool)
    fkeep = valid & (ok.any(axis=1) if any_rule else ok.all(axis=1))
    vkeep = np.zeros(V, bool)
    vkeep[f[fkeep].reshape(-1)] = True
    info = dict(verts_in=V, faces_in=F, verts_out=int(vkeep.sum()), faces_out=int(fkeep.sum()),
                bad_faces=int((~valid).sum()))
    return compact_numpy(v, f, col, vkeep, fkeep) + (info,)


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "render_mesh_depth_numpy / vertex_visibility_torch / cull_mesh_numpy"


def _device_rows(t, what, name, dtype, dev=None):
    return device_rows(t, what, name, _MIRRORS, dtype, dev)


def _device_pose(T, what, dev):
    T = torch.as_tensor(T).detach()
    if tuple(T.shape) != (4, 4):
        raise ValueError(f"{what}: T_w2c must be [4,4], got {tuple(T.shape)}")
    return T.to(dev, torch.float32).contiguous()


def render_mesh_depth(verts, faces, T_w2c, fx, fy, cx, cy, H, W, z_near: float = 0.2,
                      large_threshold: int = _cabi.MESH_RENDER_LARGE_BOX, large_grid: int = _cabi.MESH_RENDER_LARGE_GRID):
    """(depth [H,W] f32, face_id [H,W] i32, record [4] i32) on the device of `verts`: the nearest surface of the mesh
    through every pixel centre of the pinhole view (module docstring); depth 0 and face id -1 without one.  record =
    {bad faces, skipped faces, faces drawn by the large-face launch, 0}.  Four launches, no host read.  A face whose
    clamped box holds more than `large_threshold` pixels is drawn by a workgroup instead of a lane, by `large_grid`
    workgroups that stride the list of such faces; neither changes the image."""
    what = "render_mesh_depth"
    verts = _device_rows(verts, what, "verts", torch.float32)
    dev = verts.device
    faces = _device_rows(faces, what, "faces", torch.int32, dev)
    H, W = _check_image(what, H, W)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    _check_counts(what, V, F)
    large_threshold, large_grid = int(large_threshold), int(large_grid)
    if large_threshold < 0 or large_grid < 1:
        raise ValueError(f"{what}: large_threshold must be >= 0 and large_grid >= 1")
    T = _device_pose(T_w2c, what, dev)
    L = _cabi.lib()
    scratch, _ = workspace("render", dev, (H, W, F), L.mgs_mesh_render_scratch_bytes,
                           f"{what}: {H} x {W} pixels / {F} faces: H W and 3 F must stay below 2^31")
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    face_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    record = torch.empty(_cabi.MESH_RENDER_RECORD_INTS, dtype=torch.int32, device=dev)
    a = _cabi.MeshRenderArgs()
    a.num_verts, a.num_faces, a.width, a.height = V, F, W, H
    a.large_threshold, a.large_grid = min(large_threshold, 2 ** 31 - 1), min(large_grid, 65535)
    a.fx, a.fy, a.cx, a.cy, a.z_near = float(fx), float(fy), float(cx), float(cy), float(z_near)
    a.verts, a.faces, a.T, a.scratch = _ptr(verts), _ptr(faces), T.data_ptr(), scratch.data_ptr()
    a.depth, a.face_id, a.record = depth.data_ptr(), face_id.data_ptr(), record.data_ptr()
    _cabi.check(L.mgs_mesh_render(C.byref(a), stream_ptr(dev)), "mgs_mesh_render")
    return depth, face_id, record


def vertex_visibility(verts, T_w2c, fx, fy, cx, cy, H, W, depth=None, eps: float = 0.05, empty_visible: bool = True,
                      z_near: float = 0.2, out=None):
    """seen_count [V] i32 on the device of `verts`: `out` (zeros when None) with one added for every vertex this view
    sees - zc > z_near, the rounded pixel inside the image and, with `depth` [H,W] (a rendered or a sensor depth plane),
    not more than `eps` behind it; a pixel without depth passes iff `empty_visible`.  depth=None is the frustum-only
    protocol.  One launch, one thread per vertex, no atomics, no host read.

    eps = 0.05 is this project's choice: it equals evaluate_mesh's default threshold, in the units of the mesh."""
    what = "vertex_visibility"
    verts = _device_rows(verts, what, "verts", torch.float32)
    dev = verts.device
    H, W = _check_image(what, H, W)
    V = int(verts.shape[0])
    _check_counts(what, V, 0)
    T = _device_pose(T_w2c, what, dev)
    if depth is not None:
        if not torch.is_tensor(depth) or depth.device != dev or depth.numel() != H * W:
            raise ValueError(f"{what}: depth must be [{H},{W}] on the device of verts")
        depth = depth.detach().to(torch.float32).contiguous()
    if out is None:
        out = torch.zeros(V, dtype=torch.int32, device=dev)
    elif (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.int32 or tuple(out.shape) != (V,)
          or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous int32 tensor [{V}] on the device of verts")
    a = _cabi.VertexVisibilityArgs()
    a.num_verts, a.width, a.height, a.empty_visible = V, W, H, 1 if empty_visible else 0
    a.fx, a.fy, a.cx, a.cy, a.z_near, a.eps = float(fx), float(fy), float(cx), float(cy), float(z_near), float(eps)
    a.verts, a.T, a.depth, a.seen_count = _ptr(verts), T.data_ptr(), (None if depth is None else depth.data_ptr()), _ptr(out)
    _cabi.check(_cabi.lib().mgs_vertex_visibility(C.byref(a), stream_ptr(dev)), "mgs_vertex_visibility")
    return out


def cull_mesh(verts, faces, colors=None, seen_count=None, min_views: int = 1, rule: str = "all"):
    """(verts [V',3] f32, faces [F',3] i32, colors [V',3] f32 | None, info) on the device: the faces of which all
    (rule="all") or any (rule="any") vertices have seen_count >= min_views, the vertices they name, both in their order,
    the faces re-indexed.  A face with an index outside [0,V) is dropped and counted (info["bad_faces"]).  One host read,
    of the counts, between the scan and the emission."""
    what = "cull_mesh"
    any_rule, min_views = _check_rule(what, rule, min_views)
    faces = _device_rows(faces, what, "faces", torch.int32)
    dev = faces.device
    verts = _device_rows(verts, what, "verts", torch.float32, dev)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    _check_counts(what, V, F)
    if not torch.is_tensor(seen_count) or seen_count.device != dev or tuple(seen_count.shape) != (V,):
        raise ValueError(f"{what}: seen_count must be [{V}] on the device of faces")
    seen_count = seen_count.detach().to(torch.int32).contiguous()
    colors = device_colors(colors, what, V, dev)
    L = _cabi.lib()
    scratch, counts = workspace("cull", dev, (V, F), L.mgs_mesh_cull_scratch_bytes,
                                f"{what}: {V} vertices / {F} faces: 3 V and 3 F must stay below 2^31", _cabi.MESH_CULL_COUNTS)
    a = _cabi.MeshCullArgs()
    a.num_verts, a.num_faces, a.rule = V, F, any_rule
    a.min_views = max(-2 ** 31, min(min_views, 2 ** 31 - 1))
    a.faces, a.seen_count, a.scratch, a.counts = _ptr(faces), _ptr(seen_count), scratch.data_ptr(), counts.data_ptr()
    _cabi.check(L.mgs_mesh_cull_count(C.byref(a), stream_ptr(dev)), "mgs_mesh_cull_count")
    V2, F2, bad, _ = (int(c) for c in counts.cpu())              # the one host read
    out_v, out_f, out_c = emit_compacted(a, L.mgs_mesh_cull_emit, "mgs_mesh_cull_emit", verts, colors, V2, F2)
    return out_v, out_f, out_c, dict(verts_in=V, faces_in=F, verts_out=V2, faces_out=F2, bad_faces=bad)


# ---- the protocol ----------------------------------------------------------------------------------------------------
def _numpy_render(v, f, view, z_near):
    T, fx, fy, cx, cy, H, W = view
    return render_mesh_depth_numpy(v, f, T, fx, fy, cx, cy, H, W, z_near)[0]


def _device_render(v, f, view, z_near):
    T, fx, fy, cx, cy, H, W = view
    return render_mesh_depth(v, f, T, fx, fy, cx, cy, H, W, z_near)[0]


def _cull_by_visibility(mirror, mesh, views, occluder, depth_planes, eps, min_views, rule, empty_visible, z_near):
    what = "cull_by_visibility"
    _check_rule(what, rule, min_views)
    if not isinstance(mesh, (tuple, list)) or len(mesh) not in (2, 3):
        raise ValueError(f"{what}: mesh is (verts, faces) or (verts, faces, colors)")
    verts, faces = mesh[0], mesh[1]
    colors = mesh[2] if len(mesh) == 3 else None
    views = [view_tuple(v) for v in views]
    if depth_planes is not None and len(depth_planes) != len(views):
        raise ValueError(f"{what}: depth_planes must hold one plane per view")
    if isinstance(occluder, str):
        if occluder != "self":
            raise ValueError(f'{what}: occluder is "self", a (verts, faces) mesh or None')
        occluder = (verts, faces)
    render = _numpy_render if mirror else _device_render
    visible = vertex_visibility_torch if mirror else vertex_visibility
    if mirror:
        verts = torch.from_numpy(np.ascontiguousarray(_as_numpy(verts, np.float32)).reshape(-1, 3))
    seen = None
    for k, view in enumerate(views):
        depth = None
        if depth_planes is not None:
            depth = depth_planes[k]
        elif occluder is not None:
            depth = render(occluder[0], occluder[1], view, z_near)
        if mirror and depth is not None:
            depth = torch.as_tensor(_as_numpy(depth, np.float32))
        T, fx, fy, cx, cy, H, W = view
        seen = visible(verts, T, fx, fy, cx, cy, H, W, depth=depth, eps=eps, empty_visible=empty_visible, z_near=z_near,
                       out=seen)
    if seen is None:                                               # no view: nothing was seen
        seen = torch.zeros(int(verts.shape[0]), dtype=torch.int32, device=verts.device)
    if mirror:
        return cull_mesh_numpy(verts.numpy(), faces, colors, seen_count=seen.numpy(), min_views=min_views, rule=rule)
    return cull_mesh(verts, faces, colors, seen_count=seen, min_views=min_views, rule=rule)


def cull_by_visibility(mesh, views, occluder="self", depth_planes=None, eps: float = 0.05, min_views: int = 1,
                       rule: str = "all", empty_visible: bool = True, z_near: float = 0.2):
    """(verts, faces, colors | None, info) on the device: `mesh` = (verts, faces[, colors]) without what fewer than
    `min_views` of `views` saw.  `views` is a list of (T_w2c, fx, fy, cx, cy, H, W) or of camera objects (view_tuple).
    Per view the depth of the `occluder` - "self", another (verts, faces) mesh, or None for the frustum-only test - is
    rendered (render_mesh_depth) unless `depth_planes` supplies one plane per view (sensor depth), and
    vertex_visibility accumulates; cull_mesh runs once at the end (its one host read)."""
    return _cull_by_visibility(False, mesh, views, occluder, depth_planes, eps, min_views, rule, empty_visible, z_near)


def cull_by_visibility_numpy(mesh, views, occluder="self", depth_planes=None, eps: float = 0.05, min_views: int = 1,
                             rule: str = "all", empty_visible: bool = True, z_near: float = 0.2):
    """cull_by_visibility through the mirrors, on the host."""
    return _cull_by_visibility(True, mesh, views, occluder, depth_planes, eps, min_views, rule, empty_visible, z_near)


def cull_pair(mirror, pred, gt, views, occlusion="gt", eps: float = 0.05, min_views: int = 1, rule: str = "all",
              empty_visible: bool = True, z_near: float = 0.2):
    """((pred verts, faces), (gt verts, faces), culled pred faces, culled gt faces): both meshes, in the ground truth's
    frame, culled against the same views.  occlusion "gt" tests both against the ground truth's rendered depth (rendered
    once per view), "self" each against its own, None is the frustum-only test.  A bad face raises ValueError."""
    if occlusion not in ("gt", "self", None):
        raise ValueError(f'evaluate_mesh: cull occlusion is "gt", "self" or None, got {occlusion!r}')
    views = [view_tuple(v) for v in views]
    planes = None
    if occlusion == "gt":
        planes = [(_numpy_render if mirror else _device_render)(gt[0], gt[1], view, z_near) for view in views]
    occluder = "self" if occlusion == "self" else None
    out, dropped = [], []
    for name, mesh in (("pred", pred), ("gt", gt)):
        v, f, _, info = _cull_by_visibility(mirror, (mesh[0], mesh[1]), views, occluder, planes, eps, min_views, rule,
                                            empty_visible, z_near)
        if info["bad_faces"]:
            raise ValueError(f"evaluate_mesh: {info['bad_faces']} faces of the {name} mesh hold an index outside [0, V)")
        out.append((v, f))
        dropped.append(info["faces_in"] - info["faces_out"])
    return out[0], out[1], dropped[0], dropped[1]


def _mesh_depth_l1(mirror, pred, gt, views, transform, z_near):
    from .mesh_eval import apply_transform
    views = [view_tuple(v) for v in views]
    render = _numpy_render if mirror else _device_render
    if mirror:
        pv = apply_transform(torch.from_numpy(np.ascontiguousarray(_as_numpy(pred[0], np.float32)).reshape(-1, 3)), transform)
    else:
        pv = apply_transform(_device_rows(pred[0], "mesh_depth_l1", "pred verts", torch.float32), transform)
    sums, counts = [], []
    for view in views:
        dp, dg = (torch.as_tensor(render(v, f, view, z_near)) for v, f in ((pv, pred[1]), (gt[0], gt[1])))
        both = (dp > 0) & (dg > 0)
        sums.append(torch.where(both, (dp - dg).abs(), torch.zeros_like(dp)).to(torch.float64).sum())
        counts.append(both.sum())
    if not views:
        return float("nan"), 0
    rec = torch.stack([torch.stack(sums), torch.stack(counts).to(torch.float64)]).cpu().numpy()      # the one host read
    used = rec[1] > 0
    value = float((rec[0][used] / rec[1][used]).mean()) if used.any() else float("nan")
    return value, int(rec[1].sum())


def mesh_depth_l1(pred, gt, views, transform=None, z_near: float = 0.2):
    """(depth L1, pixels used): the mean over `views` of the mean |d_pred - d_gt| over the pixels where both meshes'
    rendered depths are positive - the "Depth L1" column of the reconstruction tables, in the units of the meshes.
    `transform` (mesh_eval.apply_transform) moves pred's vertices into gt's frame first.  A view without a common pixel
    is left out of the mean; NaN when none has one.  The reduction is torch on the device; one host read at the end."""
    return _mesh_depth_l1(False, pred, gt, views, transform, z_near)


def mesh_depth_l1_numpy(pred, gt, views, transform=None, z_near: float = 0.2):
    """mesh_depth_l1 through the mirror render, on the host."""
    return _mesh_depth_l1(True, pred, gt, views, transform, z_near)


# ---- frames ----------------------------------------------------------------------------------------------------------
FRAME_MODES = ("shaded", "normal", "color", "depth")


def _quantise(x):
    """trunc(clamp(x, 0, 1) 255) in fp32, a NaN black: the viewer's rgb rule (viewer.compose_torch)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        x = np.clip(np.where(np.isnan(x), np.float32(0.0), x), np.float32(0.0), np.float32(1.0))
        return (x * np.float32(255.0)).astype(np.uint8)


def _frame_arguments(what, mode, colors, background, V):
    if mode not in FRAME_MODES:
        raise ValueError(f"{what}: mode must be one of {FRAME_MODES}, got {mode!r}")
    if mode == "color":
        if colors is None:
            raise ValueError(f'{what}: mode "color" needs colors [V,3]')
        if tuple(colors.shape) != (V, 3):
            raise ValueError(f"{what}: colors must be [{V},3], got {tuple(colors.shape)}")
    bg = _quantise(np.asarray(background, np.float32).reshape(-1))
    if bg.shape != (3,):
        raise ValueError(f"{what}: background is (r, g, b) in [0, 1]")
    return bg


def render_mesh_frame_numpy(verts, faces, view, mode: str = "shaded", colors=None, background=(0.0, 0.0, 0.0),
                            z_near: float = 0.2):
    """uint8 [H,W,3] in plain NumPy on top of render_mesh_depth_numpy: the contract of render_mesh_frame."""
    from .mesh_normals import face_normals_numpy
    what = "render_mesh_frame"
    T, fx, fy, cx, cy, H, W = view_tuple(view)
    v = np.ascontiguousarray(_as_numpy(verts, np.float32)).reshape(-1, 3)
    f = _as_numpy(faces).reshape(-1, 3).astype(np.int64)
    if colors is not None:
        colors = _as_numpy(colors)
    bg = _frame_arguments(what, mode, colors, background, v.shape[0])
    depth, face_id, _ = render_mesh_depth_numpy(v, f, T, fx, fy, cx, cy, H, W, z_near)
    hit = face_id >= 0
    fid = np.where(hit, face_id, 0)
    out = np.empty((H, W, 3), np.uint8)
    out[:] = bg
    if mode == "depth":
        from .viewer import compose_torch
        return np.where(hit[:, :, None], compose_torch(torch.from_numpy(depth), "depth").numpy(), out)
    if not hit.any():
        return out
    T = _as_numpy(T).astype(np.float32).reshape(4, 4)
    with np.errstate(all="ignore"):
        if mode == "color":
            col = colors.astype(np.float32) / np.float32(255.0) if colors.dtype == np.uint8 else colors.astype(np.float32)
            u, w, zc = project_numpy(v, T, fx, fy, cx, cy)
            X, Y = np.rint(u * np.float32(256.0)), np.rint(w * np.float32(256.0))
            ys, xs = np.nonzero(hit)
            tri = f[fid[ys, xs]]                                                  # [n,3]: drawn faces, so every vertex is good
            x, y = X[tri].astype(np.int64), Y[tri].astype(np.int64)
            iz = 1.0 / zc[tri].astype(np.float64)
            a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
            s = np.where(a2 > 0, 1, -1)
            px, py = 256 * xs.astype(np.int64), 256 * ys.astype(np.int64)
            edge = lambda a, b: s * ((x[:, b] - x[:, a]) * (py - y[:, a]) - (y[:, b] - y[:, a]) * (px - x[:, a]))
            t = [edge(1, 2).astype(np.float64) * iz[:, 0], edge(2, 0).astype(np.float64) * iz[:, 1],
                 edge(0, 1).astype(np.float64) * iz[:, 2]]
            den = (t[0] + t[1]) + t[2]
            c = col[tri].astype(np.float64)                                       # [n,3 corners,3 channels]
            num = (t[0][:, None] * c[:, 0] + t[1][:, None] * c[:, 1]) + t[2][:, None] * c[:, 2]
            out[ys, xs] = _quantise((num / den[:, None]).astype(np.float32))
            return out
        n = face_normals_numpy(v, f)[0][fid]                                      # [H,W,3]
        nc = [(T[r, 0] * n[..., 0] + T[r, 1] * n[..., 1]) + T[r, 2] * n[..., 2] for r in range(3)]
        if mode == "shaded":
            grey = _quantise(np.float32(0.25) + np.float32(0.75) * np.abs(nc[2]))
            rgb = np.stack([grey, grey, grey], -1)
        else:
            rx = ((np.arange(W, dtype=np.float32) - np.float32(cx)) / np.float32(fx))[None, :]
            ry = ((np.arange(H, dtype=np.float32) - np.float32(cy)) / np.float32(fy))[:, None]
            away = ((nc[0] * rx + nc[1] * ry) + nc[2]) > 0
            rgb = np.stack([_quantise(np.float32(0.5) * np.where(away, -c, c) + np.float32(0.5)) for c in nc], -1)
        assert nc[0].dtype == np.float32
    return np.where(hit[:, :, None], rgb, out)


def render_mesh_frame(verts, faces, view, mode: str = "shaded", colors=None, background=(0.0, 0.0, 0.0),
                      z_near: float = 0.2):
    """uint8 [H,W,3] on the device of `verts`: a picture of the mesh at `view` (what view_tuple accepts).
    render_mesh_depth runs first, then face_normals where the mode needs them, then ONE launch, one lane per pixel; no
    host read.  A pixel without a face gets `background` (r, g, b in [0, 1]); every channel is quantised as the viewer's
    rgb frames are, trunc(clamp(x, 0, 1) 255).  With n_c the face's unit normal in the camera frame:

      "shaded"  grey 0.25 + 0.75 |n_c.z|: a headlight, the same from both sides of a face;
      "normal"  0.5 n_c + 0.5 as rgb, n_c turned to face the camera - surface.depth_normal_torch's orientation: its
                normal is (d/dy) x (d/dx) of the back-projected depth, which always has n . ray < 0 - so n_c is negated
                where n_c . ((x - cx) / fx, (y - cy) / fy, 1) > 0, and a wall seen head-on is (127, 127, 0) in both;
      "color"   the vertex colours `colors` [V,3] (fp32 in [0, 1], or uint8), interpolated perspective-correctly with
                the renderer's own edge functions and inverse depths;
      "depth"   the viewer's depth view of the rendered depth (jet between 0.1 and the largest depth)."""
    from .mesh_normals import face_normals
    what = "render_mesh_frame"
    T, fx, fy, cx, cy, H, W = view_tuple(view)
    verts = _device_rows(verts, what, "verts", torch.float32)
    dev = verts.device
    faces = _device_rows(faces, what, "faces", torch.int32, dev)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if colors is not None:
        if not torch.is_tensor(colors) or colors.device != dev:
            raise ValueError(f"{what}: colors must be on the device of verts")
        colors = colors.detach().contiguous() if colors.dtype == torch.uint8 else colors.detach().to(torch.float32).contiguous()
    bg = _frame_arguments(what, mode, colors, background, V)
    H, W = _check_image(what, H, W)
    if 3 * H * W > _cabi.MESH_RENDER_MAX_PIXELS:
        raise ValueError(f"{what}: {H} x {W} pixels: 3 H W must stay below 2^31")
    depth, face_id, _ = render_mesh_depth(verts, faces, T, fx, fy, cx, cy, H, W, z_near)
    T = _device_pose(T, what, dev)
    L = _cabi.lib()
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    a = _cabi.MeshShadeArgs()
    a.num_verts, a.num_faces, a.width, a.height = V, F, W, H
    a.fx, a.fy, a.cx, a.cy, a.z_near = float(fx), float(fy), float(cx), float(cy), float(z_near)
    a.background[0], a.background[1], a.background[2] = (int(b) for b in bg)
    a.T, a.face_id, a.out = T.data_ptr(), face_id.data_ptr(), out.data_ptr()
    keep = None
    if mode == "depth":
        from .viewer import _lut
        lut = _lut(dev).contiguous()
        keep = (lut, torch.empty(int(L.mgs_view_compose_scratch_bytes()), dtype=torch.uint8, device=dev))
        c = _cabi.ViewComposeArgs()
        c.width, c.height, c.mode = W, H, _cabi.VIEW_DEPTH
        c.src, c.lut, c.out, c.scratch = depth.data_ptr(), lut.data_ptr(), out.data_ptr(), keep[1].data_ptr()
        _cabi.check(L.mgs_view_compose(C.byref(c), stream_ptr(dev)), "mgs_view_compose")
        a.mode = _cabi.MESH_SHADE_MASK
    elif mode == "color":
        a.mode, a.colors_u8 = _cabi.MESH_SHADE_COLOR, 1 if colors.dtype == torch.uint8 else 0
        a.verts, a.faces, a.colors = _ptr(verts), _ptr(faces), _ptr(colors)
    else:
        keep = face_normals(verts, faces)[0]
        a.mode = _cabi.MESH_SHADE_SHADED if mode == "shaded" else _cabi.MESH_SHADE_NORMAL
        a.face_normal = _ptr(keep)
    _cabi.check(L.mgs_mesh_shade(C.byref(a), stream_ptr(dev)), "mgs_mesh_shade")
    return out
