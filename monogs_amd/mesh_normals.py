"""Mesh normals: unit normals of faces and area-weighted normals of vertices - on the device (csrc/mesh_normals.hip; the
contract is in include/monogs_raster.h and DESIGN.md "Mesh normals").

    normal, record = face_normals(verts, faces)        # [F,3] f32, [2] i32 {bad faces, degenerate faces}; no host read
    normal, record = vertex_normals(verts, faces)      # [V,3] f32, the same record; no host read

mesh_eval.evaluate_mesh(normals=True) scores normal consistency with the first, eval_native.save_mesh(normals=True)
writes the second into mesh.ply, mesh_render.render_mesh_frame shades with the first.

The mirrors ARE the contract:

  * `face_normals_numpy` - the cross product of mesh_eval.face_weights_numpy (every product and difference its own fp32
    rounding), L = sqrt((cx^2 + cy^2) + cz^2), n = c / L.  A face with an index outside [0,V) is bad, a face whose L is 0
    or not finite is degenerate; both get (0,0,0) and are counted;
  * `vertex_normals_numpy` - the sum over the faces that name the vertex of their un-normalised cross products, in fixed
    point: with E the binary exponent of the largest |component| of any usable face, q = trunc(c 2^(30 - E)) (exact in
    fp64, |q| < 2^31) is added to int64 sums, which no F < 2^31 can overflow; n = s / sqrt((sx^2 + sy^2) + sz^2) in
    fp64, one conversion to fp32; (0,0,0) where the sum is zero.  A face with a non-finite component or with
    c = (0,0,0) is degenerate here and left out.

The consequence of the fixed point: a face whose cross product is below 2^-30 of the largest contributes nothing.  That
is the sampler's rule for areas, and harmless on extracted meshes, whose faces are of one size.

Sums of integers do not depend on their order, so the device equals the mirrors bit for bit, and itself from run to run.
There is no CPU fall-back behind face_normals / vertex_normals: off the GPU they raise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _cabi
from ._device import device_rows, ptr as _ptr, stream_ptr, workspace


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def face_cross_numpy(verts, faces):
    """(c [F,3] f32, valid [F] bool): (b - a) x (c - a) of every face in single fp32 roundings (zeros where an index
    lies outside [0,V): not valid)."""
    v = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V, F = v.shape[0], f.shape[0]
    valid = ((f >= 0) & (f < V)).all(axis=1) if F else np.zeros(0, bool)
    c = np.zeros((F, 3), np.float32)
    if F == 0 or V == 0:
        return c, valid
    fs = np.where(valid[:, None], f, 0)
    with np.errstate(all="ignore"):
        a, b, d = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
        e, g = b - a, d - a
        c[:, 0] = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
        c[:, 1] = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
        c[:, 2] = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
    c[~valid] = 0
    return c, valid


def face_normals_numpy(verts, faces):
    """(normal [F,3] f32, record [2] i32 {bad faces, degenerate faces}) in plain NumPy: the contract of face_normals."""
    c, valid = face_cross_numpy(verts, faces)
    with np.errstate(all="ignore"):
        L = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        ok = valid & np.isfinite(L) & (L > 0)
        n = np.where(ok[:, None], c / np.where(ok, L, np.float32(1.0))[:, None], np.float32(0.0))
    assert L.dtype == n.dtype == np.float32
    return n, np.array([(~valid).sum(), (valid & ~ok).sum()], np.int32)


def vertex_normals_numpy(verts, faces):
    """(normal [V,3] f32, record [2] i32 {bad faces, degenerate faces}) in plain NumPy: the contract of vertex_normals
    (module docstring)."""
    V = np.asarray(verts).reshape(-1, 3).shape[0]
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    c, valid = face_cross_numpy(verts, faces)
    use = valid & np.isfinite(c).all(axis=1) & (c != 0).any(axis=1)
    record = np.array([(~valid).sum(), (valid & ~use).sum()], np.int32)
    s = np.zeros((V, 3), np.int64)
    if use.any():
        amax = float(np.abs(c[use]).view(np.uint32).max().view(np.float32))       # the integer maximum of the bits
        E = int(np.frexp(amax)[1]) - 1
        q = np.trunc(np.ldexp(c[use].astype(np.float64), 30 - E)).astype(np.int64)
        for k in range(3):
            np.add.at(s, f[use, k], q)
    s = s.astype(np.float64)
    L = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    ok = L > 0
    n = np.where(ok[:, None], s / np.where(ok, L, 1.0)[:, None], 0.0).astype(np.float32)
    return n, record


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "face_normals_numpy / vertex_normals_numpy"


def _mesh_arguments(what, verts, faces):
    verts = device_rows(verts, what, "verts", _MIRRORS, torch.float32)
    dev = verts.device
    faces = device_rows(faces, what, "faces", _MIRRORS, torch.int32, dev)
    a = _cabi.MeshNormalsArgs()
    a.num_verts, a.num_faces = int(verts.shape[0]), int(faces.shape[0])
    a.verts, a.faces = _ptr(verts), _ptr(faces)
    record = torch.empty(_cabi.MESH_NORMAL_RECORD_INTS, dtype=torch.int32, device=dev)
    a.record = record.data_ptr()
    return a, dev, record, (verts, faces)


def face_normals(verts, faces):
    """(normal [F,3] f32, record [2] i32) on the device of `verts`: the unit normal (b - a) x (c - a) / |.| of every face
    (module docstring); (0,0,0) for a bad or degenerate face.  record = {bad faces, degenerate faces}.  One launch, one
    lane per face, no host read."""
    a, dev, record, keep = _mesh_arguments("face_normals", verts, faces)
    normal = torch.empty(a.num_faces, 3, dtype=torch.float32, device=dev)
    a.normals = _ptr(normal)
    _cabi.check(_cabi.lib().mgs_face_normals(C.byref(a), stream_ptr(dev)), "mgs_face_normals")
    return normal, record


def vertex_normals(verts, faces):
    """(normal [V,3] f32, record [2] i32) on the device of `verts`: the area-weighted normal of every vertex, summed in
    fixed point by integer atomics and therefore the same bits in every run (module docstring); (0,0,0) for a vertex no
    usable face names or whose faces cancel.  A face whose cross product is below 2^-30 of the mesh's largest contributes
    nothing.  record = {bad faces, degenerate faces}.  Three launches, no host read."""
    what = "vertex_normals"
    a, dev, record, keep = _mesh_arguments(what, verts, faces)
    L = _cabi.lib()
    scratch, _ = workspace("vertex_normals", dev, (a.num_verts,), L.mgs_vertex_normals_scratch_bytes,
                           f"{what}: {a.num_verts} vertices: 3 V must stay below 2^31")
    normal = torch.empty(a.num_verts, 3, dtype=torch.float32, device=dev)
    a.scratch, a.normals = scratch.data_ptr(), _ptr(normal)
    _cabi.check(L.mgs_vertex_normals(C.byref(a), stream_ptr(dev)), "mgs_vertex_normals")
    return normal, record
