"""Mesh clean-up: connected components of an indexed triangle mesh, clusters kept by size, vertices / colours / faces
compacted, on the device (csrc/mesh_clean.hip; the contract is in include/monogs_raster.h and DESIGN.md "Mesh clean-up").

    verts, faces, colors = vol.extract_mesh()
    verts, faces, colors, info = clean_mesh(verts, faces, colors, keep_largest=1)     # ONE host read, of the counts
    labels = connected_components(verts.shape[0], faces)                              # [V] i32, no host read

The mirrors `clean_mesh_numpy` and `connected_components_numpy` ARE the contract:

  * two vertices are connected when a face names both; the label of a vertex is the smallest vertex index of its
    component (a vertex no face names is its own label, with a cluster of 0 faces);
  * the size of a cluster is its number of faces, a face belonging to the cluster of its first index; degenerate and
    duplicate faces are ordinary faces;
  * a cluster is kept iff faces >= max(min_faces, 1) and, with `keep_largest`, its rank in the order (face count
    descending, label ascending) is < keep_largest;
  * the kept vertices, colours and faces keep their relative order; the faces are re-indexed;
  * a face with an index outside [0,V) connects nothing and is never emitted; its presence raises ValueError.

Nothing in this depends on an execution order, so the device's output equals the mirror's bit for bit.  There is no CPU
fall-back behind clean_mesh / connected_components: off the GPU they raise."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _cabi
from ._device import compact_numpy, device_colors, device_rows, emit_compacted, stream_ptr, workspace

INFO_KEYS = ("num_clusters", "kept_clusters", "verts_in", "faces_in", "verts_out", "faces_out")


def _check_params(keep_largest, min_faces):
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError(f"keep_largest must be None or >= 0, got {keep_largest}")
    if int(min_faces) < 0:
        raise ValueError(f"min_faces must be >= 0, got {min_faces}")
    return (None if keep_largest is None else int(keep_largest)), int(min_faces)


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def _faces_numpy(num_verts, faces):
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    valid = ((f >= 0) & (f < int(num_verts))).all(axis=1) if f.shape[0] else np.zeros(0, bool)
    return f, valid


def connected_components_numpy(num_verts: int, faces) -> np.ndarray:
    """labels [V] i32: the smallest vertex index of each vertex's component.  Hook the larger root of every edge to the
    smallest root it meets, compress every path to its root, repeat until no edge joins two roots."""
    V = int(num_verts)
    f, valid = _faces_numpy(V, faces)
    f = f[valid]
    a = np.concatenate([f[:, 0], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    p = np.arange(V, dtype=np.int64)
    while True:
        pa, pb = p[a], p[b]
        m = pa != pb
        if not m.any():
            break
        a, b, pa, pb = a[m], b[m], pa[m], pb[m]          # an edge inside one tree stays inside it
        np.minimum.at(p, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
    return p.astype(np.int32)


def clean_mesh_numpy(verts, faces, colors=None, keep_largest: Optional[int] = None, min_faces: int = 0):
    """(verts, faces, colors | None, info) in plain NumPy: the contract of clean_mesh."""
    keep_largest, min_faces = _check_params(keep_largest, min_faces)
    v = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3)
    V = v.shape[0]
    f, valid = _faces_numpy(V, faces)
    F = f.shape[0]
    if not valid.all():
        raise ValueError(f"clean_mesh: {int((~valid).sum())} of {F} faces hold an index outside [0, {V})")
    col = None if colors is None else np.ascontiguousarray(np.asarray(colors, np.float32)).reshape(V, 3)
    labels = connected_components_numpy(V, f).astype(np.int64)
    face_label = labels[f[:, 0]]
    count = np.bincount(face_label, minlength=V)
    roots = np.flatnonzero(count >= 1)                       # ascending label
    order = roots[np.lexsort((roots, -count[roots]))]        # face count descending, label ascending
    if keep_largest is not None:
        order = order[:keep_largest]
    kept = order[count[order] >= max(min_faces, 1)]
    keep_root = np.zeros(V, bool)
    keep_root[kept] = True
    vkeep = keep_root[labels]
    fkeep = keep_root[face_label]
    info = dict(num_clusters=int(roots.size), kept_clusters=int(kept.size), verts_in=V, faces_in=F,
                verts_out=int(vkeep.sum()), faces_out=int(fkeep.sum()))
    return compact_numpy(v, f, col, vkeep, fkeep) + (info,)


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "clean_mesh_numpy / connected_components_numpy"


def _workspace(dev, V, F):
    """(scratch bytes, counts [5] i32)"""
    return workspace("clean", dev, (V, F), _cabi.lib().mgs_mesh_clean_scratch_bytes,
                     f"mesh clean-up: {V} vertices / {F} faces: 3 V and 3 F must stay below 2^31", _cabi.MESH_CLEAN_COUNTS)


def _args(V, faces, scratch):
    a = _cabi.MeshCleanArgs()
    a.num_verts, a.num_faces, a.keep_largest, a.min_faces = V, int(faces.shape[0]), -1, 0
    a.faces = faces.data_ptr() if faces.shape[0] else None
    a.scratch = scratch.data_ptr()
    return a


def connected_components(num_verts: int, faces) -> torch.Tensor:
    """labels [V] i32 on the device of `faces` [F,3]: the smallest vertex index of each vertex's component.  Three
    launches, no host read; indices outside [0,V) connect nothing."""
    faces = device_rows(faces, "connected_components", "faces", _MIRRORS, torch.int32)
    V, dev = int(num_verts), faces.device
    if V < 0:
        raise ValueError("connected_components: num_verts must be >= 0")
    scratch, _ = _workspace(dev, V, int(faces.shape[0]))
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    a = _args(V, faces, scratch)
    a.labels = labels.data_ptr() if V else None
    _cabi.check(_cabi.lib().mgs_mesh_components(C.byref(a), stream_ptr(dev)), "mgs_mesh_components")
    return labels


def clean_mesh(verts, faces, colors=None, keep_largest: Optional[int] = None, min_faces: int = 0):
    """(verts [V',3] f32, faces [F',3] i32, colors [V',3] f32 | None, info) on the device: the clusters of the mesh kept
    by size (module docstring), everything else dropped and the rest compacted in order.  One host read, of the counts
    record, between the scan and the emission; a face with an index outside [0,V) raises ValueError after it."""
    keep_largest, min_faces = _check_params(keep_largest, min_faces)
    faces = device_rows(faces, "clean_mesh", "faces", _MIRRORS, torch.int32)
    dev = faces.device
    if not torch.is_tensor(verts) or verts.device != dev or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("clean_mesh: verts must be [V,3] on the device of faces")
    verts = verts.detach().to(torch.float32).contiguous()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    colors = device_colors(colors, "clean_mesh", V, dev)
    L = _cabi.lib()
    scratch, counts = _workspace(dev, V, F)
    a = _args(V, faces, scratch)
    a.keep_largest = -1 if keep_largest is None else min(keep_largest, 2 ** 31 - 1)
    a.min_faces = min(min_faces, 2 ** 31 - 1)
    a.counts = counts.data_ptr()
    _cabi.check(L.mgs_mesh_clean_count(C.byref(a), stream_ptr(dev)), "mgs_mesh_clean_count")
    V2, F2, clusters, kept, bad = (int(c) for c in counts.cpu())
    if bad:
        raise ValueError(f"clean_mesh: {bad} of {F} faces hold an index outside [0, {V})")
    out_v, out_f, out_c = emit_compacted(a, L.mgs_mesh_clean_emit, "mgs_mesh_clean_emit", verts, colors, V2, F2)
    info = dict(num_clusters=clusters, kept_clusters=kept, verts_in=V, faces_in=F, verts_out=V2, faces_out=F2)
    return out_v, out_f, out_c, info
