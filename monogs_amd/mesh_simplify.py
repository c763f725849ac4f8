"""Mesh simplification by vertex clustering on the device (csrc/mesh_simplify.hip; the contract is in
include/monogs_raster.h and DESIGN.md "Mesh simplification").

    verts, faces, colors = vol.extract_mesh()
    verts, faces, colors, info = simplify_mesh(verts, faces, colors, cell=2 * vol.voxel_size, origin=vol.origin)

The mirror `simplify_mesh_numpy` IS the contract:

  * origin: the one given, or the per-axis minimum over the vertices whose three coordinates are finite;
  * per axis, in single fp32 roundings, t = (v - o) / cell, c = floor(t), fr = t - c; c must lie in [-2^20, 2^20).  A
    vertex with a non-finite coordinate or a cell out of range is bad: ValueError;
  * a cluster is the set of vertices of one cell, its label its smallest vertex index;
  * its position, per axis: S = sum of trunc(fr 2^24) as int64 over its n vertices, m = double(S) / (double(n) 2^24),
    float(double(o) + (double(c) + m) double(cell)); its colour the same mean of trunc(clamp(x, 0, 1) 2^24), NaN as 0;
  * every face index is mapped to its label; a face with two equal labels is collapsed and dropped; of the faces with one
    set of three labels (any order, either winding) the one with the smallest face index stays; kept faces keep their
    relative order and winding.  A face with an index outside [0,V) is bad: ValueError;
  * a cluster is emitted iff a kept face names it, in ascending label order; the faces are re-indexed.

Clustering can flip a triangle (evaluate_mesh(normals=True) reports normal_flipped), a closed input need not stay closed,
and simplifying twice is not the identity on the bits.  Nothing depends on an execution order, so the device's output
equals the mirror's bit for bit.  There is no CPU fall-back behind simplify_mesh: off the GPU it raises."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _cabi
from ._device import device_colors, device_rows, emit_compacted, stream_ptr, workspace

INFO_KEYS = ("verts_in", "faces_in", "verts_out", "faces_out", "num_clusters", "collapsed_faces", "duplicate_faces")
CELL_LIMIT = 1 << 20          # cells lie in [-2^20, 2^20)
FIXED_ONE = 1 << 24           # the fixed point of fractions and colours
_M64 = (1 << 64) - 1


def _check_cell(cell):
    c = np.float32(cell)
    if not (math.isfinite(float(c)) and float(c) > 0.0):
        raise ValueError(f"simplify_mesh: cell must be a finite fp32 value > 0, got {cell!r}")
    return c


def _check_origin(origin):
    if origin is None:
        return None
    o = np.asarray([float(x) for x in (origin.tolist() if hasattr(origin, "tolist") else origin)], np.float32)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"simplify_mesh: origin must be three finite values, got {origin!r}")
    return o


def _bad_verts_message(bad, V):
    return f"simplify_mesh: {bad} of {V} vertices are not finite or lie outside the 2^21 cells per axis"


def _bad_faces_message(bad, F, V):
    return f"simplify_mesh: {bad} of {F} faces hold an index outside [0, {V})"


# ---- the two hash functions of csrc/mesh_simplify.hip, restated -----------------------------------------------------------
def _mix64(k):
    k &= _M64
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & _M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & _M64
    k ^= k >> 33
    return k


def table_size(n):
    """Entries of the device's hash table for n items: the smallest power of two >= 2 n (set_table_size)."""
    s = 1
    while s < 2 * int(n):
        s <<= 1
    return s


def cell_key(cx, cy, cz):
    """The 63-bit key of the cell (cx, cy, cz), each in [-2^20, 2^20)."""
    return ((int(cx) + CELL_LIMIT) << 42) | ((int(cy) + CELL_LIMIT) << 21) | (int(cz) + CELL_LIMIT)


def _home_slot(key, table_size):
    """The slot at which the device starts to probe for the vertex cell `key` in a table of `table_size` entries
    (home_of_key in csrc/mesh_simplify.hip).  For the tests, which must reach probing and wrap-around on purpose; it has
    to be kept in step with the kernel BY HAND.  The output of simplify_mesh never depends on it."""
    return (_mix64(int(key)) & 0xFFFFFFFF) & (int(table_size) - 1)


def _home_slot_faces(triple, table_size):
    """The same for a face's label triple, in any order (home_of_triple); to be kept in step with the kernel by hand."""
    a, b, c = sorted(int(x) for x in triple)
    return (_mix64(_mix64((a << 32) | b) ^ c) & 0xFFFFFFFF) & (int(table_size) - 1)


# ---- mirror ----------------------------------------------------------------------------------------------------------
def _order_key(x):
    b = x.view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _min_origin(v):
    """Per-axis minimum over the vertices with three finite coordinates, by the order keys of the floats (-0 < +0); NaN
    when there is none."""
    fin = np.isfinite(v).all(axis=1)
    if not fin.any():
        return np.full(3, np.nan, np.float32)
    k = _order_key(v[fin]).min(axis=0).astype(np.uint32)
    return np.where(k >> 31, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def _group_sums(inv, num, q):
    """int64 sums of the rows of q [V,3] per group inv [V] in [0, num), every group non-empty."""
    order = np.argsort(inv, kind="stable")
    starts = np.searchsorted(inv[order], np.arange(num))
    return np.add.reduceat(q[order], starts, axis=0)


def simplify_mesh_numpy(verts, faces, colors=None, *, cell, origin=None):
    """(verts, faces, colors | None, info) in plain NumPy: the contract of simplify_mesh."""
    cell = _check_cell(cell)
    o = _check_origin(origin)
    v = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3)
    V = v.shape[0]
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    F = f.shape[0]
    col = None if colors is None else np.ascontiguousarray(np.asarray(colors, np.float32)).reshape(V, 3)
    if o is None:
        o = _min_origin(v)
    with np.errstate(all="ignore"):
        t = ((v - o[None, :]).astype(np.float32) / cell).astype(np.float32)
        c = np.floor(t)
        fr = (t - c).astype(np.float32)
        good = np.isfinite(v).all(axis=1) & ((c >= -CELL_LIMIT) & (c < CELL_LIMIT)).all(axis=1)
    if not good.all():
        raise ValueError(_bad_verts_message(int((~good).sum()), V))
    valid = ((f >= 0) & (f < V)).all(axis=1) if F else np.zeros(0, bool)
    if not valid.all():
        raise ValueError(_bad_faces_message(int((~valid).sum()), F, V))
    ci = c.astype(np.int64) + CELL_LIMIT
    key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)       # first: the smallest index of each key
    inv = inv.reshape(-1)
    num = first.shape[0]
    label = first[inv] if V else np.zeros(0, np.int64)

    lab = label[f] if F else np.zeros((0, 3), np.int64)
    collapsed = (lab[:, 0] == lab[:, 1]) | (lab[:, 1] == lab[:, 2]) | (lab[:, 0] == lab[:, 2])
    cand = np.flatnonzero(~collapsed)                                            # ascending face index
    s = np.sort(lab[cand], axis=1)
    order = np.lexsort((s[:, 2], s[:, 1], s[:, 0]))                              # stable: equal triples by face index
    ss = s[order]
    head = np.ones(order.shape[0], bool)
    head[1:] = (ss[1:] != ss[:-1]).any(axis=1)
    fkeep = np.zeros(F, bool)
    fkeep[cand[order[head]]] = True
    vkeep = np.zeros(V, bool)
    vkeep[lab[fkeep].reshape(-1)] = True                                         # labels only

    out_v = np.zeros((0, 3), np.float32)
    out_c = None if col is None else np.zeros((0, 3), np.float32)
    if vkeep.any():
        n = np.bincount(inv, minlength=num).astype(np.float64) * float(FIXED_ONE)
        S = _group_sums(inv, num, (fr * np.float32(FIXED_ONE)).astype(np.int64))
        m = S.astype(np.float64) / n[:, None]
        pos = (o.astype(np.float64)[None, :] + (c[first].astype(np.float64) + m) * np.float64(cell)).astype(np.float32)
        emitted = vkeep[first]                                                   # `first` ascends with the key, not the label:
        rank = np.argsort(first[emitted], kind="stable")                         # ascending label order
        out_v = pos[emitted][rank]
        if col is not None:
            x = np.fmin(np.fmax(col, np.float32(0)), np.float32(1))              # fmax / fmin drop a NaN: NaN -> 0
            Sc = _group_sums(inv, num, (x * np.float32(FIXED_ONE)).astype(np.int64))
            out_c = (Sc.astype(np.float64) / n[:, None]).astype(np.float32)[emitted][rank]
    new_index = np.cumsum(vkeep) - 1
    out_f = new_index[lab[fkeep]].astype(np.int32).reshape(-1, 3)
    info = dict(verts_in=V, faces_in=F, verts_out=int(vkeep.sum()), faces_out=int(fkeep.sum()), num_clusters=int(num),
                collapsed_faces=int(collapsed.sum()), duplicate_faces=int(F - collapsed.sum() - fkeep.sum()))
    return out_v, out_f, out_c, info


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "simplify_mesh_numpy"


def simplify_mesh(verts, faces, colors=None, *, cell, origin=None):
    """(verts [V',3] f32, faces [F',3] i32, colors [V',3] f32 | None, info) on the device: the vertices of every cell of
    edge `cell` (from `origin`, or from the per-axis minimum of the vertices) merged into their mean, collapsed and
    duplicate faces dropped (module docstring).  One host read, of the counts record, between the scan and the
    emission; a bad vertex or a face with an index outside [0,V) raises ValueError after it."""
    cell = _check_cell(cell)
    o = _check_origin(origin)
    faces = device_rows(faces, "simplify_mesh", "faces", _MIRRORS, torch.int32)
    dev = faces.device
    if not torch.is_tensor(verts) or verts.device != dev or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("simplify_mesh: verts must be [V,3] on the device of faces")
    verts = verts.detach().to(torch.float32).contiguous()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    colors = device_colors(colors, "simplify_mesh", V, dev)
    L = _cabi.lib()
    scratch, counts = workspace("simplify", dev, (V, F), L.mgs_mesh_simplify_scratch_bytes,
                                f"mesh simplification: {V} vertices / {F} faces: 3 V and 3 F must stay below 2^31",
                                _cabi.MESH_SIMPLIFY_COUNTS)
    a = _cabi.MeshSimplifyArgs()
    a.num_verts, a.num_faces, a.cell = V, F, float(cell)
    a.origin_from_verts = 1 if o is None else 0
    if o is not None:
        a.origin[0], a.origin[1], a.origin[2] = (float(x) for x in o)
    a.verts = verts.data_ptr() if V else None
    a.faces = faces.data_ptr() if F else None
    a.colors = colors.data_ptr() if colors is not None and V else None
    a.scratch, a.counts = scratch.data_ptr(), counts.data_ptr()
    _cabi.check(L.mgs_mesh_simplify_count(C.byref(a), stream_ptr(dev)), "mgs_mesh_simplify_count")
    V2, F2, clusters, collapsed, duplicates, bad_verts, bad_faces, _ = (int(c) for c in counts.cpu())
    if bad_verts:
        raise ValueError(_bad_verts_message(bad_verts, V))
    if bad_faces:
        raise ValueError(_bad_faces_message(bad_faces, F, V))
    out_v, out_f, out_c = emit_compacted(a, L.mgs_mesh_simplify_emit, "mgs_mesh_simplify_emit", verts, colors, V2, F2)
    info = dict(verts_in=V, faces_in=F, verts_out=V2, faces_out=F2, num_clusters=clusters, collapsed_faces=collapsed,
                duplicate_faces=duplicates)
    return out_v, out_f, out_c, info


def simplify_keywords(simplify, voxel_size, origin):
    """The simplify_mesh keywords of a volume's `simplify` dict: factor=k stands for cell = k voxel_size, and the
    volume's origin is used when none is given."""
    kw = dict(simplify)
    if "factor" in kw:
        if "cell" in kw:
            raise ValueError("simplify: give cell or factor, not both")
        kw["cell"] = float(np.float32(kw.pop("factor")) * np.float32(voxel_size))
    if "cell" not in kw:
        raise ValueError("simplify: needs cell or factor")
    if kw.get("origin") is None:
        kw["origin"] = tuple(float(x) for x in origin)
    return kw
