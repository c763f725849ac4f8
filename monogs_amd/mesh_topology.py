"""The unique undirected edges of an indexed triangle mesh and what they say about it: closed, manifold, consistently
wound (csrc/mesh_edges.hip; the contract is in include/monogs_raster.h and DESIGN.md "Mesh edges and smoothing").

    verts, faces, colors = vol.extract_mesh()
    info = mesh_topology(faces, verts.shape[0], components=True)       # info["closed"], info["euler"], ...
    edges, edge_faces, vertex_degree, vertex_flags, info = mesh_edges(faces, verts.shape[0])

The mirror `mesh_edges_numpy` IS the contract:

  * half-edge 3 f + k runs from faces[f,k] to faces[f,(k+1)%3]; its key is (lo << 32) | hi of the two indices;
  * a face with an index outside [0,V) is bad: ValueError.  A face with two equal indices is degenerate: it is counted
    and contributes no edge;
  * the representative of an edge is the smallest half-edge index with its key; edges [E,2] holds (lo, hi) in ascending
    representative order, edge_faces [E] the number of half-edges with the key;
  * vertex_degree [V] is the number of unique edges at the vertex; vertex_flags bit 0: referenced (degree > 0), bit 1:
    the vertex lies on an edge whose count is not 2;
  * info (INFO_KEYS): boundary_edges (count 1), manifold_edges (count 2), nonmanifold_edges (count >= 3),
    inconsistent_edges (count 2 with both half-edges in one direction), euler = referenced_verts - edges + (faces_in -
    degenerate_faces), closed = no boundary and no non-manifold edge, oriented = closed and no inconsistent edge.

Everything is an integer and nothing depends on an execution order, so the device's output equals the mirror's bit for
bit.  There is no CPU fall-back behind mesh_edges / mesh_topology: off the GPU they raise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _cabi
from ._device import device_rows, stream_ptr, workspace
from .mesh_simplify import _mix64, table_size

INFO_KEYS = ("verts_in", "faces_in", "edges", "boundary_edges", "manifold_edges", "nonmanifold_edges",
             "inconsistent_edges", "degenerate_faces", "referenced_verts", "boundary_verts", "euler", "closed", "oriented")
FLAG_REFERENCED, FLAG_BOUNDARY = 1, 2


def _bad_faces_message(what, bad, F, V):
    return f"{what}: {bad} of {F} faces hold an index outside [0, {V})"


def edge_key(a, b):
    """The 64-bit key of the undirected edge {a, b}: (lo << 32) | hi."""
    lo, hi = (int(a), int(b)) if int(a) < int(b) else (int(b), int(a))
    return (lo << 32) | hi


def _home_slot_edges(a, b, table_size):
    """The slot at which the device starts to probe for the edge {a, b} in a table of `table_size` entries (home_of_key
    in csrc/mesh_edges.hip; the table of F faces has mesh_simplify.table_size(3 F) entries).  For the tests, which must
    reach probing and wrap-around on purpose; it has to be kept in step with the kernel BY HAND.  The output of
    mesh_edges never depends on it."""
    return (_mix64(edge_key(a, b)) & 0xFFFFFFFF) & (int(table_size) - 1)


def _info(V, F, edges, boundary, manifold, nonmanifold, inconsistent, degenerate, referenced, boundary_verts):
    closed = boundary == 0 and nonmanifold == 0
    return dict(verts_in=V, faces_in=F, edges=edges, boundary_edges=boundary, manifold_edges=manifold,
                nonmanifold_edges=nonmanifold, inconsistent_edges=inconsistent, degenerate_faces=degenerate,
                referenced_verts=referenced, boundary_verts=boundary_verts, euler=referenced - edges + (F - degenerate),
                closed=closed, oriented=closed and inconsistent == 0)


def _check_num_verts(what, num_verts):
    V = int(num_verts)
    if V < 0:
        raise ValueError(f"{what}: num_verts must be >= 0")
    return V


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def mesh_edges_numpy(faces, num_verts, _what="mesh_edges"):
    """(edges [E,2] i32, edge_faces [E] i32, vertex_degree [V] i32, vertex_flags [V] i32, info) in plain NumPy: the
    contract of mesh_edges."""
    V = _check_num_verts(_what, num_verts)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    F = f.shape[0]
    valid = ((f >= 0) & (f < V)).all(axis=1)
    if not valid.all():
        raise ValueError(_bad_faces_message(_what, int((~valid).sum()), F, V))
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    u, v = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                  # half-edge 3 f + k: u -> v
    h = np.flatnonzero(np.repeat(~degenerate, 3))                      # ascending half-edge index
    u, v = u[h], v[h]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    _, first, inv, count = np.unique((lo << 32) | hi, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    forward = np.bincount(inv, weights=(u < v), minlength=first.shape[0]).astype(np.int64)
    order = np.argsort(h[first], kind="stable")                        # ascending representative
    first, count, forward = first[order], count[order], forward[order]
    edges = np.stack([lo[first], hi[first]], 1).astype(np.int32).reshape(-1, 2)
    degree = np.bincount(edges.reshape(-1), minlength=V).astype(np.int32)
    flags = (degree > 0).astype(np.int32)
    flags[edges[count != 2].reshape(-1)] |= FLAG_BOUNDARY
    info = _info(V, F, int(edges.shape[0]), int((count == 1).sum()), int((count == 2).sum()), int((count >= 3).sum()),
                 int(((count == 2) & (forward != 1)).sum()), int(degenerate.sum()), int((degree > 0).sum()),
                 int((flags & FLAG_BOUNDARY != 0).sum()))
    return edges, count.astype(np.int32), degree, flags, info


def mesh_topology_numpy(faces, num_verts, components=False):
    """info of mesh_edges_numpy; with `components` also the number of connected components among the referenced
    vertices (mesh_clean.connected_components_numpy): the contract of mesh_topology."""
    _, _, degree, _, info = mesh_edges_numpy(faces, num_verts, "mesh_topology")
    if components:
        from .mesh_clean import connected_components_numpy
        labels = connected_components_numpy(int(num_verts), faces)
        info["components"] = int(np.unique(labels[degree > 0]).shape[0])
    return info


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "mesh_edges_numpy / mesh_topology_numpy"


def info_of_record(V, F, rec):
    """info from the integers of the device's record (MGS_MESH_EDGES_RECORD_INTS)."""
    return _info(V, F, rec[0], rec[4], rec[5], rec[6], rec[7], rec[8], rec[2], rec[3])


def too_large_message(what, V, F):
    return f"{what}: {V} vertices / {F} faces: 3 V must stay below 2^31 and 3 F at or below 2^30"


def _count(what, faces, num_verts):
    """Runs mgs_mesh_edges_count and reads the record: (args, record list, vertex_degree, vertex_flags, faces)."""
    V = _check_num_verts(what, num_verts)
    faces = device_rows(faces, what, "faces", _MIRRORS, torch.int32)
    dev, F = faces.device, int(faces.shape[0])
    L = _cabi.lib()
    scratch, record = workspace("edges", dev, (V, F), L.mgs_mesh_edges_scratch_bytes, too_large_message(what, V, F),
                                _cabi.MESH_EDGES_RECORD_INTS)
    degree = torch.empty(V, dtype=torch.int32, device=dev)
    flags = torch.empty(V, dtype=torch.int32, device=dev)
    a = _cabi.MeshEdgesArgs()
    a.num_verts, a.num_faces = V, F
    a.faces = faces.data_ptr() if F else None
    a.scratch, a.record = scratch.data_ptr(), record.data_ptr()
    a.vertex_degree = degree.data_ptr() if V else None
    a.vertex_flags = flags.data_ptr() if V else None
    _cabi.check(L.mgs_mesh_edges_count(C.byref(a), stream_ptr(dev)), "mgs_mesh_edges_count")
    rec = [int(x) for x in record.cpu()]
    if rec[9]:
        raise ValueError(_bad_faces_message(what, rec[9], F, V))
    return a, rec, degree, flags, faces


def mesh_edges(faces, num_verts):
    """(edges [E,2] i32, edge_faces [E] i32, vertex_degree [V] i32, vertex_flags [V] i32, info) on the device of
    `faces` [F,3] (module docstring).  One host read, of the record, between the scan and the emission; a face with an
    index outside [0,V) raises ValueError after it."""
    a, rec, degree, flags, faces = _count("mesh_edges", faces, num_verts)
    dev, E = faces.device, rec[0]
    edges = torch.empty(E, 2, dtype=torch.int32, device=dev)
    edge_faces = torch.empty(E, dtype=torch.int32, device=dev)
    a.out_num_edges = E
    if E:
        a.edges, a.edge_faces = edges.data_ptr(), edge_faces.data_ptr()
    _cabi.check(_cabi.lib().mgs_mesh_edges_emit(C.byref(a), stream_ptr(dev)), "mgs_mesh_edges_emit")
    return edges, edge_faces, degree, flags, info_of_record(a.num_verts, a.num_faces, rec)


def mesh_topology(faces, num_verts, components=False):
    """info (INFO_KEYS) of the mesh on the device of `faces`: the count launches of mesh_edges and one host read, no
    emission.  With `components` also "components", the number of distinct mesh_clean.connected_components labels among
    the referenced vertices (one more host read)."""
    a, rec, degree, _, faces = _count("mesh_topology", faces, num_verts)
    info = info_of_record(a.num_verts, a.num_faces, rec)
    if components:
        from .mesh_clean import connected_components
        labels = connected_components(a.num_verts, faces)
        named = torch.zeros(a.num_verts, dtype=torch.int32, device=faces.device)     # referenced vertices per label
        named.index_add_(0, labels.long(), (degree > 0).to(torch.int32))
        info["components"] = int((named > 0).sum())
    return info
