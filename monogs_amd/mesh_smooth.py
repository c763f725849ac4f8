"""Laplacian and Taubin smoothing of an indexed triangle mesh on the device (csrc/mesh_edges.hip; the contract is in
include/monogs_raster.h and DESIGN.md "Mesh edges and smoothing").

    verts, faces, colors = vol.extract_mesh()
    verts, info = smooth_mesh(verts, faces)                            # 10 iterations of Taubin's lambda | mu

mu=None is plain Laplacian smoothing - one step of weight lam per iteration, which shrinks the mesh; otherwise every
iteration is a lam step and then a mu step (Taubin), which does not.  The weights are uniform over the neighbours along
the UNIQUE edges of the mesh (mesh_topology.mesh_edges), as in Open3D's filter_smooth_laplacian / filter_smooth_taubin.

The mirror `smooth_mesh_numpy` IS the contract.  One step with weight w (fp32, widened to fp64), Jacobi style, reading the
previous positions only:

  * E is the unbiased exponent field (bits >> 23) - 127 of the largest |coordinate| among the INPUT vertices - an integer
    maximum over the float bits, taken once per call; K = 28;
  * a vertex with degree 0 keeps its bits, and with boundary="pin" so does a vertex on an edge whose face count is not 2
    (flag bit 1); boundary="free" moves those too;
  * every other vertex, per axis: S = sum over its d neighbours of q(p_u) as int64 with q(p) = int64(fmax(fmin(ldexp(
    double(p), K - E), 2^62), -2^62)) - the scaling is exact, the conversion truncates -, m = ldexp(double(S) / double(d),
    E - K), p' = float(double(p) + w (m - double(p))), every fp64 operation one rounding.  The clamp and the int64
    wrap-around only say what mirror and device agree on where no sane call comes;
  * a vertex with a non-finite coordinate is bad: ValueError; so is a face with an index outside [0,V).

The sums are integers, so the device's output equals the mirror's bit for bit whatever order the neighbours arrive in.
`faces` and colours are untouched.  There is no CPU fall-back behind smooth_mesh: off the GPU it raises."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _cabi
from ._device import device_rows, stream_ptr, workspace
from .mesh_topology import (FLAG_BOUNDARY, INFO_KEYS as TOPOLOGY_KEYS, _bad_faces_message, info_of_record,
                            mesh_edges_numpy, too_large_message)

INFO_KEYS = TOPOLOGY_KEYS + ("iterations", "steps", "pinned_verts")
FIXED_BITS = 28               # K: the largest |coordinate| scales into [2^28, 2^29)
MAX_ITERATIONS = _cabi.MESH_SMOOTH_MAX_ITERATIONS


def _check_params(iterations, lam, mu, boundary):
    """(iterations, lam fp32, mu fp32 | None, pin): the refusals before any launch."""
    if isinstance(iterations, bool) or int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"smooth_mesh: iterations must be an integer in [0, {MAX_ITERATIONS}], got {iterations!r}")
    lam32 = np.float32(lam)
    if not (math.isfinite(float(lam32)) and 0.0 < float(lam32) <= 1.0):
        raise ValueError(f"smooth_mesh: lam must lie in (0, 1], got {lam!r}")
    mu32 = None
    if mu is not None:
        mu32 = np.float32(mu)
        if not (math.isfinite(float(mu32)) and -1.0 <= float(mu32) < 0.0):
            raise ValueError(f"smooth_mesh: mu must lie in [-1, 0) or be None, got {mu!r}")
    if boundary not in ("pin", "free"):
        raise ValueError(f"smooth_mesh: boundary must be 'pin' or 'free', got {boundary!r}")
    return int(iterations), lam32, mu32, boundary == "pin"


def _bad_verts_message(bad, V):
    return f"smooth_mesh: {bad} of {V} vertices are not finite"


def _info(topology, iterations, taubin, pin):
    return dict(topology, iterations=iterations, steps=iterations * (2 if taubin else 1),
                pinned_verts=topology["boundary_verts"] if pin else 0)


# ---- mirror ----------------------------------------------------------------------------------------------------------
def smooth_mesh_numpy(verts, faces, iterations=10, lam=0.5, mu=-0.53, boundary="pin"):
    """(verts' [V,3] f32, info) in plain NumPy: the contract of smooth_mesh."""
    iterations, lam32, mu32, pin = _check_params(iterations, lam, mu, boundary)
    p = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3).copy()
    V = p.shape[0]
    finite = np.isfinite(p).all(axis=1)
    edges, _, degree, flags, topology = mesh_edges_numpy(faces, V, "smooth_mesh")
    if not finite.all():
        raise ValueError(_bad_verts_message(int((~finite).sum()), V))
    info = _info(topology, iterations, mu32 is not None, pin)
    moves = degree > 0
    if pin:
        moves &= (flags & FLAG_BOUNDARY) == 0
    rows = np.flatnonzero(moves)
    if iterations == 0 or rows.size == 0:
        return p, info
    maxbits = int((p.view(np.uint32) & np.uint32(0x7FFFFFFF)).max())
    E = (maxbits >> 23) - 127
    # the rows of the neighbours, CSR: vertex at[k] has the neighbour other[k]
    at = np.concatenate([edges[:, 0], edges[:, 1]]).astype(np.int64)
    other = np.concatenate([edges[:, 1], edges[:, 0]]).astype(np.int64)[np.argsort(at, kind="stable")]
    starts = np.concatenate([[0], np.cumsum(degree.astype(np.int64))])[:-1]
    d = degree[rows].astype(np.float64)[:, None]
    two62 = np.float64(2.0 ** 62)
    weights = [np.float64(lam32)] if mu32 is None else [np.float64(lam32), np.float64(mu32)]
    for _ in range(iterations):
        for w in weights:
            with np.errstate(all="ignore"):
                q = np.fmax(np.fmin(np.ldexp(p.astype(np.float64), FIXED_BITS - E), two62), -two62).astype(np.int64)
                # reduceat over the rows with neighbours only: the starts of empty rows would repeat their successor's
                S = np.add.reduceat(q[other], starts[degree > 0], axis=0)
                S = S[np.searchsorted(np.flatnonzero(degree > 0), rows)]
                m = np.ldexp(S.astype(np.float64) / d, E - FIXED_BITS)
                P = p[rows].astype(np.float64)
                new = (P + w * (m - P)).astype(np.float32)
            p = p.copy()
            p[rows] = new
    return p, info


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "smooth_mesh_numpy"


def smooth_mesh(verts, faces, iterations=10, lam=0.5, mu=-0.53, boundary="pin"):
    """(verts' [V,3] f32, info) on the device: `iterations` of Taubin's lam | mu steps (mu=None: of Laplacian lam steps)
    over the unique-edge neighbours, boundary vertices pinned or free (module docstring).  The edge set, a CSR vertex
    adjacency and one gather launch per step; one host read, of the record, after the last step.  A non-finite vertex or
    a face with an index outside [0,V) raises ValueError after it."""
    iterations, lam32, mu32, pin = _check_params(iterations, lam, mu, boundary)
    faces = device_rows(faces, "smooth_mesh", "faces", _MIRRORS, torch.int32)
    dev = faces.device
    if not torch.is_tensor(verts) or verts.device != dev or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("smooth_mesh: verts must be [V,3] on the device of faces")
    verts = verts.detach().to(torch.float32).contiguous()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    L = _cabi.lib()
    scratch, record = workspace("smooth", dev, (V, F), L.mgs_mesh_smooth_scratch_bytes,
                                too_large_message("smooth_mesh", V, F), _cabi.MESH_EDGES_RECORD_INTS)
    out = torch.empty(V, 3, device=dev)
    a = _cabi.MeshSmoothArgs()
    a.num_verts, a.num_faces, a.iterations = V, F, iterations
    a.taubin, a.boundary_free = (0 if mu32 is None else 1), (0 if pin else 1)
    a.lam, a.mu = float(lam32), (0.0 if mu32 is None else float(mu32))
    a.verts = verts.data_ptr() if V else None
    a.faces = faces.data_ptr() if F else None
    a.scratch, a.record = scratch.data_ptr(), record.data_ptr()
    a.out_verts = out.data_ptr() if V else None
    _cabi.check(L.mgs_mesh_smooth(C.byref(a), stream_ptr(dev)), "mgs_mesh_smooth")
    rec = [int(x) for x in record.cpu()]
    if rec[9]:
        raise ValueError(_bad_faces_message("smooth_mesh", rec[9], F, V))
    if rec[10]:
        raise ValueError(_bad_verts_message(rec[10], V))
    return out, _info(info_of_record(V, F, rec), iterations, mu32 is not None, pin)
