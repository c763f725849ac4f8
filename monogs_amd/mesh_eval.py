"""Mesh evaluation: points sampled on two surfaces, nearest distances in both directions, and the geometry numbers every
dense-SLAM paper reports - on the device (csrc/mesh_eval.hip; the contract is in include/monogs_raster.h and DESIGN.md
"Mesh evaluation").

    points, face_index = sample_surface(verts, faces, 200_000, seed=0)             # no host read
    d2, index = nearest_distance(query, ref)                                       # no host read
    scores = evaluate_mesh((verts, faces), (gt_verts, gt_faces), threshold=0.05)   # ONE host read, of the record

The mirrors ARE the contract:

  * `philox4x32_10` - the generator of keyframe_seed.hip, pinned to the Random123 known answers;
  * `sample_surface_numpy` - integer face weights q = trunc(A 2^(30 - E)) from the fp32 area A and the exponent E of the
    largest, an exact uint64 CDF, t = 64 random bits mod T, the smallest face with C[f] > t, a folded 24-bit barycentric
    pair; the device gives the same bits;
  * `nearest_distance_torch` - chunked brute force in eager fp32 torch, one rounding per operation, the pair (d2, index)
    compared lexicographically; runs on CPU or GPU tensors; the device's grid search gives the same bits;
  * `distance_stats_numpy`, `evaluate_mesh_numpy` - counts and maxima equal exactly, the fp64 sums to the order of adding;
  * `normal_stats_numpy` - with normals=True, n . m of the face normals (mesh_normals.py) of every sample and its nearest
    neighbour in single fp32 roundings; pairs, flipped and skipped pairs exactly, the fp64 sum of |n . m| likewise.

There is no CPU fall-back behind sample_surface / nearest_distance / evaluate_mesh: off the GPU they raise."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _cabi
from ._device import device_rows, ptr as _ptr, stream_ptr, workspace

METRIC_KEYS = ("accuracy", "completion", "chamfer", "precision", "recall", "completion_ratio", "f_score", "hausdorff",
               "n_pred", "n_gt", "bad_faces")
NORMAL_KEYS = ("normal_accuracy", "normal_completion", "normal_consistency", "normal_flipped", "normal_skipped")
SAMPLE_STREAM = 2          # Philox counter (j, 0, SAMPLE_STREAM, 0); keyframe seeding uses streams 0 and 1


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key) -> np.ndarray:
    """Philox-4x32-10 (Salmon et al., SC'11) of counters [..., 4] u32 under key (k0, k1): [..., 4] u32."""
    c = np.asarray(counter, np.uint64) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sample_words_numpy(n: int, seed: int = 0) -> np.ndarray:
    """[n,4] u32: the words the device draws for samples 0..n-1 under `seed`."""
    ctr = np.zeros((int(n), 4), np.uint64)
    ctr[:, 0] = np.arange(int(n), dtype=np.uint64)
    ctr[:, 2] = SAMPLE_STREAM
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def face_weights_numpy(verts, faces):
    """(q [F] u64, bad faces): the integer weight of every face."""
    v = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V, F = v.shape[0], f.shape[0]
    valid = ((f >= 0) & (f < V)).all(axis=1) if F else np.zeros(0, bool)
    fs = np.where(valid[:, None], f, 0) if V else np.zeros_like(f)
    q = np.zeros(F, np.uint64)
    if F == 0 or V == 0:
        return q, int((~valid).sum())
    with np.errstate(all="ignore"):
        a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
        e, g = b - a, c - a
        nx = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
        ny = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
        nz = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
        A = np.sqrt((nx * nx + ny * ny) + nz * nz)
    assert A.dtype == np.float32
    A = np.where(valid & np.isfinite(A), A, np.float32(0.0))
    amax = float(A.view(np.uint32).max().view(np.float32))        # the integer maximum of the bits: A >= 0
    if amax > 0.0:
        E = int(np.frexp(amax)[1]) - 1
        q = np.trunc(np.ldexp(A.astype(np.float64), 30 - E)).astype(np.uint64)
    return q, int((~valid).sum())


def sample_surface_numpy(verts, faces, n: int, seed: int = 0, randoms=None, with_record: bool = False):
    """(points [n,3] f32, face_index [n] i32) in plain NumPy: the contract of sample_surface.  `with_record` adds the
    record [4] i32: {T == 0, bad faces, low word of T, high word of T}."""
    n = int(n)
    if n < 0:
        raise ValueError("sample_surface: n must be >= 0")
    v = np.ascontiguousarray(np.asarray(verts, np.float32)).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    q, bad = face_weights_numpy(v, f)
    cdf = np.cumsum(q, dtype=np.uint64)
    T = int(cdf[-1]) if cdf.size else 0
    record = np.array([1 if T == 0 else 0, bad, T & 0xFFFFFFFF, T >> 32], np.uint32).view(np.int32)
    if T == 0:
        out = np.full((n, 3), np.nan, np.float32), np.full(n, -1, np.int32)
        return out + (record,) if with_record else out
    if randoms is None:
        w = sample_words_numpy(n, seed)
    else:
        w = np.ascontiguousarray(np.asarray(randoms)).reshape(n, 4).astype(np.int64).astype(np.uint32)
    w64 = w.astype(np.uint64)
    t = (w64[:, 0] | (w64[:, 1] << np.uint64(32))) % np.uint64(T)
    face = np.searchsorted(cdf, t, side="right")                  # the smallest f with C[f] > t
    k1, k2 = (w[:, 2] >> 8).astype(np.int64), (w[:, 3] >> 8).astype(np.int64)
    fold = k1 + k2 > (1 << 24)
    k1, k2 = np.where(fold, (1 << 24) - k1, k1), np.where(fold, (1 << 24) - k2, k2)
    u1 = (k1.astype(np.float32) * np.float32(2.0 ** -24))[:, None]
    u2 = (k2.astype(np.float32) * np.float32(2.0 ** -24))[:, None]
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    with np.errstate(all="ignore"):
        p = (a + u1 * (b - a)) + u2 * (c - a)
    assert p.dtype == np.float32
    out = p, face.astype(np.int32)
    return out + (record,) if with_record else out


def nearest_distance_torch(query, ref, chunk_elems: int = 1 << 24):
    """(d2 [P] f32, index [P] i32 as torch tensors on the device of `query`): brute force, the contract of
    nearest_distance.  One rounding per operation; no fused multiply-add (every product and sum is its own op)."""
    q = torch.as_tensor(query).detach().to(torch.float32).reshape(-1, 3)
    r = torch.as_tensor(ref).detach().to(torch.float32).reshape(-1, 3).to(q.device)
    P, Q = q.shape[0], r.shape[0]
    inf = float("inf")
    d2 = torch.full((P,), inf, dtype=torch.float32, device=q.device)
    idx = torch.full((P,), -1, dtype=torch.int32, device=q.device)
    if P == 0 or Q == 0:
        return d2, idx
    ok_r = torch.isfinite(r).all(dim=1)
    ids = torch.arange(Q, device=q.device, dtype=torch.int64)
    big = torch.full((), 2 ** 31 - 1, dtype=torch.int64, device=q.device)
    rx, ry, rz = (r[:, i].contiguous()[None, :] for i in range(3))
    step = max(1, int(chunk_elems) // Q)
    for s in range(0, P, step):
        qc = q[s:s + step]
        dx, dy, dz = qc[:, 0:1] - rx, qc[:, 1:2] - ry, qc[:, 2:3] - rz
        d = dx * dx
        d = d + dy * dy
        d = d + dz * dz
        d = torch.where(ok_r[None, :], d, torch.full((), inf, dtype=torch.float32, device=q.device))
        m = d.min(dim=1).values
        first = torch.where((d == m[:, None]) & ok_r[None, :], ids[None, :], big).min(dim=1).values
        ok_q = torch.isfinite(qc).all(dim=1) & (first < big)
        d2[s:s + step] = torch.where(ok_q, m, torch.full_like(m, inf))
        idx[s:s + step] = torch.where(ok_q, first, torch.full_like(first, -1)).to(torch.int32)
    return d2, idx


def distance_stats_numpy(d2, threshold: float) -> dict:
    """{"n", "below", "max", "sum"} over the finite d = sqrt(d2) (fp32, correctly rounded): the record of one direction."""
    d2 = np.asarray(d2, np.float32).reshape(-1)
    d = np.sqrt(d2[np.isfinite(d2) & (d2 >= 0)])
    assert d.dtype == np.float32
    return dict(n=int(d.size), below=int((d < np.float32(threshold)).sum()), max=float(d.max()) if d.size else 0.0,
                sum=float(d.astype(np.float64).sum()))


def metrics_from_record(record, n_pred: int, n_gt: int) -> dict:
    """The dict of evaluate_mesh from the record [12] f64 (include/monogs_raster.h); raises ValueError on its flags."""
    rec = [float(x) for x in record]
    n0, b0, m0, s0, n1, b1, m1, s1 = rec[:8]
    bad = int(rec[9]) + int(rec[11])
    if bad:
        raise ValueError(f"evaluate_mesh: {bad} faces hold an index outside [0, V)")
    if rec[8] or rec[10]:
        which = " and ".join(w for w, flag in (("pred", rec[8]), ("gt", rec[10])) if flag)
        raise ValueError(f"evaluate_mesh: the {which} mesh has no face with area, nothing to sample")
    nan = float("nan")
    acc, comp = (s0 / n0 if n0 else nan), (s1 / n1 if n1 else nan)
    prec, rec_ = (b0 / n0 if n0 else 0.0), (b1 / n1 if n1 else 0.0)
    return dict(accuracy=acc, completion=comp, chamfer=0.5 * (acc + comp), precision=prec, recall=rec_,
                completion_ratio=rec_, f_score=(2.0 * prec * rec_ / (prec + rec_) if prec + rec_ > 0 else 0.0),
                hausdorff=max(m0, m1), n_pred=int(n_pred), n_gt=int(n_gt), bad_faces=0)


def normal_stats_numpy(face, d2, index, ref_face, normals, ref_normals) -> dict:
    """{"n", "sum", "flipped", "skipped"} of one direction: for sample i on face `face[i]` with the neighbour index[i] on
    face ref_face[index[i]], t = (n.x m.x + n.y m.y) + n.z m.z of the two face normals in single fp32 roundings; the
    pair is skipped when an index is out of range, d2[i] is not finite or either normal is (0,0,0).  "sum" is the fp64
    sum of |t|."""
    face, index = np.asarray(face, np.int64).reshape(-1), np.asarray(index, np.int64).reshape(-1)
    ref_face = np.asarray(ref_face, np.int64).reshape(-1)
    d2 = np.asarray(d2, np.float32).reshape(-1)
    nn, mm = np.asarray(normals, np.float32).reshape(-1, 3), np.asarray(ref_normals, np.float32).reshape(-1, 3)
    ok = np.isfinite(d2) & (face >= 0) & (face < nn.shape[0]) & (index >= 0) & (index < ref_face.shape[0])
    g = np.where(ok, ref_face[np.where(ok, index, 0)] if ref_face.size else 0, -1)
    ok &= (g >= 0) & (g < mm.shape[0])
    n, m = nn[face[ok]], mm[g[ok]]
    both = (n != 0).any(axis=1) & (m != 0).any(axis=1)
    n, m = n[both], m[both]
    t = (n[:, 0] * m[:, 0] + n[:, 1] * m[:, 1]) + n[:, 2] * m[:, 2]
    assert t.dtype == np.float32
    return dict(n=int(t.size), sum=float(np.abs(t).astype(np.float64).sum()), flipped=int((t < 0).sum()),
                skipped=int(d2.size - t.size))


def normal_metrics_from_record(record) -> dict:
    """The NORMAL_KEYS of evaluate_mesh(normals=True) from the eight doubles behind the record (include/monogs_raster.h:
    {pairs, sum |t|, pairs with t < 0, skipped pairs} per direction)."""
    n0, s0, f0, k0, n1, s1, f1, k1 = (float(x) for x in record)
    nan = float("nan")
    acc, comp = (s0 / n0 if n0 else nan), (s1 / n1 if n1 else nan)
    return dict(normal_accuracy=acc, normal_completion=comp, normal_consistency=0.5 * (acc + comp),
                normal_flipped=((f0 + f1) / (n0 + n1) if n0 + n1 else nan), normal_skipped=int(k0) + int(k1))


def _matrix34(transform):
    """(s, R, t) or a 4x4 matrix -> twelve fp32 numbers, row-major [3,4]."""
    if isinstance(transform, (tuple, list)) and len(transform) == 3:
        s, R, t = transform
        R = np.asarray(torch.as_tensor(R).detach().cpu().numpy() if torch.is_tensor(R) else R, np.float64).reshape(3, 3)
        t = np.asarray(torch.as_tensor(t).detach().cpu().numpy() if torch.is_tensor(t) else t, np.float64).reshape(3)
        M = np.concatenate([float(s) * R, t[:, None]], axis=1)
    else:
        M = np.asarray(transform.detach().cpu().numpy() if torch.is_tensor(transform) else transform, np.float64)
        if M.shape != (4, 4):
            raise ValueError("evaluate_mesh: transform must be (s, R, t) or a 4x4 matrix")
        M = M[:3]
    return M.astype(np.float32)


def apply_transform(verts: torch.Tensor, transform) -> torch.Tensor:
    """verts [V,3] under `transform`: ((m0 x + m1 y) + m2 z) + t per axis in eager fp32 torch, every step its own
    operation - the same bits on the host and on the device."""
    if transform is None:
        return verts
    M = _matrix34(transform)
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    rows = [((float(M[i, 0]) * x + float(M[i, 1]) * y) + float(M[i, 2]) * z) + float(M[i, 3]) for i in range(3)]
    return torch.stack(rows, dim=1).contiguous()


def _is_mesh(gt):
    return isinstance(gt, (tuple, list)) and len(gt) == 2


def _cull_arguments(cull, gt):
    """The keyword arguments of mesh_render.cull_pair from evaluate_mesh's `cull` dict."""
    if not isinstance(cull, dict) or "views" not in cull:
        raise ValueError("evaluate_mesh: cull must be a dict with the key 'views' (and occlusion, eps, min_views, rule)")
    if not _is_mesh(gt):
        raise ValueError("evaluate_mesh: cull needs the ground truth as a (verts, faces) mesh")
    unknown = set(cull) - {"views", "occlusion", "eps", "min_views", "rule", "empty_visible", "z_near"}
    if unknown:
        raise ValueError(f"evaluate_mesh: unknown cull keys {sorted(unknown)}")
    kw = dict(cull)
    kw.setdefault("occlusion", "gt")
    return kw


def _check_normals(normals, gt):
    if normals and not _is_mesh(gt):
        raise ValueError("evaluate_mesh: normals=True needs the ground truth as a (verts, faces) mesh")
    return bool(normals)


def evaluate_mesh_numpy(pred, gt, n_samples: int = 200_000, threshold: float = 0.05, seed: int = 0, transform=None,
                        with_record: bool = False, cull=None, normals: bool = False):
    """The mirror of evaluate_mesh on the host: the NumPy sampler, the brute-force distances (CPU torch), fp64 sums;
    `cull` through the mirrors of mesh_render, `normals` through face_normals_numpy and normal_stats_numpy."""
    normals = _check_normals(normals, gt)
    pv = apply_transform(torch.as_tensor(np.asarray(pred[0], np.float32)).reshape(-1, 3), transform).numpy()
    culled = None
    if cull is not None:
        from .mesh_render import cull_pair
        pred, gt, *culled = cull_pair(True, (pv, pred[1]), gt, **_cull_arguments(cull, gt))
        pv = pred[0]
    pp, pf, prec = sample_surface_numpy(pv, pred[1], n_samples, seed, with_record=True)
    if _is_mesh(gt):
        gp, gf, grec = sample_surface_numpy(gt[0], gt[1], n_samples, seed + 1, with_record=True)
    else:
        gp, gf, grec = np.ascontiguousarray(np.asarray(gt, np.float32)).reshape(-1, 3), None, np.zeros(4, np.int32)
    N = _cabi.MESH_EVAL_RECORD_DOUBLES
    record = np.zeros(N + (_cabi.MESH_EVAL_NORMAL_DOUBLES if normals else 0))
    if normals:
        from .mesh_normals import face_normals_numpy
        pn, gn = face_normals_numpy(pv, pred[1])[0], face_normals_numpy(gt[0], gt[1])[0]
    for d, (a, b) in enumerate(((pp, gp), (gp, pp))):
        d2, index = (t.numpy() for t in nearest_distance_torch(torch.from_numpy(a), torch.from_numpy(b)))
        st = distance_stats_numpy(d2, threshold)
        record[4 * d:4 * d + 4] = st["n"], st["below"], st["max"], st["sum"]
        if normals:
            st = normal_stats_numpy(*((pf, d2, index, gf, pn, gn) if d == 0 else (gf, d2, index, pf, gn, pn)))
            record[N + 4 * d:N + 4 * d + 4] = st["n"], st["sum"], st["flipped"], st["skipped"]
    record[8:12] = prec[0], prec[1], grec[0], grec[1]
    out = metrics_from_record(record[:N], pp.shape[0], gp.shape[0])
    if normals:
        out.update(normal_metrics_from_record(record[N:]))
    if culled is not None:
        out["culled_pred_faces"], out["culled_gt_faces"] = culled
    return (out, record) if with_record else out


# ---- the device ------------------------------------------------------------------------------------------------------
_MIRRORS = "sample_surface_numpy / nearest_distance_torch / evaluate_mesh_numpy"


def _workspace(kind, dev, size, nbytes_fn, what):
    return workspace(kind, dev, size, nbytes_fn, f"{what}: {size} items: 3 n must stay below 2^31")[0]


def _device_points(t, what, name, dev=None):
    return device_rows(t, what, name, _MIRRORS, dev=dev)


def sample_surface(verts, faces, n: int, seed: int = 0, randoms=None, with_record: bool = False):
    """(points [n,3] f32, face_index [n] i32) on the device of `verts`: n points uniform on the surface of the mesh
    (module docstring).  Five launches, no host read.  `randoms` [n,4] (u32 words held in an int32 or wider integer
    tensor) replaces the generator.  `with_record` adds the device record [4] i32 {T == 0, bad faces, T low, T high}."""
    what = "sample_surface"
    verts = _device_points(verts, what, "verts").detach().to(torch.float32).contiguous()
    dev = verts.device
    faces = _device_points(faces, what, "faces", dev).detach().to(torch.int32).contiguous()
    n = int(n)
    if n < 0 or n > _cabi.MESH_EVAL_MAX_ITEMS:
        raise ValueError(f"{what}: n must lie in [0, {_cabi.MESH_EVAL_MAX_ITEMS}], got {n}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    a = _cabi.SurfaceSampleArgs()
    a.num_verts, a.num_faces, a.num_samples = V, F, n
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.verts, a.faces = _ptr(verts), _ptr(faces)
    if randoms is not None:
        if not torch.is_tensor(randoms) or randoms.device != dev or tuple(randoms.shape) != (n, 4):
            raise ValueError(f"{what}: randoms must be [{n},4] on the device of verts")
        randoms = randoms.detach().to(torch.int64).to(torch.int32).contiguous()      # the low 32 bits
        a.randoms = _ptr(randoms)
    L = _cabi.lib()
    scratch = _workspace("sample", dev, (F,), L.mgs_surface_sample_scratch_bytes, what)
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face_index = torch.empty(n, dtype=torch.int32, device=dev)
    record = torch.empty(_cabi.SAMPLE_RECORD_INTS, dtype=torch.int32, device=dev)
    a.scratch, a.points, a.face_index, a.record = scratch.data_ptr(), _ptr(points), _ptr(face_index), record.data_ptr()
    _cabi.check(L.mgs_surface_sample(C.byref(a), stream_ptr(dev)), "mgs_surface_sample")
    return (points, face_index, record) if with_record else (points, face_index)


def nearest_distance(query, ref, cell_size=None):
    """(d2 [P] f32, index [P] i32) on the device: for every query the squared distance to, and the index of, its exact
    nearest neighbour among `ref` (module docstring; (inf, -1) without one).  Ten launches, no host read."""
    what = "nearest_distance"
    query = _device_points(query, what, "query").detach().to(torch.float32).contiguous()
    dev = query.device
    ref = _device_points(ref, what, "ref", dev).detach().to(torch.float32).contiguous()
    h = 0.0
    if cell_size is not None:
        h = float(cell_size)
        if not (h > 0.0 and math.isfinite(h)):
            raise ValueError(f"{what}: cell_size must be None or a positive number, got {cell_size}")
    P, Q = int(query.shape[0]), int(ref.shape[0])
    L = _cabi.lib()
    scratch = _workspace("nearest", dev, (Q,), L.mgs_nearest_scratch_bytes, what)
    d2 = torch.empty(P, dtype=torch.float32, device=dev)
    index = torch.empty(P, dtype=torch.int32, device=dev)
    a = _cabi.NearestArgs()
    a.num_query, a.num_ref, a.cell_size = P, Q, h
    a.query, a.ref, a.scratch, a.d2, a.index = _ptr(query), _ptr(ref), scratch.data_ptr(), _ptr(d2), _ptr(index)
    _cabi.check(L.mgs_nearest_distance(C.byref(a), stream_ptr(dev)), "mgs_nearest_distance")
    return d2, index


def distance_stats(d2_pred_to_gt, d2_gt_to_pred, threshold: float, sample_records=(None, None),
                   record=None) -> torch.Tensor:
    """The device record [12] f64 of the two directions (include/monogs_raster.h): one launch per direction and a final
    one.  No host read.  `record`: a float64 device tensor whose first twelve elements are written instead of a new one."""
    what = "distance_stats"
    if not torch.is_tensor(d2_pred_to_gt) or d2_pred_to_gt.device.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (HIP kernels, gfx950); distance_stats_numpy runs anywhere")
    dev = d2_pred_to_gt.device
    thr = float(threshold)
    if not thr >= 0.0:
        raise ValueError(f"{what}: threshold must be >= 0, got {threshold}")
    L = _cabi.lib()
    scratch = _workspace("stats", dev, (), L.mgs_mesh_eval_scratch_bytes, what)
    if record is None:
        record = torch.empty(_cabi.MESH_EVAL_RECORD_DOUBLES, dtype=torch.float64, device=dev)
    a = _cabi.MeshEvalArgs()
    a.threshold, a.scratch, a.record = thr, scratch.data_ptr(), record.data_ptr()
    keep = []
    for d, t in enumerate((d2_pred_to_gt, d2_gt_to_pred)):
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
        keep.append(t)
        a.num, a.direction, a.d2 = int(t.shape[0]), d, _ptr(t)
        _cabi.check(L.mgs_mesh_eval_stats(C.byref(a), stream_ptr(dev)), "mgs_mesh_eval_stats")
    for d, r in enumerate(sample_records):
        a.sample_record[d] = None if r is None else r.data_ptr()
    _cabi.check(L.mgs_mesh_eval_finish(C.byref(a), stream_ptr(dev)), "mgs_mesh_eval_finish")
    return record


def normal_stats(pred_side, gt_side, record: torch.Tensor) -> torch.Tensor:
    """The eight doubles of the two directions of normal consistency (include/monogs_raster.h) into `record` [8] f64 on
    the device.  A side is (face of every sample [n] i32, d2 [n], neighbour index [n] i32, face normals [F,3]) of one
    mesh, all on the device of `record`.  One launch per direction and a final one.  No host read."""
    dev = record.device
    L = _cabi.lib()
    scratch = _workspace("normal_stats", dev, (), L.mgs_mesh_eval_normal_scratch_bytes, "normal_stats")
    a = _cabi.MeshEvalNormalArgs()
    a.scratch, a.record = scratch.data_ptr(), record.data_ptr()
    for d, (own, other) in enumerate(((pred_side, gt_side), (gt_side, pred_side))):
        face, d2, index, normal = own
        a.num, a.num_ref, a.num_faces, a.num_ref_faces = (int(t.shape[0]) for t in (face, other[0], normal, other[3]))
        a.direction = d
        a.d2, a.index, a.face, a.ref_face = _ptr(d2), _ptr(index), _ptr(face), _ptr(other[0])
        a.normals, a.ref_normals = _ptr(normal), _ptr(other[3])
        _cabi.check(L.mgs_mesh_eval_normal_stats(C.byref(a), stream_ptr(dev)), "mgs_mesh_eval_normal_stats")
    _cabi.check(L.mgs_mesh_eval_normal_finish(C.byref(a), stream_ptr(dev)), "mgs_mesh_eval_normal_finish")
    return record


def evaluate_mesh(pred, gt, n_samples: int = 200_000, threshold: float = 0.05, seed: int = 0, transform=None,
                  with_record: bool = False, cull=None, normals: bool = False):
    """The geometry scores of the mesh `pred` = (verts, faces) against `gt` = (verts, faces), or a point tensor [M,3]
    that is used as it is: a dict of METRIC_KEYS, in the units of the input.  `transform` - (s, R, t) or a 4x4 matrix,
    e.g. the Sim(3) of the trajectory alignment - is applied to pred's vertices first (apply_transform).  pred is
    sampled with `seed`, gt with `seed + 1`; ONE host read, of the record; bad faces or a mesh without area raise
    ValueError after it.

    `cull` = dict(views=..., occlusion="gt" | "self" | None, eps=0.05, min_views=1, rule="all") applies the visibility
    protocol of mesh_render first: after `transform`, in the ground truth's frame, both meshes lose what fewer than
    `min_views` of `views` (the ground-truth poses) saw - "gt" tests both against the ground-truth mesh's rendered depth,
    "self" each against its own, None the frustum alone - and what is left is scored.  The dict then also holds
    culled_pred_faces and culled_gt_faces, and each of the two culls adds one host read (of its counts).

    `normals=True` (both sides must be meshes) adds NORMAL_KEYS behind METRIC_KEYS: with the unit normals of the two
    meshes as they were sampled (mesh_normals.face_normals), every sample and its nearest neighbour give
    t = n_sample . n_neighbour; normal_accuracy and normal_completion are the mean |t| of pred -> gt and gt -> pred,
    normal_consistency their mean, normal_flipped the share of pairs with t < 0 (0 for two meshes wound alike, 1 when one
    is wound the other way), normal_skipped the pairs without a neighbour or without a normal.  The eight doubles behind
    them travel behind the record's twelve in the same single host read."""
    what = "evaluate_mesh"
    normals = _check_normals(normals, gt)
    pv = _device_points(pred[0], what, "pred verts").detach().to(torch.float32)
    dev = pv.device
    pv = apply_transform(pv, transform)
    culled = None
    if cull is not None:
        from .mesh_render import cull_pair
        kw = _cull_arguments(cull, gt)
        pred, gt, *culled = cull_pair(False, (pv, pred[1]), (_device_points(gt[0], what, "gt verts", dev), gt[1]), **kw)
        pv = pred[0]
    pp, pf, prec = sample_surface(pv, pred[1], n_samples, seed, with_record=True)
    if _is_mesh(gt):
        gv = _device_points(gt[0], what, "gt verts", dev)
        gp, gf, grec = sample_surface(gv, gt[1], n_samples, seed + 1, with_record=True)
    else:
        gp, grec = _device_points(gt, what, "gt points", dev).detach().to(torch.float32).contiguous(), None
    d_pg, i_pg = nearest_distance(pp, gp)
    d_gp, i_gp = nearest_distance(gp, pp)
    N = _cabi.MESH_EVAL_RECORD_DOUBLES
    record = None
    if normals:
        from .mesh_normals import face_normals
        record = torch.empty(N + _cabi.MESH_EVAL_NORMAL_DOUBLES, dtype=torch.float64, device=dev)
        pn, gn = face_normals(pv, pred[1])[0], face_normals(gv, gt[1])[0]
        normal_stats((pf, d_pg, i_pg, pn), (gf, d_gp, i_gp, gn), record[N:])
    record = distance_stats(d_pg, d_gp, threshold, (prec, grec), record).cpu().numpy()        # the one host read
    out = metrics_from_record(record[:N], pp.shape[0], gp.shape[0])
    if normals:
        out.update(normal_metrics_from_record(record[N:]))
    if culled is not None:
        out["culled_pred_faces"], out["culled_gt_faces"] = culled
    return (out, record) if with_record else out
