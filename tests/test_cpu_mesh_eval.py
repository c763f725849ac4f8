"""Mesh evaluation off the GPU (monogs_amd/mesh_eval.py and the C ABI's argument checks): the mirrors against statements
that know nothing of them - Random123's known answers, fp64 barycentric coordinates, SciPy's KD-tree, analytic scenes -
and the refusals of the entry points.

Measured here (mirrors, seed 0): the floaters mesh of mesh_clean_cases against the big sphere alone at 8192 samples per
side and threshold 0.5 voxel scores precision 0.873 / recall 1.0 uncleaned and 1.0 / 1.0 after keep_largest=1, the largest
distance between the two samplings of the sphere being 0.44 voxel; the two-layer volume of surface_cases scores precision
0.625 fused from the mean depth and 1.0 fused from the median depth at threshold = the truncation distance (0.08)."""
import ctypes as C
import functools
import inspect
import math

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_eval_cases as K

TOL = 8.0 * 2.0 ** -24


def test_philox_known_answers():
    from monogs_amd.mesh_eval import philox4x32_10, sample_words_numpy
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, np.uint64), key)
        assert got.dtype == np.uint32 and " ".join(f"{int(w):08x}" for w in got) == want
    batch = philox4x32_10(np.array([k[0] for k in kat[:1]] * 3, np.uint64), (0, 0))
    assert batch.shape == (3, 4) and (batch == batch[0]).all()
    w = sample_words_numpy(5, seed=(7 << 32) | 9)
    assert np.array_equal(w[3], philox4x32_10(np.array([3, 0, 2, 0], np.uint64), (9, 7)))


# ---- the sampler mirror ------------------------------------------------------------------------------------------------
def _assert_on_faces(v, f, points, face_index):
    """fp64 barycentric coordinates of every point on its face: non-negative, summing to 1, the point in the plane."""
    a, b, c = (v[f[face_index, k]].astype(np.float64) for k in range(3))
    p = points.astype(np.float64)
    e, g, r = b - a, c - a, p - a
    ee, eg, gg = (e * e).sum(1), (e * g).sum(1), (g * g).sum(1)
    det = ee * gg - eg * eg
    u = (gg * (r * e).sum(1) - eg * (r * g).sum(1)) / det
    w = (ee * (r * g).sum(1) - eg * (r * e).sum(1)) / det
    extent = np.abs(np.stack([a, b, c])).max(axis=(0, 2))
    residual = np.linalg.norm(r - u[:, None] * e - w[:, None] * g, axis=1)
    assert (residual <= TOL * extent).all(), float((residual / extent).max())
    longest = np.sqrt(np.maximum(np.maximum(ee, gg), ((g - e) ** 2).sum(1)))
    tol = TOL * extent / (np.sqrt(det) / longest)                 # a coordinate moves by (point error) / altitude
    assert (u >= -tol).all() and (w >= -tol).all() and (u + w <= 1.0 + tol).all()


@pytest.mark.parametrize("name", ["odd", "degenerate", "bad_index", "ratio"])
def test_sampler_mirror_points_lie_on_their_faces(name):
    from monogs_amd.mesh_eval import face_weights_numpy, sample_surface_numpy
    v, f = K.sampler_mesh(name)
    p, fi, rec = sample_surface_numpy(v, f, 5000, seed=11, with_record=True)
    assert p.shape == (5000, 3) and p.dtype == np.float32 and fi.shape == (5000,) and fi.dtype == np.int32
    q, bad = face_weights_numpy(v, f)
    assert rec[0] == 0 and rec[1] == bad == (2 if name == "bad_index" else 0)
    assert int(q.sum()) == (int(rec[2]) & 0xFFFFFFFF) | ((int(rec[3]) & 0xFFFFFFFF) << 32)
    assert int(q.max()) < 2 ** 31 and int(q.max()) >= 2 ** 30
    assert (q[fi] > 0).all()                                     # weight-0 faces are never drawn
    assert np.isfinite(p).all()
    _assert_on_faces(v, f, p, fi)
    if name == "ratio":
        legs = K.mesh_ratio()[2]
        assert (q[legs == 1.0] == 0).all() and (q[legs == 256.0] == 2 ** 14).all() and (q[legs == 65536.0] == 2 ** 30).all()
        assert set(np.unique(legs[fi])) == {256.0, 65536.0}
    if name == "degenerate":
        assert (q[100:140] == 0).all() and q[200] == 0 and q[300] == 0 and q[301] == 0 and q[302] == 0
        assert int((q > 0).sum()) == 700 - 44
    if name == "bad_index":
        assert q[17] == 0 and q[250] == 0


def test_sampler_mirror_share_of_a_3_to_1_mesh():
    """Seed 0; the large face's share of 65 536 samples lies within 5 sigma of 0.75 (measured 0.75156)."""
    from monogs_amd.mesh_eval import sample_surface_numpy
    v, f = K.two_triangles_3_to_1()
    n = 65536
    _, fi = sample_surface_numpy(v, f, n, seed=0)
    share = float((fi == 0).mean())
    print(f"share of the large face: {share:.5f}")
    assert abs(share - 0.75) <= 5.0 * math.sqrt(0.75 * 0.25 / n)


def test_sampler_mirror_replays_randoms_and_folds_exactly():
    from monogs_amd.mesh_eval import sample_surface_numpy, sample_words_numpy
    v, f = K.sampler_mesh("odd")
    n = 700
    p, fi = sample_surface_numpy(v, f, n, seed=5)
    words = sample_words_numpy(n, 5)
    p2, fi2 = sample_surface_numpy(v, f, n, seed=99, randoms=words)
    assert np.array_equal(p.view(np.int32), p2.view(np.int32)) and np.array_equal(fi, fi2)
    p3, fi3 = sample_surface_numpy(v, f, n, randoms=words.astype(np.int64).astype(np.int32))     # words held as int32
    assert np.array_equal(p.view(np.int32), p3.view(np.int32)) and np.array_equal(fi, fi3)
    # the extremes of the fold on one triangle: (a, b, c) = (0, x, y)
    tv, tf = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    w = K.replay_words(6, 0)
    tp, tfi = sample_surface_numpy(tv, tf, 6, randoms=w)
    assert (tfi == 0).all()
    top = 1.0 - 2.0 ** -24
    assert np.array_equal(tp[:, :2], np.array([[0, 0], [2.0 ** -24, 2.0 ** -24], [0.5, 0.5], [0.5 - 2.0 ** -24, 0.5],
                                                [top, 0], [0, top]], np.float32))


def test_sampler_mirror_without_area():
    from monogs_amd.mesh_eval import sample_surface_numpy
    for name in ("zero_area", "no_faces"):
        v, f = K.sampler_mesh(name)
        p, fi, rec = sample_surface_numpy(v, f, 33, seed=1, with_record=True)
        assert p.shape == (33, 3) and np.isnan(p).all() and (fi == -1).all() and fi.dtype == np.int32
        assert rec.tolist() == [1, 0, 0, 0]
    p, fi = sample_surface_numpy(*K.sampler_mesh("odd"), 0)
    assert p.shape == (0, 3) and fi.shape == (0,)
    with pytest.raises(ValueError):
        sample_surface_numpy(*K.sampler_mesh("odd"), -1)


# ---- the brute force against SciPy's KD-tree ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd_sizes", "plane", "outlier", "duplicates", "outside", "empty_region", "non_finite",
                                  "surface"])
def test_brute_force_against_the_kd_tree(name):
    from scipy.spatial import cKDTree
    from monogs_amd.mesh_eval import nearest_distance_torch
    q, r, _ = K.nearest_case(name)
    d2, idx = nearest_distance_torch(torch.from_numpy(q), torch.from_numpy(r))
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(q),)
    d, idx = np.sqrt(d2.numpy().astype(np.float64)), idx.numpy()
    ok_r = np.isfinite(r).all(axis=1)
    ok_q = np.isfinite(q).all(axis=1)
    assert np.isinf(d[~ok_q]).all() and (idx[~ok_q] == -1).all()
    keep = np.flatnonzero(ok_r)
    kd, ki = cKDTree(r[keep].astype(np.float64)).query(q[ok_q].astype(np.float64), k=2)
    got_d, got_i = d[ok_q], idx[ok_q]
    assert ok_r[got_i].all()                                     # a non-finite reference point is never a neighbour
    assert (np.abs(got_d - kd[:, 0]) <= 1e-6 * kd[:, 0]).all(), float((np.abs(got_d - kd[:, 0]) / kd[:, 0]).max())
    clear = kd[:, 1] - kd[:, 0] > 2e-6 * kd[:, 1]               # the runner-up is further away than the tolerance
    assert clear.sum() > 0.5 * len(clear) or name == "duplicates"
    assert np.array_equal(got_i[clear], keep[ki[clear, 0]])


@pytest.mark.parametrize("name", ["lattice_ties", "duplicates", "coincident"])
def test_brute_force_ties_take_the_smallest_index(name):
    from monogs_amd.mesh_eval import nearest_distance_torch
    q, r, _ = K.nearest_case(name)
    d2, idx = (t.numpy() for t in nearest_distance_torch(torch.from_numpy(q), torch.from_numpy(r), chunk_elems=50000))
    dx, dy, dz = (q[:, None, k] - r[None, :, k] for k in range(3))
    full = (dx * dx + dy * dy) + dz * dz                         # NumPy fp32: the same single roundings
    assert full.dtype == np.float32
    assert np.array_equal(d2, full.min(axis=1)) and np.array_equal(idx, full.argmin(axis=1))     # argmin: the first
    ties = (full == full.min(axis=1, keepdims=True)).sum(axis=1)
    if name == "lattice_ties":
        assert (ties == 8).all() and (d2 == 0.75).all()
    elif name == "duplicates":
        assert (ties >= 3).all()
    else:
        assert (ties == len(r)).all() and (idx == 0).all()


def test_brute_force_without_neighbours():
    from monogs_amd.mesh_eval import nearest_distance_torch
    for name in ("no_ref", "all_non_finite"):
        q, r, _ = K.nearest_case(name)
        d2, idx = nearest_distance_torch(torch.from_numpy(q), torch.from_numpy(r))
        assert torch.isinf(d2).all() and (idx == -1).all() and d2.shape == (len(q),)
    q, r, _ = K.nearest_case("no_query")
    d2, idx = nearest_distance_torch(torch.from_numpy(q), torch.from_numpy(r))
    assert d2.shape == (0,) and idx.shape == (0,)


# ---- analytic scenes ---------------------------------------------------------------------------------------------------
def test_two_parallel_squares():
    from monogs_amd.mesh_eval import METRIC_KEYS, evaluate_mesh_numpy
    D, pitch = 0.25, 1.0 / 32.0                                  # D^2 and its root are exact in fp32
    far = math.sqrt(D * D + 0.5 * pitch * pitch)
    pred, gt = K.square(0.0, 3), K.square_lattice(D, pitch)
    out, rec = evaluate_mesh_numpy(pred, gt, n_samples=4096, threshold=D * 0.999, with_record=True)
    assert tuple(out) == METRIC_KEYS
    assert out["n_pred"] == 4096 and out["n_gt"] == 33 * 33 and rec[0] == 4096 and rec[4] == 33 * 33
    assert D <= out["accuracy"] <= far * (1 + 1e-6)
    assert out["completion"] >= D and D <= rec[2] <= far * (1 + 1e-6)          # rec[2]: the largest pred -> gt distance
    assert out["chamfer"] == 0.5 * (out["accuracy"] + out["completion"])
    assert out["precision"] == 0.0 and out["recall"] == 0.0 and out["f_score"] == 0.0
    out = evaluate_mesh_numpy(pred, gt, n_samples=4096, threshold=far * 1.001)
    assert out["precision"] == 1.0 and out["recall"] == out["completion_ratio"] > 0.9       # gt -> pred meets 4096 samples
    assert out["f_score"] == 2.0 * out["recall"] / (1.0 + out["recall"])
    # the threshold is compared in fp32, strictly
    out = evaluate_mesh_numpy(pred, gt, n_samples=512, threshold=D)
    assert out["precision"] == 0.0
    # a transform that moves pred onto gt's plane: (s, R, t) and the same as a 4x4 matrix
    lifted = evaluate_mesh_numpy(pred, gt, n_samples=512, threshold=pitch, transform=(1.0, np.eye(3), (0.0, 0.0, D)))
    M = np.eye(4)
    M[2, 3] = D
    assert lifted == evaluate_mesh_numpy(pred, gt, n_samples=512, threshold=pitch, transform=M)
    assert lifted["accuracy"] <= pitch / math.sqrt(2.0) and lifted["precision"] == 1.0


@functools.lru_cache(maxsize=None)
def _floater_scores(cleaned):
    from monogs_amd.mesh_clean import clean_mesh_numpy
    from monogs_amd.mesh_eval import evaluate_mesh_numpy
    v, f, _ = MC.floater_mesh()
    bv, bf, _ = MC.floater_mesh(True)
    if cleaned:
        v, f, _, _ = clean_mesh_numpy(v, f, None, keep_largest=1)
    return evaluate_mesh_numpy((v, f), (bv, bf), n_samples=8192, threshold=0.5 * MC.FLOATER_VOXEL, seed=0)


def test_floaters_cost_precision_and_the_clean_up_restores_it():
    raw, clean = _floater_scores(False), _floater_scores(True)
    print(f"floaters: precision {raw['precision']:.4f} recall {raw['recall']:.4f}; cleaned: precision "
          f"{clean['precision']:.4f} recall {clean['recall']:.4f} hausdorff {clean['hausdorff']:.3f}")
    assert raw["recall"] == 1.0 and raw["precision"] < 0.9
    assert clean["precision"] == 1.0 and clean["recall"] == 1.0


def test_a_mesh_against_itself_under_two_seeds():
    out = _floater_scores(True)                                  # the cleaned mesh IS the big sphere's (test_gpu_mesh_clean)
    assert out["f_score"] == 1.0 and 0.0 < out["chamfer"] < 0.5 and out["hausdorff"] < 0.5


def test_flags_raise():
    from monogs_amd.mesh_eval import evaluate_mesh_numpy
    v, f = K.sampler_mesh("bad_index")
    with pytest.raises(ValueError, match="2 faces"):
        evaluate_mesh_numpy((v, f), K.square(0.0), n_samples=64)
    with pytest.raises(ValueError, match="no face with area"):
        evaluate_mesh_numpy(K.sampler_mesh("zero_area"), K.square(0.0), n_samples=64)
    with pytest.raises(ValueError, match="gt mesh"):
        evaluate_mesh_numpy(K.square(0.0), K.sampler_mesh("no_faces"), n_samples=64)


def test_two_layer_mirrors_show_the_median_step_at_the_truncation_distance():
    """The vertices a mean-depth fusion leaves between the layers (test_cpu_surface.py) as a metric."""
    import surface_cases as SC
    from monogs_amd import surface as SF, tsdf as T, viewer as V
    from monogs_amd.mesh_eval import evaluate_mesh_numpy
    sc = SC.scene("two_layer")
    cam = SC.camera(sc)
    proj = V.project_torch(SC.model(sc), cam)
    median, _ = SF.median_depth_torch(proj, sc.cam.H, sc.cam.W)
    color, depth, opacity = V.blend_torch(proj, sc.cam.H, sc.cam.W, sc.bg)
    vol = SC.LAYER_VOLUME
    nx, ny, nz = vol["dims"]
    trunc = 4.0 * vol["voxel_size"]
    precision = {}
    for mode, plane in (("mean", depth), ("median", median)):
        planes = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
        T.integrate_torch(*planes, vol["origin"], vol["voxel_size"], trunc, plane, cam.T, cam.fx, cam.fy, cam.cx, cam.cy,
                          image=color, opacity=opacity, min_opacity=0.95, normalize=mode == "mean")
        verts, faces, _ = T.extract_mesh_numpy(*(p.numpy() for p in planes), vol["origin"], vol["voxel_size"], 1.0)
        precision[mode] = evaluate_mesh_numpy((verts, faces), K.two_layer_truth(sc.cam), 8192, trunc)["precision"]
    print(f"precision at {trunc}: mean {precision['mean']:.4f}, median {precision['median']:.4f}")
    assert precision["median"] > precision["mean"] and precision["median"] == 1.0


# ---- the boundary ------------------------------------------------------------------------------------------------------
NAMES = ("mgs_surface_sample_args_size", "mgs_surface_sample_scratch_bytes", "mgs_surface_sample",
         "mgs_nearest_args_size", "mgs_nearest_scratch_bytes", "mgs_nearest_distance",
         "mgs_mesh_eval_args_size", "mgs_mesh_eval_scratch_bytes", "mgs_mesh_eval_stats", "mgs_mesh_eval_finish")


def test_exports_struct_sizes_and_abi_version(built):
    from monogs_amd import _cabi
    for n in NAMES:
        assert n in _cabi.EXPORTS, n
    L = _cabi.lib()
    assert L.mgs_surface_sample_args_size() == C.sizeof(_cabi.SurfaceSampleArgs) == 4 * 4 + 8 + 7 * 8
    assert L.mgs_nearest_args_size() == C.sizeof(_cabi.NearestArgs) == 4 * 4 + 5 * 8
    assert L.mgs_mesh_eval_args_size() == C.sizeof(_cabi.MeshEvalArgs) == 4 * 4 + 5 * 8
    assert _cabi.ABI_VERSION == 10 and L.mgs_abi_version() == 10
    assert L.mgs_struct_size(len(_cabi.struct_mirrors())) == -1          # the list ends where it ended


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    fake = 4096                                                           # never dereferenced on the host
    big = (2 ** 31 - 1) // 3
    assert 3 * big < 2 ** 31 <= 3 * (big + 1) and _cabi.MESH_EVAL_MAX_ITEMS == big
    for fn in (L.mgs_surface_sample, L.mgs_nearest_distance, L.mgs_mesh_eval_stats, L.mgs_mesh_eval_finish):
        assert fn(None, None) == -1
    # the sampler
    a = _cabi.SurfaceSampleArgs()
    a.num_verts, a.num_faces, a.num_samples = 8, 4, 16
    assert L.mgs_surface_sample(C.byref(a), None) == -1                   # no scratch
    a.scratch = fake
    assert L.mgs_surface_sample(C.byref(a), None) == -1                   # no record
    a.record = fake
    assert L.mgs_surface_sample(C.byref(a), None) == -1                   # no faces
    a.faces = fake
    assert L.mgs_surface_sample(C.byref(a), None) == -1                   # no verts
    a.verts = fake
    assert L.mgs_surface_sample(C.byref(a), None) == -1                   # no outputs
    a.points = fake
    assert L.mgs_surface_sample(C.byref(a), None) == -1                   # no face_index
    a.face_index = fake
    for field in ("num_verts", "num_faces", "num_samples"):
        keep = getattr(a, field)
        setattr(a, field, -1)
        assert L.mgs_surface_sample(C.byref(a), None) == -1
        setattr(a, field, big + 1)
        assert L.mgs_surface_sample(C.byref(a), None) == -3               # 3 n >= 2^31
        setattr(a, field, keep)
    assert L.mgs_surface_sample_scratch_bytes(-1) == 0 and L.mgs_surface_sample_scratch_bytes(big + 1) == 0
    pad = lambda b: (b + 255) // 256 * 256
    assert L.mgs_surface_sample_scratch_bytes(0) == 256
    F = 262200
    assert L.mgs_surface_sample_scratch_bytes(F) == 256 + pad(4 * F) + pad(8 * F) + pad(8 * 1025)
    assert L.mgs_surface_sample_scratch_bytes(big) > 12 * big
    # nearest distance
    b = _cabi.NearestArgs()
    b.num_query, b.num_ref = 16, 8
    assert L.mgs_nearest_distance(C.byref(b), None) == -1                 # no scratch
    b.scratch = fake
    assert L.mgs_nearest_distance(C.byref(b), None) == -1                 # no ref
    b.ref = fake
    assert L.mgs_nearest_distance(C.byref(b), None) == -1                 # no query
    b.query = b.d2 = fake
    assert L.mgs_nearest_distance(C.byref(b), None) == -1                 # no index
    b.index = fake
    for bad in (-1.0, float("nan")):
        b.cell_size = bad
        assert L.mgs_nearest_distance(C.byref(b), None) == -1
    b.cell_size = 0.0
    for field in ("num_query", "num_ref"):
        keep = getattr(b, field)
        setattr(b, field, -1)
        assert L.mgs_nearest_distance(C.byref(b), None) == -1
        setattr(b, field, big + 1)
        assert L.mgs_nearest_distance(C.byref(b), None) == -3
        setattr(b, field, keep)
    b.num_query = 0
    assert L.mgs_nearest_distance(C.byref(b), None) == 0                  # nothing to answer: no launch
    assert L.mgs_nearest_scratch_bytes(-1) == 0 and L.mgs_nearest_scratch_bytes(big + 1) == 0
    cells = _cabi.NEAREST_MAX_CELLS
    fixed = 256 + pad(4 * cells) + pad(4 * (cells + 1)) + pad(4 * (cells // 256 + 1))
    assert L.mgs_nearest_scratch_bytes(0) == fixed                        # the cap on the cells sizes it without a read
    assert L.mgs_nearest_scratch_bytes(4099) == fixed + pad(4 * 4099) + pad(16 * 4099)
    # the statistics
    c = _cabi.MeshEvalArgs()
    c.num, c.direction, c.threshold = 32, 0, 0.5
    assert L.mgs_mesh_eval_stats(C.byref(c), None) == -1 and L.mgs_mesh_eval_finish(C.byref(c), None) == -1   # no scratch
    c.scratch = fake
    assert L.mgs_mesh_eval_stats(C.byref(c), None) == -1                  # no d2
    assert L.mgs_mesh_eval_finish(C.byref(c), None) == -1                 # no record
    c.d2 = c.record = fake
    for direction in (-1, 2):
        c.direction = direction
        assert L.mgs_mesh_eval_stats(C.byref(c), None) == -1
    c.direction = 1
    for bad in (-0.5, float("nan")):
        c.threshold = bad
        assert L.mgs_mesh_eval_stats(C.byref(c), None) == -1
    c.threshold = 0.5
    c.num = -1
    assert L.mgs_mesh_eval_stats(C.byref(c), None) == -1 and L.mgs_mesh_eval_finish(C.byref(c), None) == -1
    c.num = big + 1
    assert L.mgs_mesh_eval_stats(C.byref(c), None) == -3
    assert L.mgs_mesh_eval_scratch_bytes() == 2 * 256 * 32


def test_device_entry_points_raise_off_the_gpu():
    from monogs_amd import mesh_eval as ME
    v, f = (torch.from_numpy(t) for t in K.sampler_mesh("odd"))
    pts = torch.from_numpy(K.nearest_case("odd_sizes")[0])
    with pytest.raises(RuntimeError, match="GPU only"):
        ME.sample_surface(v, f, 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        ME.sample_surface(v.numpy(), f.numpy(), 100)
    with pytest.raises(RuntimeError, match="GPU only"):
        ME.nearest_distance(pts, pts)
    with pytest.raises(RuntimeError, match="GPU only"):
        ME.distance_stats(pts[:, 0], pts[:, 1], 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ME.evaluate_mesh((v, f), (v, f))


def test_plumbing_defaults_to_off():
    from monogs_amd import slam_surrogate
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_eval import evaluate_mesh, evaluate_mesh_numpy
    p = inspect.signature(save_mesh).parameters
    assert p["gt"].default is None and p["eval_kw"].default is None
    p = inspect.signature(slam_surrogate.evaluate_mesh).parameters
    assert list(p)[:4] == ["result", "gt", "voxel_size", "monocular"] and p["monocular"].default is True
    for fn in (evaluate_mesh, evaluate_mesh_numpy):
        p = inspect.signature(fn).parameters
        assert (p["n_samples"].default, p["threshold"].default, p["seed"].default, p["transform"].default) == (
            200_000, 0.05, 0, None)
