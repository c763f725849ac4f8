"""The mirrors of mesh rendering and culling (monogs_amd/mesh_render.py) against independent statements: exact depths and
covered sets of a fronto-parallel square, the analytic ray-plane depth of a slanted plane, a closed room without cracks,
the shadow of a pillar, the cull's bookkeeping, and the two scenes in which the protocol has to move a score.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_render_cases as RC


def _render(name, **kw):
    return RC.mirror_render(name, **kw)


# ---- render_mesh_depth_numpy -----------------------------------------------------------------------------------------
def test_fronto_parallel_square_is_exact_closed_and_tie_broken():
    depth, face, record = _render("square")
    x0, y0, x1, y1 = RC.SQUARE_CORNERS
    ys, xs = np.mgrid[0:16, 0:16]
    inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)          # the CLOSED square: its edge pixels included
    assert np.array_equal(face >= 0, inside)
    assert np.all(depth[inside] == np.float32(2.0)) and np.all(depth[~inside] == 0.0) and np.all(face[~inside] == -1)
    diagonal = inside & (xs - x0 == ys - y0)                            # shared by both triangles: the smaller id
    assert diagonal.sum() == 9 and np.all(face[diagonal] == 0)
    assert np.all(face[inside & (xs - x0 > ys - y0)] == 0) and np.all(face[inside & (xs - x0 < ys - y0)] == 1)
    assert tuple(record) == RC.RECORDS["square"]


def test_slanted_plane_against_the_ray_plane_depth():
    """The rendered depth is the exact perspective interpolation of the SNAPPED triangle.  1 / z is affine in (u, v); a
    vertex moved by at most 1/512 pixel per axis changes the interpolated 1 / z by at most (|g_u| + |g_v|) / 512 inside
    the triangle, i.e. the depth by (|z_u| + |z_v|) / 512 with z_u = z^2 a / (c fx), z_v = z^2 b / (c fy) the depth
    gradient per pixel; z is taken at its largest over the image grown by a pixel, which also covers the second order.  On
    top: the fp32 roundings of the vertices' z, of zc and of the result, and the fp32 error of u, v (a few ulp of 70
    pixels, 1e-5 pixel) - eight ulp of the largest depth in all."""
    depth, face, record = _render("slanted")
    c, a, b = RC.SLANT
    _, fx, fy, cx, cy, H, W = RC.SLANT_VIEW
    ys, xs = np.mgrid[-1:H + 1, -1:W + 1].astype(np.float64)
    z = c / (1.0 - a * (xs - cx) / fx - b * (ys - cy) / fy)
    zmax = z.max()
    bound = zmax ** 2 * (abs(a) / fx + abs(b) / fy) / c / 512.0 + 8.0 * 2.0 ** -23 * zmax
    err = np.abs(depth.astype(np.float64) - z[1:-1, 1:-1])
    print(f"slanted plane: largest error {err.max():.3e}, bound {bound:.3e}")
    assert np.all(face >= 0) and err.max() <= bound
    assert bound < 1e-4                                                 # the bound means something: 3e-5 of the depth
    assert tuple(record) == RC.RECORDS["slanted"]


def test_closed_box_from_inside_has_no_cracks():
    depth, face, record = _render("box_inside")
    _, _, _, _, _, H, W = RC.WIDE_VIEW
    assert int((face >= 0).sum()) == H * W and np.all(depth > 0)
    walls = np.unique(face // 128)                                      # 2 x 8 x 8 faces per wall
    assert 5 in walls and len(walls) >= 3                               # the far wall and some of the others
    assert record[0] == 0 and record[1] > 0                             # the faces around and behind the camera are skipped


@pytest.mark.parametrize("name", sorted(RC.RECORDS))
def test_records_of_the_special_cases(name):
    depth, face, record = _render(name)
    assert tuple(record) == RC.RECORDS[name]
    assert depth.dtype == np.float32 and face.dtype == np.int32 and record.dtype == np.int32
    assert np.array_equal(depth > 0, face >= 0)
    drawn = set(np.unique(face[face >= 0]).tolist())
    want = {"behind_and_nan": {0}, "bad_index": {0}, "zero_area": {2}, "coplanar_duplicates": {0}, "snap_limit": {0, 1},
            "large_boxes": {0, 1, 2}, "empty_faces": set(), "empty_all": set()}
    if name in want:
        assert drawn == want[name]


def test_threshold_changes_the_record_only():
    base = _render("large_boxes")
    for thr, large in ((0, 3), (1023, 3), (1024, 2), (1025, 1), (70 * 45, 0)):
        depth, face, record = _render("large_boxes", large_threshold=thr)
        assert record[2] == large
        assert np.array_equal(depth.view(np.int32), base[0].view(np.int32)) and np.array_equal(face, base[1])


# ---- vertex_visibility_torch -----------------------------------------------------------------------------------------
def test_pillar_hides_the_wall_behind_it():
    from monogs_amd.mesh_render import project_numpy, vertex_visibility_torch
    v, f, (T, fx, fy, cx, cy, H, W) = RC.render_case("pillar_room")
    depth, _, _ = _render("pillar_room")
    eps = 0.05
    with_depth = vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W, depth=depth, eps=eps)
    frustum = vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W)
    assert with_depth.dtype == torch.int32 and tuple(with_depth.shape) == (v.shape[0],)
    hidden, clear = RC.pillar_vertex_sets()
    assert len(hidden) == 15 and len(clear) == 20
    assert np.all(with_depth.numpy()[hidden] == 0) and np.all(frustum.numpy()[hidden] == 1)
    assert np.all(with_depth.numpy()[clear] == 1) and np.all(frustum.numpy()[clear] == 1)
    # the margin: the wall's own rendered depth at the vertex's pixel differs from the vertex's by far less than eps
    u, w, zc = project_numpy(v, T, fx, fy, cx, cy)
    px, py = np.floor(u[clear] + 0.5).astype(int), np.floor(w[clear] + 0.5).astype(int)
    gap = np.abs(zc[clear] - depth[py, px]).max()
    print(f"pillar room: largest self-depth discrepancy on the clear wall {gap:.2e}")
    assert gap < 0.5 * eps
    # behind the camera and outside the image: never seen; the count accumulates in place
    assert np.all(frustum.numpy()[v[:, 2] == -2.0] == 0)
    again = vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W, depth=depth, eps=eps, out=frustum)
    assert again is frustum and np.array_equal(frustum.numpy()[clear], np.full(20, 2, np.int32))
    # a pixel without depth passes iff empty_visible
    nothing = np.zeros((H, W), np.float32)
    assert np.array_equal(vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W, depth=nothing).numpy(),
                          vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W).numpy())
    assert int(vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W, depth=nothing, empty_visible=False).sum()) == 0


# ---- cull_mesh_numpy -------------------------------------------------------------------------------------------------
def test_cull_mesh_keeps_order_and_drops_the_unreferenced():
    from monogs_amd.mesh_render import INFO_KEYS, cull_mesh_numpy
    v = np.arange(24, dtype=np.float32).reshape(8, 3)
    col = v[::-1].copy()
    f = np.array([[0, 1, 2], [2, 3, 4], [5, 4, 3], [0, 0, 8], [6, 6, 6]], np.int32)       # face 3 is bad; 7 is unreferenced
    seen = np.array([1, 1, 1, 0, 2, 2, 0, 5], np.int32)
    ov, of, oc, info = cull_mesh_numpy(v, f, col, seen_count=seen)
    assert tuple(info) == INFO_KEYS
    assert info == dict(verts_in=8, faces_in=5, verts_out=3, faces_out=1, bad_faces=1)
    assert np.array_equal(ov, v[:3]) and np.array_equal(oc, col[:3]) and of.tolist() == [[0, 1, 2]]
    ov, of, oc, info = cull_mesh_numpy(v, f, col, seen_count=seen, rule="any")
    assert np.array_equal(ov, v[:6]) and of.tolist() == [[0, 1, 2], [2, 3, 4], [5, 4, 3]] and info["verts_out"] == 6
    ov, of, oc, info = cull_mesh_numpy(v, f, None, seen_count=seen, min_views=2, rule="any")
    assert oc is None and np.array_equal(ov, v[2:6]) and of.tolist() == [[0, 1, 2], [3, 2, 1]]
    assert cull_mesh_numpy(v, f, None, seen_count=seen, min_views=2)[3]["faces_out"] == 0
    assert of.dtype == np.int32 and ov.dtype == np.float32


@pytest.mark.parametrize("param", RC.CULL_PARAMS, ids=lambda p: f"{p[0]}-m{p[1]}-{p[2]}")
def test_cull_mesh_against_a_plain_loop(param):
    from monogs_amd.mesh_render import cull_mesh_numpy
    which, min_views, rule = param
    v, f, _ = RC.render_case("pillar_room")
    seen = RC.seen_vectors(v.shape[0])[which]
    keep_f, used = [], set()
    for face in f.tolist():
        flags = [seen[i] >= min_views for i in face]
        if (any(flags) if rule == "any" else all(flags)):
            keep_f.append(face)
            used.update(face)
    order = sorted(used)
    index = {old: new for new, old in enumerate(order)}
    ov, of, _, info = cull_mesh_numpy(v, f, None, seen_count=seen, min_views=min_views, rule=rule)
    assert np.array_equal(ov, v[order]) and of.tolist() == [[index[i] for i in face] for face in keep_f]
    assert info["verts_out"] == len(order) and info["faces_out"] == len(keep_f) and info["bad_faces"] == 0
    if which == "none":
        assert info["faces_out"] == 0 and info["verts_out"] == 0
    if which == "every":
        assert info["faces_out"] == f.shape[0] and info["verts_out"] == v.shape[0]


# ---- the protocol ----------------------------------------------------------------------------------------------------
_KW = dict(n_samples=RC.SPHERE_SAMPLES, threshold=RC.SPHERE_THRESHOLD, seed=0)


def test_hidden_sphere_costs_precision_until_it_is_culled():
    """Measured with seed 0, 4000 samples, threshold 0.2: un-culled precision 0.80125, recall 1.0, accuracy 0.12267;
    culled (occlusion "self"): precision 1.0, recall 1.0, 224 of pred's faces dropped - the whole inner sphere - and none
    of gt's.  The frustum-only test drops nothing: the inner sphere is inside every frustum."""
    from monogs_amd.mesh_eval import METRIC_KEYS, evaluate_mesh_numpy
    pred, gt, views = RC.hidden_sphere()
    raw = evaluate_mesh_numpy(pred, gt, **_KW)
    assert tuple(raw) == METRIC_KEYS                                    # cull=None: today's dict
    assert raw["precision"] < 0.9 and raw["recall"] == 1.0
    for occlusion in ("self", "gt"):
        out = evaluate_mesh_numpy(pred, gt, cull=dict(views=views, occlusion=occlusion), **_KW)
        assert tuple(out) == METRIC_KEYS + ("culled_pred_faces", "culled_gt_faces")
        assert out["precision"] == 1.0 and out["recall"] == 1.0 and out["f_score"] == 1.0
        assert out["culled_pred_faces"] == 224 and out["culled_gt_faces"] == 0
    frustum = evaluate_mesh_numpy(pred, gt, cull=dict(views=views, occlusion=None), **_KW)
    assert frustum["culled_pred_faces"] == 0 and frustum["precision"] == raw["precision"]


def test_far_hemisphere_costs_recall_until_it_is_culled():
    """Measured with seed 0, 4000 samples, threshold 0.2: un-culled recall 0.77925 (completion 0.12854), precision 1.0;
    culled: recall 1.0, 326 of gt's 960 faces dropped, none of pred's."""
    from monogs_amd.mesh_eval import evaluate_mesh_numpy
    pred, gt, views = RC.far_hemisphere()
    raw = evaluate_mesh_numpy(pred, gt, **_KW)
    assert raw["recall"] < 0.9 and raw["precision"] == 1.0
    out = evaluate_mesh_numpy(pred, gt, cull=dict(views=views, occlusion="self"), **_KW)
    assert out["recall"] == 1.0 and out["precision"] == 1.0
    assert out["culled_gt_faces"] == gt[1].shape[0] - pred[1].shape[0] == 326 and out["culled_pred_faces"] == 0


def test_cull_by_visibility_options_and_depth_l1():
    from monogs_amd.mesh_render import cull_by_visibility_numpy, mesh_depth_l1_numpy, view_tuple
    v, f, view = RC.render_case("pillar_room")
    depth, _, _ = _render("pillar_room")
    hidden, clear = RC.pillar_vertex_sets()
    wall = (v[clear[0]], v[hidden[0]])
    own = cull_by_visibility_numpy((v, f), [view])[0]
    planes = cull_by_visibility_numpy((v, f), [view], occluder=None, depth_planes=[depth])[0]
    frustum = cull_by_visibility_numpy((v, f), [view], occluder=None)[0]
    has = lambda vs, p: bool((vs == p).all(axis=1).any())
    assert np.array_equal(own, planes)                                  # the supplied plane is the rendered one
    assert has(own, wall[0]) and not has(own, wall[1]) and has(frustum, wall[1])
    assert cull_by_visibility_numpy((v, f), [view, view], min_views=2)[3] == cull_by_visibility_numpy((v, f), [view])[3]
    assert cull_by_visibility_numpy((v, f), [], occluder=None)[3]["faces_out"] == 0

    class Camera:
        T, fx, fy, cx, cy, image_height, image_width = view

    assert view_tuple(Camera())[1:] == view[1:]
    with pytest.raises(ValueError):
        view_tuple((view[0], 1.0, 1.0))
    # the square at depth 2.0 against the same square at 2.5, moved there by a transform: |d_pred - d_gt| = 0.5 and 0
    sv, sf, sview = RC.render_case("square")
    gt = (sv * np.float32(1.25), sf)                                    # scaled about the camera: the same pixels
    assert mesh_depth_l1_numpy((sv, sf), gt, [sview, sview]) == (0.5, 162)
    assert mesh_depth_l1_numpy((sv, sf), gt, [sview], transform=(1.25, np.eye(3), np.zeros(3))) == (0.0, 81)
    far = (RC.look(16, 16, 16.0, RC.pose(3.0)),)                        # looks away: no common pixel
    value, pixels = mesh_depth_l1_numpy((sv, sf), gt, far)
    assert np.isnan(value) and pixels == 0


# ---- the boundary ----------------------------------------------------------------------------------------------------
NAMES = ("mgs_mesh_render_args_size", "mgs_mesh_render_scratch_bytes", "mgs_mesh_render",
         "mgs_vertex_visibility_args_size", "mgs_vertex_visibility",
         "mgs_mesh_cull_args_size", "mgs_mesh_cull_scratch_bytes", "mgs_mesh_cull_count", "mgs_mesh_cull_emit")


def test_exports_and_struct_sizes(built):
    from monogs_amd import _cabi
    for n in NAMES:
        assert n in _cabi.EXPORTS, n
    L = _cabi.lib()
    assert L.mgs_mesh_render_args_size() == C.sizeof(_cabi.MeshRenderArgs) == 12 * 4 + 7 * 8
    assert L.mgs_vertex_visibility_args_size() == C.sizeof(_cabi.VertexVisibilityArgs) == 10 * 4 + 4 * 8
    assert L.mgs_mesh_cull_args_size() == C.sizeof(_cabi.MeshCullArgs) == 4 * 4 + 9 * 8 + 2 * 4
    assert _cabi.MESH_RENDER_LARGE_BOX == 1024 and _cabi.MESH_RENDER_RECORD_INTS == 4 and _cabi.MESH_CULL_COUNTS == 4


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    fake = 4096                                                           # never dereferenced on the host
    big = (2 ** 31 - 1) // 3
    for fn in (L.mgs_mesh_render, L.mgs_vertex_visibility, L.mgs_mesh_cull_count, L.mgs_mesh_cull_emit):
        assert fn(None, None) == -1
    a = _cabi.MeshRenderArgs()
    a.num_verts, a.num_faces, a.width, a.height, a.large_threshold = 8, 4, 70, 45, 1024
    a.fx = a.fy = 16.0
    for field in ("T", "scratch", "depth", "face_id", "record", "faces", "verts"):
        assert L.mgs_mesh_render(C.byref(a), None) == -1                  # `field` is still missing
        setattr(a, field, fake)
    for field, bad, status in (("width", 0, -1), ("height", 0, -1), ("num_verts", -1, -1), ("num_faces", -1, -1),
                               ("large_grid", -1, -1), ("num_verts", big + 1, -3), ("num_faces", big + 1, -3),
                               ("fx", float("nan"), -1), ("z_near", float("nan"), -1)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert L.mgs_mesh_render(C.byref(a), None) == status, field
        setattr(a, field, keep)
    a.width, a.height = 65536, 32768                                      # H W = 2^31
    assert L.mgs_mesh_render(C.byref(a), None) == -3
    pad = lambda b: (b + 255) // 256 * 256
    assert L.mgs_mesh_render_scratch_bytes(45, 70, 1003) == pad(8 * 3150) + pad(4 * 1003) + 256
    assert L.mgs_mesh_render_scratch_bytes(32768, 65536, 4) == 0 and L.mgs_mesh_render_scratch_bytes(0, 70, 4) == 0
    assert L.mgs_mesh_render_scratch_bytes(45, 70, big + 1) == 0 and L.mgs_mesh_render_scratch_bytes(45, 70, -1) == 0
    assert L.mgs_mesh_render_scratch_bytes(32768, 65535, 0) > 0
    b = _cabi.VertexVisibilityArgs()
    b.num_verts, b.width, b.height = 8, 70, 45
    for field in ("T", "verts", "seen_count"):
        assert L.mgs_vertex_visibility(C.byref(b), None) == -1
        setattr(b, field, fake)
    for field, bad, status in (("width", 0, -1), ("num_verts", -1, -1), ("num_verts", big + 1, -3),
                               ("eps", float("nan"), -1)):
        keep = getattr(b, field)
        setattr(b, field, bad)
        assert L.mgs_vertex_visibility(C.byref(b), None) == status, field
        setattr(b, field, keep)
    c = _cabi.MeshCullArgs()
    c.num_verts, c.num_faces = 8, 4
    for field in ("scratch", "faces", "counts", "seen_count"):
        assert L.mgs_mesh_cull_count(C.byref(c), None) == -1
        setattr(c, field, fake)
    for field, bad, status in (("rule", 2, -1), ("rule", -1, -1), ("num_verts", -1, -1), ("num_faces", big + 1, -3)):
        keep = getattr(c, field)
        setattr(c, field, bad)
        assert L.mgs_mesh_cull_count(C.byref(c), None) == status, field
        setattr(c, field, keep)
    c.out_num_verts, c.out_num_faces = 9, 0                               # more than went in
    assert L.mgs_mesh_cull_emit(C.byref(c), None) == -1
    c.out_num_verts, c.out_num_faces = 3, 1                               # no arrays to write to
    assert L.mgs_mesh_cull_emit(C.byref(c), None) == -1
    c.out_num_verts = c.out_num_faces = 0
    assert L.mgs_mesh_cull_emit(C.byref(c), None) == 0                    # nothing to emit: nothing launched
    assert L.mgs_mesh_cull_scratch_bytes(0, 0) == 256
    assert L.mgs_mesh_cull_scratch_bytes(636, 960) == pad(4 * 636) + pad(4 * 960) + pad(16 * 4)
    assert L.mgs_mesh_cull_scratch_bytes(big + 1, 4) == 0 and L.mgs_mesh_cull_scratch_bytes(4, -1) == 0


def test_python_entry_points_refuse():
    from monogs_amd import mesh_render as MR
    v, f, (T, fx, fy, cx, cy, H, W) = RC.render_case("square")
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for call in (lambda: MR.render_mesh_depth(tv, tf, T, fx, fy, cx, cy, H, W),
                 lambda: MR.vertex_visibility(tv, T, fx, fy, cx, cy, H, W),
                 lambda: MR.cull_mesh(tv, tf, seen_count=torch.zeros(4, dtype=torch.int32)),
                 lambda: MR.cull_by_visibility((tv, tf), [(T, fx, fy, cx, cy, H, W)]),
                 lambda: MR.mesh_depth_l1((tv, tf), (tv, tf), [(T, fx, fy, cx, cy, H, W)])):
        with pytest.raises(RuntimeError, match="GPU only"):                 # off the GPU: no fall-back
            call()
    with pytest.raises(ValueError, match="H and W"):
        MR.render_mesh_depth_numpy(v, f, T, fx, fy, cx, cy, 0, W)
    with pytest.raises(ValueError, match="2\\^31"):
        MR.render_mesh_depth_numpy(v, f, T, fx, fy, cx, cy, 32768, 65536)
    with pytest.raises(ValueError, match="2\\^31"):
        MR._check_counts("render_mesh_depth", 4, (2 ** 31 - 1) // 3 + 1)
    with pytest.raises(ValueError, match="rule"):
        MR.cull_mesh_numpy(v, f, seen_count=np.zeros(4, np.int32), rule="most")
    with pytest.raises(ValueError, match="seen_count"):
        MR.cull_mesh_numpy(v, f, seen_count=np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="depth"):
        MR.vertex_visibility_torch(v, T, fx, fy, cx, cy, H, W, depth=np.zeros((3, 3), np.float32))
    from monogs_amd.mesh_eval import evaluate_mesh_numpy
    with pytest.raises(ValueError, match="views"):
        evaluate_mesh_numpy((v, f), (v, f), n_samples=16, cull=dict(occlusion="gt"))
    with pytest.raises(ValueError, match="occlusion"):
        evaluate_mesh_numpy((v, f), (v, f), n_samples=16, cull=dict(views=[], occlusion="other"))
    with pytest.raises(ValueError, match="mesh"):
        evaluate_mesh_numpy((v, f), v, n_samples=16, cull=dict(views=[]))
