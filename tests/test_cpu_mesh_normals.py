"""Mesh normals without a GPU: the mirrors (face and vertex normals, normal consistency, frames of a mesh), the PLY
layout with normals, and the entry points' argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_eval_cases as K
import mesh_normal_cases as N
import mesh_render_cases as R


# ---- face normals ------------------------------------------------------------------------------------------------------
def test_face_normals_of_hand_made_triangles():
    from monogs_amd.mesh_normals import face_normals_numpy
    v, f, want = N.axis_triangles()
    n, rec = face_normals_numpy(v, f)
    assert n.dtype == np.float32 and np.array_equal(n, want) and rec.tolist() == [0, 0]
    # a slanted face: (1,1,1) / sqrt(3) to the last bit of fp32 arithmetic
    n, _ = face_normals_numpy(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), [[0, 1, 2]])
    assert np.array_equal(n[0], np.full(3, np.float32(1.0) / np.sqrt(np.float32(3.0)), np.float32))


def test_face_normals_of_bad_and_degenerate_faces():
    from monogs_amd.mesh_normals import face_normals_numpy
    v, f = K.sampler_mesh("bad_index")
    n, rec = face_normals_numpy(v, f)
    assert rec.tolist() == [2, 0] and not n[[17, 250]].any()
    assert np.abs(np.linalg.norm(np.delete(n, [17, 250], 0), axis=1) - 1).max() < 1e-6
    v, f = K.sampler_mesh("degenerate")
    n, rec = face_normals_numpy(v, f)
    dead = list(range(100, 140)) + [200, 300, 301, 302]        # no area, three equal points, NaN, infinity, overflow
    assert rec.tolist() == [0, len(dead)] and not n[dead].any() and np.isfinite(n).all()
    v, f = K.sampler_mesh("zero_area")
    assert face_normals_numpy(v, f)[1].tolist() == [0, 50]
    n, rec = face_normals_numpy(*K.sampler_mesh("no_faces"))
    assert n.shape == (0, 3) and rec.tolist() == [0, 0]
    n, rec = face_normals_numpy(np.zeros((0, 3), np.float32), [[0, 1, 2]])
    assert rec.tolist() == [1, 0] and not n.any()


# ---- vertex normals ----------------------------------------------------------------------------------------------------
def test_vertex_normals_of_a_sphere_point_outward():
    from monogs_amd.mesh_normals import vertex_normals_numpy
    v, f = N.sphere()
    assert v.shape == (482, 3) and f.shape == (960, 3)
    n, rec = vertex_normals_numpy(v, f)
    assert n.dtype == np.float32 and rec.tolist() == [0, 0]
    ref = N.area_normals_float64(v, f)
    radial = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    worst = (ref * radial).sum(axis=1).min()
    assert abs(worst - 0.99943) < 1e-5                           # the float64 area-weighted sum at its worst vertex
    assert (n.astype(np.float64) * radial).sum(axis=1).min() > 0.999
    assert np.abs(n - ref).max() < 1e-6                          # the fixed point against the float64 sum


def test_vertex_normals_special_cases():
    from monogs_amd.mesh_normals import vertex_normals_numpy
    v, f, expected = N.special()
    n, rec = vertex_normals_numpy(v, f)
    assert rec.tolist() == [0, 0]
    for row, want in zip(n, expected):
        assert row.tolist() == ([0.0, 0.0, 0.0] if want is None else list(want))
    # the small face alone is the largest: its vertices get a normal
    n, _ = vertex_normals_numpy(v, f[3:])
    assert n[7:].tolist() == [[0.0, 0.0, 1.0]] * 3 and not n[:7].any()
    # bad faces are counted and left out; no face at all, and no usable face
    bv, bf = K.sampler_mesh("bad_index")
    n, rec = vertex_normals_numpy(bv, bf)
    assert rec.tolist() == [2, 0] and not n[3 * 17:3 * 17 + 3].any() and np.isfinite(n).all()
    n, rec = vertex_normals_numpy(*K.sampler_mesh("no_faces"))
    assert n.shape == (5, 3) and not n.any() and rec.tolist() == [0, 0]
    zv, zf = K.sampler_mesh("zero_area")
    n, rec = vertex_normals_numpy(zv, zf)
    assert not n.any() and rec.tolist() == [0, 50]
    dv, df = K.sampler_mesh("degenerate")
    n, rec = vertex_normals_numpy(dv, df)
    assert rec[0] == 0 and rec[1] >= 43 and np.isfinite(n).all()


def test_extracted_mesh_is_wound_towards_the_positive_tsdf():
    """tsdf._tet_table winds every triangle so that its normal points to the outside corners, the positive-TSDF side.
    The floater volume's TSDF is positive outside its sphere: every vertex normal of the extraction points away from
    the centre."""
    from monogs_amd.mesh_normals import vertex_normals_numpy
    v, f, _ = MC.floater_mesh(big_only=True)
    assert (v.shape[0], f.shape[0]) == MC.BIG_ONLY_VF
    n, rec = vertex_normals_numpy(v, f)
    assert rec.tolist() == [0, 0]
    centre = np.asarray(MC.FLOATER_SPHERES[0][0])
    radial = v - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (n * radial).sum(axis=1)
    print(f"extraction: n . radial in [{dots.min():.4f}, {dots.max():.4f}]")
    assert dots.min() > 0.9


# ---- normal consistency ------------------------------------------------------------------------------------------------
def test_normal_consistency_of_two_spheres():
    from monogs_amd.mesh_eval import METRIC_KEYS, NORMAL_KEYS
    out, rec = N.mirror_scores("spheres")
    assert tuple(out) == METRIC_KEYS + NORMAL_KEYS and rec.shape == (20,)
    print({k: out[k] for k in NORMAL_KEYS})
    assert out["normal_consistency"] > 0.99 and out["normal_flipped"] == 0 and out["normal_skipped"] == 0
    assert abs(out["normal_accuracy"] - 0.9965) < 2e-4 and abs(out["normal_completion"] - 0.9964) < 2e-4
    assert out["normal_consistency"] == 0.5 * (out["normal_accuracy"] + out["normal_completion"])
    assert rec[12] == rec[16] == N.EVAL_SAMPLES


def test_normal_consistency_flags_a_flipped_winding():
    out, _ = N.mirror_scores("flipped")
    assert out["normal_flipped"] == 1.0 and out["normal_consistency"] > 0.99 and out["normal_skipped"] == 0


def test_normal_consistency_of_a_rotated_box_is_low():
    out, _ = N.mirror_scores("box")
    print(out["normal_accuracy"], out["normal_completion"])
    assert out["normal_consistency"] < 0.8
    assert abs(out["normal_accuracy"] - 0.716) < 2e-3 and abs(out["normal_completion"] - 0.724) < 2e-3


def test_normals_keyword_leaves_the_old_path_alone():
    from monogs_amd.mesh_eval import METRIC_KEYS, evaluate_mesh_numpy
    pred, gt = N.eval_scenes()["spheres"]
    kw = dict(n_samples=N.EVAL_SAMPLES, threshold=0.05, seed=N.EVAL_SEED, with_record=True)
    old, rec = evaluate_mesh_numpy(pred, gt, **kw)
    assert tuple(old) == METRIC_KEYS and rec.shape == (12,)
    new, nrec = N.mirror_scores("spheres")
    assert np.array_equal(rec.view(np.int64), nrec[:12].view(np.int64))
    assert all(new[k] == old[k] for k in METRIC_KEYS)
    with pytest.raises(ValueError, match="normals=True"):
        evaluate_mesh_numpy(pred, gt[0], n_samples=64, normals=True)         # a point tensor as ground truth


def test_normal_stats_skip_rules():
    from monogs_amd.mesh_eval import normal_metrics_from_record, normal_stats_numpy
    nn = np.array([[0, 0, 1], [0, 0, 0], [1, 0, 0]], np.float32)
    mm = np.array([[0, 0, -1], [0, 1, 0]], np.float32)
    face = [0, 1, 2, 0, 0, 0, -1]
    d2 = np.array([0.1, 0.1, 0.1, np.inf, 0.1, np.nan, 0.1], np.float32)
    index = [0, 0, 1, 0, -1, 0, 0]
    st = normal_stats_numpy(face, d2, index, [0, 1], nn, mm)
    assert st == dict(n=2, sum=1.0, flipped=1, skipped=5)
    out = normal_metrics_from_record([2, 1.0, 1, 5, 0, 0.0, 0, 3])
    assert out["normal_accuracy"] == 0.5 and np.isnan(out["normal_completion"]) and out["normal_flipped"] == 0.5
    assert out["normal_skipped"] == 8


# ---- PLY -------------------------------------------------------------------------------------------------------------
def test_mesh_ply_with_normals(tmp_path):
    from monogs_amd.mesh_normals import vertex_normals_numpy
    from monogs_amd.ply_io import read_mesh_ply, write_mesh_ply
    v, f = N.sphere()
    n = vertex_normals_numpy(v, f)[0]
    col = N.frame_colors(v.shape[0], u8=True)
    with_n, without = str(tmp_path / "n.ply"), str(tmp_path / "p.ply")
    write_mesh_ply(with_n, v, f, torch.from_numpy(col), normals=n)
    write_mesh_ply(without, v, f, torch.from_numpy(col))
    head = open(with_n, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    props = [ln.split()[-1] for ln in head if ln.startswith("property") and "list" not in ln]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert os.path.getsize(with_n) - os.path.getsize(without) == 12 * v.shape[0] + len("property float nx\n") * 3
    rv, rf, rc, rn = read_mesh_ply(with_n, with_normals=True)
    assert np.array_equal(rn.numpy().view(np.int32), n.view(np.int32)) and np.array_equal(rv.numpy().view(np.int32), v.view(np.int32))
    assert np.array_equal(rf.numpy(), f) and np.array_equal(rc.numpy(), col)
    three = read_mesh_ply(with_n)
    assert len(three) == 3 and torch.equal(three[0], rv) and torch.equal(three[1], rf) and torch.equal(three[2], rc)
    pv, pf, pc, pn = read_mesh_ply(without, with_normals=True)
    assert pn is None and torch.equal(pv, rv) and torch.equal(pf, rf) and torch.equal(pc, rc)
    with pytest.raises(ValueError, match="normals"):
        write_mesh_ply(with_n, v, f, normals=n[:-1])


def test_mesh_ply_without_normals_is_the_old_file(tmp_path):
    """The bytes of a file without normals, stated independently: the header as it has always been, V rows of three
    little-endian floats and three bytes, F rows of a count and three little-endian ints."""
    from monogs_amd.ply_io import write_mesh_ply
    v, f, _ = N.axis_triangles()
    col = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]], np.uint8)
    path = str(tmp_path / "old.ply")
    write_mesh_ply(path, v, f, torch.from_numpy(col))
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 4\n"
            b"property list uchar int vertex_indices\nend_header\n")
    want += b"".join(v[i].astype("<f4").tobytes() + col[i].tobytes() for i in range(4))
    want += b"".join(b"\x03" + f[i].astype("<i4").tobytes() for i in range(4))
    assert open(path, "rb").read() == want


# ---- frames ------------------------------------------------------------------------------------------------------------
def test_frames_of_the_square_against_hand_values():
    from monogs_amd.mesh_render import render_mesh_frame_numpy
    v, f, view = R.case_square()
    bg = (51, 102, 255)
    inside, outside = (8, 7), (1, 1)                             # (row, column)
    want = {"shaded": (255, 255, 255),                           # head-on: I = 0.25 + 0.75 = 1
            "normal": (127, 127, 0),                             # (0, 0, -1) towards the camera: 0.5, 0.5, 0
            "depth": (127, 0, 0)}                                # every depth is the largest: the top of the jet map
    for mode, rgb in want.items():
        frame = render_mesh_frame_numpy(v, f, view, mode, background=N.BACKGROUND)
        assert frame.dtype == np.uint8 and frame.shape == (16, 16, 3)
        assert tuple(frame[inside]) == rgb and tuple(frame[outside]) == bg, mode
        covered = (frame != np.array(bg, np.uint8)).any(axis=2)
        assert covered.sum() == 81 and covered[4:13, 3:12].all()                 # the 9 x 9 pixel centres of the square
    # the two windings give the same shade and, turned to the camera, the same normal colour
    back = render_mesh_frame_numpy(v, f[:, ::-1], view, "normal", background=N.BACKGROUND)
    assert np.array_equal(back, render_mesh_frame_numpy(v, f, view, "normal", background=N.BACKGROUND))
    # colours: the corners are ON pixel centres and get their own colour, the centre the mean of the diagonal's ends
    col = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    frame = render_mesh_frame_numpy(v, f, view, "color", colors=col, background=N.BACKGROUND)
    assert tuple(frame[4, 3]) == (255, 0, 0) and tuple(frame[4, 11]) == (0, 255, 0) and tuple(frame[12, 11]) == (0, 0, 255)
    assert tuple(frame[12, 3]) == (255, 255, 255) and tuple(frame[8, 7]) == (127, 0, 127) and tuple(frame[outside]) == bg
    u8 = render_mesh_frame_numpy(v, f, view, "color", colors=(col * 255).astype(np.uint8), background=N.BACKGROUND)
    assert np.array_equal(u8, frame)
    with pytest.raises(ValueError):
        render_mesh_frame_numpy(v, f, view, "color")
    with pytest.raises(ValueError):
        render_mesh_frame_numpy(v, f, view, "flat")


def test_colour_frame_weights_sum_to_one():
    from monogs_amd.mesh_render import render_mesh_frame_numpy
    view = R.SQUARE_VIEW
    v, f = R.from_pixels([(1.5, 2.25, 1.0), (14.25, 4.5, 3.0), (5.75, 13.5, 2.0)], view)
    frame = render_mesh_frame_numpy(v, f, view, "color", colors=np.eye(3, dtype=np.float32))
    inside = frame.any(axis=2)
    assert inside.sum() > 40
    total = frame.astype(np.int64).sum(axis=2)[inside]
    assert total.min() >= 253 and total.max() <= 257


def test_frames_of_empty_and_odd_meshes():
    bg = np.array((51, 102, 255), np.uint8)
    for mode in ("shaded", "normal", "color", "depth"):
        assert (N.mirror_frame("empty_all", mode) == bg).all()
        frame = N.mirror_frame("bad_index", mode)
        assert frame.shape == (16, 16, 3) and (frame != bg).any() and (frame == bg).all(axis=2).any()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    for fn in (L.mgs_face_normals, L.mgs_vertex_normals, L.mgs_mesh_eval_normal_stats, L.mgs_mesh_eval_normal_finish,
               L.mgs_mesh_shade):
        assert fn(None, None) == -1
    assert L.mgs_vertex_normals_scratch_bytes(-1) == 0 and L.mgs_vertex_normals_scratch_bytes(_cabi.MESH_EVAL_MAX_ITEMS + 1) == 0
    assert L.mgs_vertex_normals_scratch_bytes(0) > 0 and L.mgs_mesh_eval_normal_scratch_bytes() > 0
    a = _cabi.MeshNormalsArgs()
    a.num_verts, a.num_faces = 10, 4
    assert L.mgs_face_normals(C.byref(a), None) == -1                        # null arrays
    a.verts = a.faces = a.normals = a.record = 4096
    assert L.mgs_vertex_normals(C.byref(a), None) == -1                      # no scratch
    for V, F in ((-1, 4), (10, -1)):
        a.num_verts, a.num_faces = V, F
        assert L.mgs_face_normals(C.byref(a), None) == -1
    a.num_verts, a.num_faces, a.record = 10, 4, None
    assert L.mgs_face_normals(C.byref(a), None) == -1
    a.record, a.num_faces = 4096, _cabi.MESH_EVAL_MAX_ITEMS + 1
    assert L.mgs_face_normals(C.byref(a), None) == -3                        # MGS_ERR_UNSUPPORTED
    e = _cabi.MeshEvalNormalArgs()
    e.num, e.num_ref, e.num_faces, e.num_ref_faces = 8, 8, 2, 2
    assert L.mgs_mesh_eval_normal_stats(C.byref(e), None) == -1              # no scratch
    e.scratch = 4096
    assert L.mgs_mesh_eval_normal_stats(C.byref(e), None) == -1              # null arrays
    assert L.mgs_mesh_eval_normal_finish(C.byref(e), None) == -1             # no record
    e.d2 = e.index = e.face = e.ref_face = e.normals = e.ref_normals = 4096
    for field, value in (("num", -1), ("num_ref", -1), ("direction", 2), ("direction", -1)):
        old = getattr(e, field)
        setattr(e, field, value)
        assert L.mgs_mesh_eval_normal_stats(C.byref(e), None) == -1, field
        setattr(e, field, old)
    s = _cabi.MeshShadeArgs()
    s.num_verts, s.num_faces, s.width, s.height = 4, 2, 16, 16
    s.fx = s.fy = 16.0
    assert L.mgs_mesh_shade(C.byref(s), None) == -1                          # null planes
    s.face_id = s.out = 4096
    assert L.mgs_mesh_shade(C.byref(s), None) == -1                          # shaded without a pose and normals
    s.T = 4096
    assert L.mgs_mesh_shade(C.byref(s), None) == -1                          # ... without normals
    s.face_normal, s.mode = 4096, _cabi.MESH_SHADE_COLOR
    assert L.mgs_mesh_shade(C.byref(s), None) == -1                          # colour without colours
    s.mode = 4
    assert L.mgs_mesh_shade(C.byref(s), None) == -1
    s.mode = _cabi.MESH_SHADE_SHADED
    for w, h in ((0, 16), (16, -1)):
        s.width, s.height = w, h
        assert L.mgs_mesh_shade(C.byref(s), None) == -1
    s.width, s.height = 32768, 32768
    assert L.mgs_mesh_shade(C.byref(s), None) == -3                          # 3 H W >= 2^31
    s.width, s.height, s.fx = 16, 16, float("nan")
    assert L.mgs_mesh_shade(C.byref(s), None) == -1


def test_off_the_gpu_the_device_functions_raise():
    from monogs_amd.mesh_normals import face_normals, vertex_normals
    from monogs_amd.mesh_render import render_mesh_frame
    v, f, view = R.case_square()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for call in (lambda: face_normals(tv, tf), lambda: vertex_normals(tv, tf), lambda: render_mesh_frame(tv, tf, view)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
