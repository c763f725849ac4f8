"""Mesh normals on the device against their mirrors: face and vertex normals bit for bit, the normal-consistency record,
frames of a mesh byte for byte, and save_mesh with normals, a preview and the new scores.

evaluate_mesh(normals=True) without `cull` makes one device-to-host copy, of the record's twenty doubles; nothing here
counts copies (the existing tests of the one host read do not either)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_eval_cases as K
import mesh_normal_cases as N
import mesh_render_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The scratch buffers the drivers keep between calls, and the allocator's cached blocks, go back to the device when
    this module is done: later modules meet the memory they met before this one existed."""
    yield
    from monogs_amd import _device
    for kind in ("vertex_normals", "normal_stats"):
        _device._scratch.pop(kind, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) for a in arrays)


def floater_volume(big_only=False):
    from monogs_amd.tsdf import TSDFVolume
    vol = TSDFVolume(MC.FLOATER_ORIGIN, MC.FLOATER_VOXEL, MC.FLOATER_DIMS, device=_dev())
    for dst, src in zip((vol.tsdf, vol.weight, vol.color), MC.floater_planes(big_only)):
        dst.copy_(torch.from_numpy(src))
    return vol


# ---- face normals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.FACE_CASES + tuple(f"soup{F}" for F in N.SOUP_SIZES))
def test_face_normals_equal_the_mirror_bit_for_bit(built, name):
    from monogs_amd.mesh_normals import face_normals, face_normals_numpy
    v, f = N.soup(int(name[4:])) if name.startswith("soup") else K.sampler_mesh(name)
    want, wrec = face_normals_numpy(v, f)
    dv, df = to_dev(v, f)
    got, rec = face_normals(dv, df)
    assert got.dtype == torch.float32 and tuple(got.shape) == (f.shape[0], 3) and rec.dtype == torch.int32
    assert rec.cpu().tolist() == wrec.tolist()
    assert np.array_equal(bits(got), want.view(np.int32))
    if name == "bad_index":
        assert wrec.tolist() == [2, 0]
    if name == "degenerate":
        assert wrec.tolist() == [0, 44]
    again, arec = face_normals(dv, df)                           # two calls, the same bytes
    assert np.array_equal(bits(again), bits(got)) and torch.equal(arec, rec)


# ---- vertex normals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["star", "strip", "sphere", "special", "bad_index", "no_faces", "degenerate", "extraction",
                                  "two_trips"])
def test_vertex_normals_equal_the_mirror_bit_for_bit(built, name):
    """The second call's bytes equal the first's: the integer atomics make the sums free of the order of arrival -
    `star` puts 3000 faces on one accumulator."""
    from monogs_amd.mesh_normals import vertex_normals, vertex_normals_numpy
    if name == "extraction":
        dv, df, _ = floater_volume().extract_mesh()
        v, f = dv.cpu().numpy(), df.cpu().numpy()
        assert (v.shape[0], f.shape[0]) == MC.FLOATER_VF
    else:
        v, f = K.sampler_mesh(name) if name == "two_trips" else N.vertex_cases()[name]
        dv, df = to_dev(v, f)
    want, wrec = vertex_normals_numpy(v, f)
    got, rec = vertex_normals(dv, df)
    assert got.dtype == torch.float32 and tuple(got.shape) == (v.shape[0], 3)
    assert rec.cpu().tolist() == wrec.tolist()
    assert np.array_equal(bits(got), want.view(np.int32))
    if name == "star":
        assert want[7].any()
    if name == "special":
        assert [row.any() for row in want] == [e is not None for e in N.special()[2]]
    if name == "no_faces":
        assert v.shape[0] == 5 and not want.any()
    again, arec = vertex_normals(dv, df)                         # two calls, the same bytes
    assert np.array_equal(bits(again), bits(got)) and torch.equal(arec, rec)


# ---- normal consistency ------------------------------------------------------------------------------------------------
def _assert_normal_scores(got, rec, want, wrec, n):
    from monogs_amd.mesh_eval import METRIC_KEYS, NORMAL_KEYS
    assert tuple(got)[:len(METRIC_KEYS) + len(NORMAL_KEYS)] == METRIC_KEYS + NORMAL_KEYS and rec.shape == wrec.shape == (20,)
    for d in range(2):
        assert tuple(rec[4 * d:4 * d + 3]) == tuple(wrec[4 * d:4 * d + 3])               # counts and maximum: exact
        assert abs(rec[4 * d + 3] - wrec[4 * d + 3]) <= n * 2.0 ** -53 * wrec[4 * d + 3]
        pairs, total, flipped, skipped = rec[12 + 4 * d:16 + 4 * d]
        print(f"direction {d}: pairs {pairs:.0f} sum |t| {float(total)!r} (mirror {float(wrec[13 + 4 * d])!r}) "
              f"flipped {flipped:.0f} skipped {skipped:.0f}")
        assert (pairs, flipped, skipped) == (wrec[12 + 4 * d], wrec[14 + 4 * d], wrec[15 + 4 * d])
        assert abs(total - wrec[13 + 4 * d]) <= n * 2.0 ** -53 * wrec[13 + 4 * d]
    assert tuple(rec[8:12]) == tuple(wrec[8:12])
    for k in ("normal_flipped", "normal_skipped"):
        assert got[k] == want[k], k
    for k in ("normal_accuracy", "normal_completion", "normal_consistency"):
        assert abs(got[k] - want[k]) <= 1e-12 * want[k], k


def _assert_old_record(rec, old, n):
    """The first twelve doubles against the normals=False record of the same call."""
    assert old.shape == (12,)
    for d in range(2):
        assert tuple(rec[4 * d:4 * d + 3]) == tuple(old[4 * d:4 * d + 3])
        assert abs(rec[4 * d + 3] - old[4 * d + 3]) <= n * 2.0 ** -53 * old[4 * d + 3]
    assert tuple(rec[8:12]) == tuple(old[8:12])


@pytest.mark.parametrize("name", ["spheres", "flipped", "box"])
def test_evaluate_mesh_normals_on_the_three_scenes(built, name):
    from monogs_amd.mesh_eval import METRIC_KEYS, evaluate_mesh
    pred, gt = (to_dev(*m) for m in N.eval_scenes()[name])
    kw = dict(n_samples=N.EVAL_SAMPLES, threshold=0.05, seed=N.EVAL_SEED, with_record=True)
    got, rec = evaluate_mesh(pred, gt, normals=True, **kw)
    want, wrec = N.mirror_scores(name)
    _assert_normal_scores(got, rec, want, wrec, N.EVAL_SAMPLES)
    old, orec = evaluate_mesh(pred, gt, **kw)
    assert tuple(old) == METRIC_KEYS
    _assert_old_record(rec, orec, N.EVAL_SAMPLES)
    if name == "spheres":
        assert got["normal_consistency"] > 0.99 and got["normal_flipped"] == 0 and got["normal_skipped"] == 0
    if name == "flipped":
        assert got["normal_flipped"] == 1.0 and got["normal_consistency"] > 0.99
    if name == "box":
        assert got["normal_consistency"] < 0.8
    with pytest.raises(ValueError, match="normals=True"):
        evaluate_mesh(pred, gt[0], n_samples=64, normals=True)               # a point tensor as ground truth


def test_evaluate_mesh_normals_on_the_floater_extractions(built):
    from monogs_amd.mesh_eval import evaluate_mesh, evaluate_mesh_numpy
    gv, gf, _ = floater_volume(big_only=True).extract_mesh()
    vol = floater_volume()
    thr = 0.5 * MC.FLOATER_VOXEL
    kw = dict(n_samples=4099, threshold=thr, seed=3, with_record=True)
    for clean in (None, dict(keep_largest=1)):
        v, f, _ = vol.extract_mesh() if clean is None else vol.extract_mesh(clean=clean)
        got, rec = evaluate_mesh((v, f), (gv, gf), normals=True, **kw)
        want, wrec = evaluate_mesh_numpy((v.cpu().numpy(), f.cpu().numpy()), (gv.cpu().numpy(), gf.cpu().numpy()),
                                         normals=True, **kw)
        _assert_normal_scores(got, rec, want, wrec, 4099)
        _assert_old_record(rec, evaluate_mesh((v, f), (gv, gf), **kw)[1], 4099)
        assert got["normal_flipped"] < 0.05                      # both extractions are wound by the same table
        if clean is not None:
            assert got["normal_consistency"] > 0.99 and got["normal_flipped"] == 0
        again = evaluate_mesh((v, f), (gv, gf), normals=True, **kw)
        assert again[0] == got and np.array_equal(again[1].view(np.int64), rec.view(np.int64))       # the same bytes


def test_evaluate_mesh_normals_with_cull(built):
    from monogs_amd.mesh_eval import METRIC_KEYS, NORMAL_KEYS, evaluate_mesh, evaluate_mesh_numpy
    pred, gt, views = R.hidden_sphere()
    kw = dict(n_samples=R.SPHERE_SAMPLES, threshold=R.SPHERE_THRESHOLD, seed=0, cull=dict(views=views), normals=True,
              with_record=True)
    got, rec = evaluate_mesh(to_dev(*pred), to_dev(*gt), **kw)
    want, wrec = evaluate_mesh_numpy(pred, gt, **kw)
    assert tuple(got) == METRIC_KEYS + NORMAL_KEYS + ("culled_pred_faces", "culled_gt_faces") == tuple(want)
    assert (got["culled_pred_faces"], got["culled_gt_faces"]) == (want["culled_pred_faces"], want["culled_gt_faces"])
    assert got["culled_pred_faces"] >= 224                       # the hidden inner sphere is gone
    _assert_normal_scores(got, rec, want, wrec, R.SPHERE_SAMPLES)


# ---- frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shaded", "normal", "color", "color_u8", "depth"])
@pytest.mark.parametrize("name", N.FRAME_CASES)
def test_render_mesh_frame_equals_the_mirror_byte_for_byte(built, name, mode):
    from monogs_amd.mesh_render import render_mesh_frame
    v, f, view = R.render_case(name)
    u8 = mode == "color_u8"
    mode = "color" if u8 else mode
    want = N.mirror_frame(name, mode, u8)
    dv, df = to_dev(v, f)
    colors = to_dev(N.frame_colors(v.shape[0], u8))[0] if mode == "color" else None
    got = render_mesh_frame(dv, df, view, mode, colors=colors, background=N.BACKGROUND)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    diff = np.argwhere(got.cpu().numpy() != want)
    assert diff.size == 0, (len(diff), diff[:4])
    if name == "large33":
        assert R.mirror_render(name)[2][2] == 33                 # every face on the large-face path
    assert torch.equal(render_mesh_frame(dv, df, view, mode, colors=colors, background=N.BACKGROUND), got)


def test_render_mesh_frame_of_one_pixel_and_bad_arguments(built):
    from monogs_amd.mesh_render import render_mesh_frame, render_mesh_frame_numpy
    v, f, _ = R.case_square()
    view = (np.eye(4, dtype=np.float32), 16.0, 16.0, 1.0, 0.0, 1, 1)         # pixel (0,0) lies inside the square
    dv, df = to_dev(v, f)
    col = N.frame_colors(4)
    for mode in ("shaded", "normal", "color", "depth"):
        want = render_mesh_frame_numpy(v, f, view, mode, colors=col, background=N.BACKGROUND)
        got = render_mesh_frame(dv, df, view, mode, colors=to_dev(col)[0], background=N.BACKGROUND)
        assert tuple(got.shape) == (1, 1, 3) and np.array_equal(got.cpu().numpy(), want)
        assert tuple(want[0, 0]) != (51, 102, 255)
    with pytest.raises(ValueError):
        render_mesh_frame(dv, df, view, "color")
    with pytest.raises(ValueError):
        render_mesh_frame(dv, df, view, "color", colors=to_dev(col[:3])[0])
    with pytest.raises(ValueError):
        render_mesh_frame(dv, df, view, "wireframe")


def test_normal_frame_of_a_head_on_wall_is_the_viewers(built):
    """The mesh renderer centres pixel (x, y) at u = x, v = y: pixel_center = 0, what depth_normal_torch documents for
    planes that are not this rasteriser's."""
    from monogs_amd.mesh_render import render_mesh_depth, render_mesh_frame
    from monogs_amd.surface import depth_normal_torch, normal_rgb_torch
    from monogs_amd.viewer import compose_torch
    v, f, view = R.case_square()
    T, fx, fy, cx, cy, H, W = view
    dv, df = to_dev(v, f)
    frame = render_mesh_frame(dv, df, view, "normal").cpu().numpy().astype(np.int64)
    depth = render_mesh_depth(dv, df, T, fx, fy, cx, cy, H, W)[0]
    viewer = compose_torch(normal_rgb_torch(depth_normal_torch(depth, fx, fy, cx, cy, pixel_center=0.0)), "rgb")
    viewer = viewer.cpu().numpy().astype(np.int64)
    x0, y0, x1, y1 = R.SQUARE_CORNERS
    inner = (slice(y0 + 1, y1), slice(x0 + 1, x1))               # a valid depth on all four sides
    assert tuple(frame[8, 7]) == (127, 127, 0)
    assert np.abs(frame[inner] - viewer[inner]).max() <= 1
    assert (viewer[inner] == np.array([127, 127, 0])).all()


# ---- save_mesh ---------------------------------------------------------------------------------------------------------
def test_save_mesh_with_normals_preview_and_scores(built, tmp_path):
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_eval import METRIC_KEYS, NORMAL_KEYS
    from monogs_amd.mesh_normals import vertex_normals
    from monogs_amd.ply_io import read_mesh_ply, write_mesh_ply
    vol = floater_volume()
    gt = floater_volume(big_only=True).extract_mesh()[:2]
    view = R._floater_view(0.0)
    clean = dict(keep_largest=1)
    scores = save_mesh(vol, str(tmp_path / "full"), clean=clean, gt=gt, normals=True, preview=view,
                       eval_kw=dict(n_samples=4099, threshold=0.5, seed=3, normals=True))
    folder = os.path.join(str(tmp_path / "full"), "point_cloud", "final")
    assert tuple(scores) == METRIC_KEYS + NORMAL_KEYS and scores["normal_consistency"] > 0.99
    with open(os.path.join(folder, "mesh_eval.json"), encoding="utf-8") as fh:
        assert json.load(fh) == scores
    pv, pf, pc, pn = read_mesh_ply(os.path.join(folder, "mesh.ply"), with_normals=True)
    v, f, _ = vol.extract_mesh(clean=clean)
    assert np.array_equal(bits(pv), bits(v)) and torch.equal(pf, f.cpu())
    assert np.array_equal(bits(pn), bits(vertex_normals(v, f)[0])) and bool(pn.any(dim=1).all())
    names = sorted(os.listdir(folder))
    preview = [n for n in names if n.startswith("mesh_preview.")]
    assert names == sorted(["mesh.ply", "mesh_eval.json"] + preview) and preview in (["mesh_preview.png"], ["mesh_preview.ppm"])
    H, W = view[5], view[6]
    if preview[0].endswith(".ppm"):
        blob = open(os.path.join(folder, preview[0]), "rb").read()
        head = b"P6\n%d %d\n255\n" % (W, H)
        assert blob.startswith(head) and len(blob) == len(head) + 3 * H * W
    else:
        from PIL import Image
        assert Image.open(os.path.join(folder, preview[0])).size == (W, H)
    # the defaults: the folder a call without the new keywords leaves, byte for byte
    plain = save_mesh(vol, str(tmp_path / "plain"), clean=clean)
    explicit = save_mesh(vol, str(tmp_path / "explicit"), clean=clean, normals=False, preview=None)
    write_mesh_ply(str(tmp_path / "direct.ply"), *vol.extract_mesh(clean=clean))
    want = open(str(tmp_path / "direct.ply"), "rb").read()
    for path in (plain, explicit):
        assert os.listdir(os.path.dirname(path)) == ["mesh.ply"] and open(path, "rb").read() == want
