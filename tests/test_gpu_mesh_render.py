"""Mesh rendering and culling on the device against the mirrors (monogs_amd/mesh_render.py): depth, face ids and the record
bit for bit and twice - the contract is order-free, so nothing is tolerated -, both paths of the render against each
other, visibility counts and culled meshes bit for bit, and the protocol through evaluate_mesh and its callers.

Sizes: mesh_render_cases.py lists the block and path boundaries and the case that crosses each."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_render_cases as RC

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def device_case(name):
    v, f, view = RC.render_case(name)
    return torch.from_numpy(v).to(_dev()), torch.from_numpy(f).to(_dev()), view


def device_mesh(mesh):
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(_dev()) for t in mesh)


def render(name, **kw):
    from monogs_amd.mesh_render import render_mesh_depth
    v, f, (T, fx, fy, cx, cy, H, W) = device_case(name)
    return render_mesh_depth(v, f, T, fx, fy, cx, cy, H, W, **kw)


def assert_planes(got, want, record=True):
    depth, face, rec = got
    assert np.array_equal(bits(depth), want[0].view(np.int32))
    assert np.array_equal(face.cpu().numpy(), want[1])
    if record:
        assert rec.cpu().tolist() == want[2].tolist()


# ---- render_mesh_depth -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RC.RENDER_CASES))
def test_render_equals_the_mirror_bit_for_bit(built, name):
    want = RC.mirror_render(name)
    got = render(name)
    _, _, (_, _, _, _, _, H, W) = device_case(name)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    assert tuple(got[0].shape) == tuple(got[1].shape) == (H, W) and tuple(got[2].shape) == (4,)
    assert_planes(got, want)
    if name in RC.RECORDS:
        assert tuple(got[2].cpu().tolist()) == RC.RECORDS[name]
    again = render(name)                                                # two calls, the same bytes
    assert np.array_equal(bits(again[0]), bits(got[0])) and torch.equal(again[1], got[1]) and torch.equal(again[2], got[2])


@pytest.mark.parametrize("name", ["large_boxes", "large33", "box_inside", "floaters_a", "snap_limit"])
def test_both_paths_write_the_same_keys(built, name):
    """Every face down the lane path (threshold above H W), every face down the workgroup path (threshold 0), and the
    default split: the same planes, and record[2] the number of faces the mirror sends down the large path."""
    want = RC.mirror_render(name)
    _, _, (_, _, _, _, _, H, W) = device_case(name)
    for thr in (1024, 0, H * W + 1):
        got = render(name, large_threshold=thr)
        assert_planes(got, want, record=False)
        rec = got[2].cpu().tolist()
        assert rec == RC.mirror_render(name, large_threshold=thr)[2].tolist()
        if name == "large_boxes":
            assert rec[2] == {1024: 2, 0: 3, H * W + 1: 0}[thr]
        if thr == H * W + 1:
            assert rec[2] == 0
    assert render(name, large_threshold=0)[2][2].item() > 0


@pytest.mark.parametrize("grid", [1, 8, 33, 256])
def test_large_launch_strides_its_list(built, grid):
    """33 large faces over 8 workgroups: five trips; 1003 faces, all large, over the same grids."""
    want = RC.mirror_render("large33")
    got = render("large33", large_grid=grid)
    assert_planes(got, want)
    assert got[2][2].item() == 33
    if grid <= 8:
        assert_planes(render("odd", large_threshold=0, large_grid=grid + 2), RC.mirror_render("odd"), record=False)


def test_render_refuses(built):
    from monogs_amd.mesh_render import render_mesh_depth
    v, f, (T, fx, fy, cx, cy, H, W) = device_case("square")
    with pytest.raises(ValueError):
        render_mesh_depth(v[:, :2], f, T, fx, fy, cx, cy, H, W)
    with pytest.raises(ValueError):
        render_mesh_depth(v, f.reshape(-1), T, fx, fy, cx, cy, H, W)
    with pytest.raises(ValueError):
        render_mesh_depth(v, f, T[:3], fx, fy, cx, cy, H, W)
    with pytest.raises(ValueError):
        render_mesh_depth(v, f, T, fx, fy, cx, cy, 0, W)
    with pytest.raises(ValueError):
        render_mesh_depth(v, f, T, fx, fy, cx, cy, 65536, 32768)
    with pytest.raises(ValueError):
        render_mesh_depth(v, f, T, fx, fy, cx, cy, H, W, large_threshold=-1)
    with pytest.raises(RuntimeError):
        render_mesh_depth(v.cpu(), f.cpu(), T, fx, fy, cx, cy, H, W)


# ---- vertex_visibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pillar_room", "odd", "behind_and_nan", "empty_all"])
def test_vertex_visibility_equals_the_mirror(built, name):
    from monogs_amd.mesh_render import vertex_visibility, vertex_visibility_torch
    v, f, (T, fx, fy, cx, cy, H, W) = device_case(name)
    hv = RC.render_case(name)[0]
    depth = render(name)[0]
    hdepth = RC.mirror_render(name)[0]
    zero = torch.zeros(H, W, device=_dev())
    for kw, hkw in ((dict(depth=depth), dict(depth=hdepth)), (dict(), dict()), (dict(depth=depth, eps=0.0), dict(depth=hdepth, eps=0.0)),
                    (dict(depth=zero, empty_visible=False), dict(depth=zero.cpu(), empty_visible=False)),
                    (dict(depth=depth, z_near=3.0), dict(depth=hdepth, z_near=3.0))):
        got = vertex_visibility(v, T, fx, fy, cx, cy, H, W, **kw)
        want = vertex_visibility_torch(hv, T, fx, fy, cx, cy, H, W, **hkw)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want.numpy())
    if name == "pillar_room":
        hidden, clear = RC.pillar_vertex_sets()
        seen = vertex_visibility(v, T, fx, fy, cx, cy, H, W, depth=depth)
        assert int(seen[torch.from_numpy(hidden).to(_dev())].sum()) == 0
        assert int(seen[torch.from_numpy(clear).to(_dev())].sum()) == len(clear)
        out = vertex_visibility(v, T, fx, fy, cx, cy, H, W, out=seen.clone())      # accumulates in place
        assert torch.equal(out, seen + vertex_visibility(v, T, fx, fy, cx, cy, H, W))
        with pytest.raises(ValueError):
            vertex_visibility(v, T, fx, fy, cx, cy, H, W, out=seen.to(torch.int64))
        with pytest.raises(ValueError):
            vertex_visibility(v, T, fx, fy, cx, cy, H, W, depth=depth[:-1])


# ---- cull_mesh -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", RC.CULL_PARAMS, ids=lambda p: f"{p[0]}-m{p[1]}-{p[2]}")
def test_cull_mesh_equals_the_mirror_bit_for_bit(built, param):
    from monogs_amd.mesh_render import cull_mesh, cull_mesh_numpy
    which, min_views, rule = param
    v, f, _ = device_case("pillar_room")
    hv, hf, _ = RC.render_case("pillar_room")
    seen = RC.seen_vectors(hv.shape[0])[which]
    col = np.random.default_rng(5).random(hv.shape).astype(np.float32)
    want = cull_mesh_numpy(hv, hf, col, seen_count=seen, min_views=min_views, rule=rule)
    dseen, dcol = torch.from_numpy(seen).to(_dev()), torch.from_numpy(col).to(_dev())
    for _ in range(2):                                                  # two calls, the same bytes
        gv, gf, gc, info = cull_mesh(v, f, dcol, seen_count=dseen, min_views=min_views, rule=rule)
        assert info == want[3]
        assert np.array_equal(bits(gv), want[0].view(np.int32)) and np.array_equal(bits(gc), want[2].view(np.int32))
        assert gf.dtype == torch.int32 and np.array_equal(gf.cpu().numpy(), want[1])
    if which == "none":
        assert info["verts_out"] == 0 and info["faces_out"] == 0
    if which == "every":
        assert info["verts_out"] == hv.shape[0] and info["faces_out"] == hf.shape[0]
    assert cull_mesh(v, f, None, seen_count=dseen, min_views=min_views, rule=rule)[2] is None


def test_cull_mesh_across_a_scan_trip(built):
    """V = 262 250 and F = 262 188 are 1025 block totals each: the one-workgroup scan takes a second trip, and kept
    vertices and faces lie on both sides of element 262 144, where it begins."""
    import mesh_clean_cases as MC
    from monogs_amd.mesh_render import cull_mesh, cull_mesh_numpy
    hv, col, hf = MC.two_scan_trips()
    V, F, trip = hv.shape[0], hf.shape[0], 1024 * 256
    assert (V, F) == (262250, 262188)
    seen = np.random.default_rng(0).integers(0, 3, V).astype(np.int32)
    dv, dc, dseen = (torch.from_numpy(t).to(_dev()) for t in (hv, col, seen))

    def check(faces, rule, min_views, calls):
        want = cull_mesh_numpy(hv, faces, col, seen_count=seen, min_views=min_views, rule=rule)
        df = torch.from_numpy(faces).to(_dev())
        for _ in range(calls):
            gv, gf, gc, info = cull_mesh(dv, df, dc, seen_count=dseen, min_views=min_views, rule=rule)
            assert info == want[3]
            assert np.array_equal(bits(gv), want[0].view(np.int32)) and np.array_equal(bits(gc), want[2].view(np.int32))
            assert gf.dtype == torch.int32 and np.array_equal(gf.cpu().numpy(), want[1])
        return want[3]

    for rule, min_views in (("all", 1), ("any", 2)):
        info = check(hf, rule, min_views, 2)                            # two calls, the same bytes
        ok = (seen >= min_views)[hf]                                    # the mirror's flags, held to its counts
        fkeep = ok.any(axis=1) if rule == "any" else ok.all(axis=1)
        vkeep = np.zeros(V, bool)
        vkeep[hf[fkeep].reshape(-1)] = True
        assert (int(fkeep.sum()), int(vkeep.sum())) == (info["faces_out"], info["verts_out"])
        assert fkeep[trip:].sum() >= 10 and vkeep[trip:].sum() >= 30
        assert fkeep[:trip].sum() >= 10 and vkeep[:trip].sum() >= 30
    bad = hf.copy()
    bad[7, 0] = bad[262150, 1] = V                                      # one bad face on each side of the trip boundary
    assert check(bad, "any", 2, 1)["bad_faces"] == 2


def test_cull_mesh_edges(built):
    from monogs_amd.mesh_render import cull_mesh, cull_mesh_numpy
    dev = _dev()
    v, f, _ = device_case("bad_index")                                  # an index V and an index -1: dropped and counted
    hv, hf, _ = RC.render_case("bad_index")
    seen = torch.ones(v.shape[0], dtype=torch.int32, device=dev)
    gv, gf, _, info = cull_mesh(v, f, seen_count=seen)
    want = cull_mesh_numpy(hv, hf, seen_count=seen.cpu().numpy())
    assert info == want[3] and info["bad_faces"] == 2 and info["faces_out"] == 1
    assert np.array_equal(bits(gv), want[0].view(np.int32)) and np.array_equal(gf.cpu().numpy(), want[1])
    for V, F in ((0, 0), (5, 0)):
        ev, ef = torch.zeros(V, 3, device=dev), torch.zeros(F, 3, dtype=torch.int32, device=dev)
        out = cull_mesh(ev, ef, seen_count=torch.ones(V, dtype=torch.int32, device=dev))
        assert out[3] == dict(verts_in=V, faces_in=F, verts_out=0, faces_out=0, bad_faces=0)
        assert tuple(out[0].shape) == (0, 3) and tuple(out[1].shape) == (0, 3)
    with pytest.raises(ValueError):
        cull_mesh(v, f, seen_count=seen, rule="most")
    with pytest.raises(ValueError):
        cull_mesh(v, f, seen_count=seen[:-1])


# ---- the protocol ----------------------------------------------------------------------------------------------------
def test_cull_by_visibility_and_depth_l1_equal_the_mirrors(built):
    from monogs_amd.mesh_render import (cull_by_visibility, cull_by_visibility_numpy, mesh_depth_l1, mesh_depth_l1_numpy)
    pred, gt, views = RC.hidden_sphere()
    dpred, dgt = device_mesh(pred), device_mesh(gt)
    for kw in (dict(), dict(occluder=None), dict(rule="any", min_views=2)):
        gv, gf, _, info = cull_by_visibility(dpred, views, **kw)
        want = cull_by_visibility_numpy(pred, views, **kw)
        assert info == want[3]
        assert np.array_equal(bits(gv), want[0].view(np.int32)) and np.array_equal(gf.cpu().numpy(), want[1])
    gv, gf, _, info = cull_by_visibility(dpred, views, occluder=dgt)
    assert info == cull_by_visibility_numpy(pred, views, occluder=gt)[3] and info["faces_out"] == gt[1].shape[0]
    shift = (1.0, np.eye(3), (0.02, 0.0, 0.0))
    got, want = mesh_depth_l1(dpred, dgt, views, transform=shift), mesh_depth_l1_numpy(pred, gt, views, transform=shift)
    assert got[1] == want[1] > 0 and abs(got[0] - want[0]) <= 1e-12 * want[0] and 0.0 < got[0] < 0.02


@functools.lru_cache(maxsize=None)
def _hidden_sphere_scores():
    """The device and the mirror at 20 000 samples (the mirror's brute force is computed once)."""
    from monogs_amd.mesh_eval import evaluate_mesh, evaluate_mesh_numpy
    pred, gt, views = RC.hidden_sphere()
    kw = dict(n_samples=20000, threshold=RC.SPHERE_THRESHOLD, seed=0, with_record=True,
              cull=dict(views=views, occlusion="self"))
    return evaluate_mesh(device_mesh(pred), device_mesh(gt), **kw), evaluate_mesh_numpy(pred, gt, **kw)


def test_evaluate_mesh_with_cull_equals_the_mirror(built):
    from monogs_amd.mesh_eval import METRIC_KEYS
    (got, rec), (want, wrec) = _hidden_sphere_scores()
    assert tuple(got) == METRIC_KEYS + ("culled_pred_faces", "culled_gt_faces")
    for d in range(2):
        assert tuple(rec[4 * d:4 * d + 3]) == tuple(wrec[4 * d:4 * d + 3])           # counts and maximum: exact
        assert abs(rec[4 * d + 3] - wrec[4 * d + 3]) <= 20000 * 2.0 ** -53 * wrec[4 * d + 3]
    assert tuple(rec[8:]) == tuple(wrec[8:]) == (0.0, 0.0, 0.0, 0.0)
    for k in ("precision", "recall", "completion_ratio", "f_score", "hausdorff", "n_pred", "n_gt", "bad_faces",
              "culled_pred_faces", "culled_gt_faces"):
        assert got[k] == want[k], k
    for k in ("accuracy", "completion", "chamfer"):
        assert abs(got[k] - want[k]) <= 1e-12 * want[k], k


def test_hidden_sphere_and_far_hemisphere_on_the_device(built):
    from monogs_amd.mesh_eval import METRIC_KEYS, evaluate_mesh
    kw = dict(n_samples=RC.SPHERE_SAMPLES, threshold=RC.SPHERE_THRESHOLD, seed=0)
    pred, gt, views = RC.hidden_sphere()
    dpred, dgt = device_mesh(pred), device_mesh(gt)
    raw = evaluate_mesh(dpred, dgt, **kw)
    assert tuple(raw) == METRIC_KEYS                                    # cull=None: exactly today's keys
    assert raw["precision"] < 0.9 and raw["recall"] == 1.0
    for occlusion in ("self", "gt"):
        out = evaluate_mesh(dpred, dgt, cull=dict(views=views, occlusion=occlusion), **kw)
        assert out["precision"] == 1.0 and out["recall"] == 1.0
        assert out["culled_pred_faces"] == 224 and out["culled_gt_faces"] == 0
    assert evaluate_mesh(dpred, dgt, cull=dict(views=views, occlusion=None), **kw)["culled_pred_faces"] == 0
    big = _hidden_sphere_scores()[0][0]
    assert big["precision"] == 1.0 and big["recall"] == 1.0 and big["culled_pred_faces"] == 224
    pred, gt, views = RC.far_hemisphere()
    dpred, dgt = device_mesh(pred), device_mesh(gt)
    raw = evaluate_mesh(dpred, dgt, **kw)
    out = evaluate_mesh(dpred, dgt, cull=dict(views=views, occlusion="self"), **kw)
    print(f"far hemisphere: recall {raw['recall']:.4f} -> {out['recall']:.4f}, gt faces culled {out['culled_gt_faces']}")
    assert raw["recall"] < 0.9 and out["recall"] == 1.0 and out["precision"] == 1.0
    assert out["culled_gt_faces"] == 326 and out["culled_pred_faces"] == 0
    with pytest.raises(ValueError, match="views"):
        evaluate_mesh(dpred, dgt, cull=dict(occlusion="gt"), **kw)
    with pytest.raises(ValueError, match="mesh"):
        evaluate_mesh(dpred, dgt[0], cull=dict(views=views), **kw)


def test_run_evaluation_and_save_mesh_with_cull(built, tmp_path):
    """The surrogate run of test_gpu_mesh_eval.py::test_save_mesh_and_run_evaluation, its ground truth in a frame that is
    a known Sim(3) of the run's, with ground-truth poses that look at it."""
    from scenes import wide_scene
    from monogs_amd import slam_surrogate
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_eval import METRIC_KEYS, apply_transform
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, ViewCamera
    dev = _dev()
    sc = wide_scene()
    cam = sc.cam
    gm = GaussianParams(*(t.to(dev) for t in (sc.means3D, sc.log_scales, sc.rot, sc.opacity_logit, sc.features_dc)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    taus = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.1, -0.05, 0.08, 0.03, -0.02, 0.01],
                         [-0.12, 0.07, 0.02, -0.02, 0.03, 0.0], [0.04, 0.11, -0.06, 0.01, 0.0, -0.03],
                         [-0.03, -0.09, 0.12, 0.0, 0.02, 0.02]])
    cams = [ViewCamera(k, torch.zeros(3, cam.H, cam.W), SE3_exp(tau), cam.projmatrix_raw, fovx, fovy, cam.H, cam.W, dev)
            for k, tau in enumerate(taus)]
    vs = 0.125
    result = {"cameras": {k: v for k, v in enumerate(cams)}, "kf_ids": [0, 1, 2, 3, 4], "gaussians": gm}
    raw = slam_surrogate.reconstruct_mesh(result, vs)
    c, t = 1.7, torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64)
    R = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    for v in cams:                                                      # x_g = c R x_w + t: the pose that sees c times the depth
        Tw = v.T.double().cpu()
        T_gt = torch.eye(4, dtype=torch.float64)
        T_gt[:3, :3] = Tw[:3, :3] @ R.T
        T_gt[:3, 3] = c * Tw[:3, 3] - T_gt[:3, :3] @ t
        v.T_gt = T_gt
    gt = (apply_transform(raw[0], (c, R, t)), raw[1])
    kw = dict(n_samples=20000, threshold=c * vs)
    plain = slam_surrogate.evaluate_mesh(result, gt, vs, monocular=True, **kw)
    assert tuple(plain) == METRIC_KEYS
    out = slam_surrogate.evaluate_mesh(result, gt, vs, monocular=True, cull=True, **kw)
    F = int(raw[1].shape[0])
    print(f"surrogate run: {F} faces, culled pred {out['culled_pred_faces']}, gt {out['culled_gt_faces']}, "
          f"f-score {plain['f_score']:.4f} -> {out['f_score']:.4f}")
    assert tuple(out) == METRIC_KEYS + ("culled_pred_faces", "culled_gt_faces")
    assert 0 <= out["culled_pred_faces"] < F and 0 <= out["culled_gt_faces"] < F and out["f_score"] > 0.99
    own = slam_surrogate.evaluate_mesh(result, gt, vs, monocular=True, cull=dict(occlusion=None, rule="any"), **kw)
    assert own["culled_gt_faces"] <= out["culled_gt_faces"]            # the frustum alone drops no more than the depth test
    # save_mesh passes the protocol on and writes the counts
    T_run = [(v.T, v.fx, v.fy, v.cx, v.cy, v.image_height, v.image_width) for v in cams]
    scores = save_mesh(gm, str(tmp_path / "culled"), cameras=cams, voxel_size=vs, gt=(raw[0], raw[1]),
                       eval_kw=dict(n_samples=20000, threshold=vs), cull=dict(views=T_run, occlusion="gt"))
    with open(os.path.join(str(tmp_path / "culled"), "point_cloud", "final", "mesh_eval.json"), encoding="utf-8") as fh:
        written = json.load(fh)
    assert written == scores and "culled_pred_faces" in written and "culled_gt_faces" in written
    assert scores["culled_pred_faces"] == scores["culled_gt_faces"] and scores["f_score"] > 0.99      # the same mesh twice
