"""mgs_remap_build and mgs_frame_prepare_remapped (frame_prepare.hip) on the MI355X: the map against the fp64 NumPy
mirror entry for entry, the remapped call against the un-remapped one (identity map), against the torch mirror with real
distortion at the tile boundaries, against hand arithmetic (the shift case), the two depth modes, determinism, the
argument errors, and the Python plumbing (FramePreparer(config=...), prepare_into, run_sequence).  The comparison rule
is test_cpu_frame_prepare.compare's."""
import ctypes as C

import numpy as np
import pytest
import torch

from monogs_amd import _cabi
from monogs_amd import frame_prepare as FP
from test_cpu_frame_prepare import compare
import remap_cases as RC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("image", "grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping", "median", "intensity")


def config(dataset_type, edge_threshold=1.1, calibration=None):
    ds = {"type": dataset_type}
    if calibration is not None:
        ds["Calibration"] = calibration
    return {"Training": {"edge_threshold": edge_threshold, "rgb_boundary_threshold": 0.01}, "Dataset": ds}


def snapshot(res):
    return {k: res[k].clone() for k in KEYS + ("gt_depth",) if res.get(k) is not None}


def same_bits(a, b, keys=KEYS):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)


def identity_map(H, W):
    u, v = np.meshgrid(np.arange(W, dtype=np.int32), np.arange(H, dtype=np.int32))
    return torch.from_numpy(np.ascontiguousarray(np.stack([32 * u, 32 * v], axis=-1)))


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


# ---- 6: the map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (33, 35), (45, 70)])
def test_remap_build_equals_the_numpy_mirror(built, H, W):
    cal = RC.calibration_for(H, W)
    K = RC.intrinsics(cal)
    P = FP.FramePreparer(H, W, DEV, config("tum"))
    assert P.map_q5 is None
    fx, fy, cx, cy = K
    new_K = RC.camera_matrix(0.9 * fx, 0.95 * fy, cx + 1.5, cy - 0.75)
    zero_row = np.array([1 / fx, 0.0, -cx / fx, 0.0, 1 / fy, -cy / fy, 0.0, 0.25, -0.25])    # Wd = 0 on row 1
    cases = {"R = I": dict(), "a 2 degree rotation, new_K != K": dict(R=rot_y(2.0), new_K=new_K),
             "Wd = 0 on a row": dict(ir=zero_row)}
    for name, kw in cases.items():
        ir, want = FP.remap_build_numpy(H, W, K, RC.FR1_DIST, **kw)
        got = P.build_remap(K, RC.FR1_DIST, **kw)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32 and tuple(got.shape) == (H, W, 2) and np.array_equal(P.remap_ir, ir)
        diff = int((got.cpu() != torch.from_numpy(want)).sum())
        print(f"{H}x{W} {name}: {diff} of {want.size} map entries differ")
        assert diff == 0, name
        if name == "Wd = 0 on a row":
            assert (want[1] == -FP.MAP_CLAMP).all() and (want[0] != -FP.MAP_CLAMP).any()
        else:
            assert (want != -FP.MAP_CLAMP).all()
    assert not np.array_equal(FP.remap_build_numpy(H, W, K, RC.FR1_DIST)[1],
                              FP.remap_build_numpy(H, W, K, RC.FR1_DIST, R=rot_y(2.0), new_K=new_K)[1])


# ---- 7: the identity map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset_type,H,W", [("tum", 17, 65), ("replica", 33, 35)])
@pytest.mark.parametrize("quantised", [False, True])
def test_identity_map_equals_the_unremapped_call(built, dataset_type, H, W, quantised):
    img = RC.make_image(H, W, H * 1000 + W, quantised=quantised).to(DEV)
    plain = snapshot(FP.FramePreparer(H, W, DEV, config(dataset_type), keep_intensity=True).prepare(img))
    R = FP.FramePreparer(H, W, DEV, config(dataset_type), keep_intensity=True, remap=identity_map(H, W))
    res = R.prepare(img)
    assert res["image"].data_ptr() == R.buffers["image"].data_ptr() != img.data_ptr()
    got = snapshot(res)
    torch.cuda.synchronize()
    assert same_bits(got, plain)


# ---- 8: real distortion against the mirror ------------------------------------------------------------------------------
DISTORTED_SHAPES = [("tum", 2, 2), ("tum", 16, 64), ("tum", 17, 65), ("tum", 48, 67), ("tum", 45, 70),
                    ("replica", 33, 35), ("replica", 65, 97)]


@pytest.mark.parametrize("dataset_type,H,W", DISTORTED_SHAPES)
def test_native_matches_the_mirror_with_real_distortion(built, dataset_type, H, W):
    et = 1.1
    _, m = RC.distorted_map(H, W)                       # asserts the border pixels of both kinds
    m = torch.from_numpy(m).to(DEV)
    P = FP.FramePreparer(H, W, DEV, config(dataset_type, et), keep_intensity=True, remap=m)
    for quantised in (False, True):
        img = RC.make_image(H, W, seed=H * 1000 + W, quantised=quantised).to(DEV)
        want = FP.prepare_frame_torch(img, dataset_type=dataset_type, edge_threshold=et, remap=m)
        got = P.prepare(img)
        torch.cuda.synchronize()
        name = f"{dataset_type} {H}x{W} {'uint8' if quantised else 'float'} remapped"
        assert torch.equal(got["image"].view(torch.int32), want["image"].view(torch.int32)), name
        assert not torch.equal(got["image"], FP.prepare_frame_torch(img, dataset_type=dataset_type,
                                                                    edge_threshold=et)["image"])
        compare(got, RC.as_case(want, H, W, dataset_type, et, name), "native vs mirror")


# ---- 9: the shift case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [False, True])
def test_shift_case_against_hand_arithmetic(built, quantised):
    H, W = 45, 70
    K, new_K = RC.shift_case(H, W)
    P = FP.FramePreparer(H, W, DEV, config("tum"))
    P.build_remap(K, (0.0,) * 5, new_K=new_K)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    assert np.array_equal(P.map_q5.cpu().numpy(), np.stack([32 * u - 168, 32 * v - 80], axis=-1))
    img = RC.make_image(H, W, 11, quantised=quantised)
    got = P.prepare(img)["image"].cpu()
    want = RC.shift_by_hand(img)
    if quantised:
        want = FP.convert_image_torch(want)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- 10: depth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [True, False])
def test_depth_modes(built, u16):
    H, W = 45, 70
    _, m = RC.distorted_map(H, W)
    m = torch.from_numpy(m).to(DEV)
    img = RC.make_image(H, W, 6, quantised=True).to(DEV)
    g = torch.Generator().manual_seed(9)
    if u16:
        depth = torch.randint(300, 40000, (H, W), generator=g).to(torch.int32).numpy().astype(np.uint16)
        scale = 5000.0
        converted = FP.convert_depth_torch(FP._as_tensor(depth), scale).to(DEV)
    else:
        depth, scale = (torch.rand(H, W, generator=g) * 5 + 0.2).to(DEV), None
        converted = depth
    plain = FP.FramePreparer(H, W, DEV, config("tum")).prepare(img, depth, scale)["gt_depth"].clone()
    keep = FP.FramePreparer(H, W, DEV, config("tum"), remap=m).prepare(img, depth, scale)["gt_depth"].clone()
    follow = FP.FramePreparer(H, W, DEV, config("tum"), remap=m, remap_depth=True).prepare(img, depth, scale)
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.int32), converted.reshape(1, H, W).view(torch.int32))
    assert torch.equal(keep.view(torch.int32), plain.view(torch.int32))
    want = FP.remap_depth_torch(converted, m).reshape(1, H, W)
    assert torch.equal(follow["gt_depth"].view(torch.int32), want.view(torch.int32))
    assert not torch.equal(want, plain) and int((want == 0).sum()) > 0
    mirror = FP.prepare_frame_torch(img, depth, dataset_type="tum", edge_threshold=1.1, depth_scale=scale, remap=m,
                                    remap_depth=True)
    assert torch.equal(mirror["gt_depth"], want) and torch.equal(mirror["image"], follow["image"])


# ---- 11: stability ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset_type", ["tum", "replica"])
def test_remapped_calls_are_bit_reproducible(built, dataset_type):
    H, W, et = 45, 70, 1.1
    _, m = RC.distorted_map(H, W)
    m = torch.from_numpy(m).to(DEV)
    P = FP.FramePreparer(H, W, DEV, config(dataset_type, et), keep_intensity=True, remap=m)
    a_img, b_img = RC.make_image(H, W, 1).to(DEV), RC.make_image(H, W, 2, quantised=True).to(DEV)
    a1 = snapshot(P.prepare(a_img))
    a2 = snapshot(P.prepare(a_img))
    assert same_bits(a1, a2)
    b = P.prepare(b_img)                                   # another image through the same scratch
    torch.cuda.synchronize()
    want = FP.prepare_frame_torch(b_img, dataset_type=dataset_type, edge_threshold=et, remap=m)
    assert torch.equal(b["image"], want["image"])
    compare(b, RC.as_case(want, H, W, dataset_type, et, f"{dataset_type} second image"), "native vs mirror")
    side = torch.cuda.Stream(device=DEV)
    Q = FP.FramePreparer(H, W, DEV, config(dataset_type, et), keep_intensity=True, remap=m)
    with torch.cuda.stream(side):
        got = Q.prepare(a_img)
    side.synchronize()
    assert same_bits(snapshot(got), a1)


# ---- 12: argument errors ---------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def raw_args(H, W, image, out, scratch):
    a = _cabi.FramePrepareArgs()
    a.width, a.height, a.mode = W, H, _cabi.FRAME_MODE_GLOBAL
    a.edge_threshold, a.rgb_boundary_threshold = 1.1, 0.01
    a.image_format, a.image_in, a.image = _cabi.FRAME_IMAGE_F32_CHW, image.data_ptr(), out["image"].data_ptr()
    a.depth_format = _cabi.FRAME_DEPTH_NONE
    a.gt_depth = out["gt_depth"].data_ptr()
    for k in ("grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping"):
        setattr(a, k, out[k].data_ptr())
    a.median_out, a.scratch = out["median"].data_ptr(), scratch.data_ptr()
    return a


def test_argument_errors_leave_the_outputs_untouched(built):
    H, W = 17, 65
    L = _cabi.lib()
    image = RC.make_image(H, W, 4).to(DEV)
    out = {k: torch.full((H * W,), SENTINEL, device=DEV) for k in ("grad_mask", "rgb_pixel_mask",
                                                                   "rgb_pixel_mask_mapping", "gt_depth")}
    out["image"] = torch.full((3 * H * W,), SENTINEL, device=DEV)
    out["median"] = torch.full((1,), SENTINEL, device=DEV)
    scratch = torch.zeros(int(L.mgs_frame_prepare_scratch_bytes(H, W)), dtype=torch.uint8, device=DEV)
    store = torch.zeros(H * W * 2 + 2, dtype=torch.int32, device=DEV)
    store[:H * W * 2] = identity_map(H, W).reshape(-1).to(DEV)
    assert store.data_ptr() % 8 == 0
    depth = torch.ones(H * W, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(a, r):
        return L.mgs_frame_prepare_remapped(C.byref(a), None if r is None else C.byref(r), stream)

    def remap(ptr, mode=_cabi.FRAME_REMAP_DEPTH_NONE):
        r = _cabi.FrameRemapArgs()
        r.map_q5, r.depth_mode = ptr, mode
        return r

    good = store.data_ptr()
    bad = []
    bad.append(("a null remap struct", raw_args(H, W, image, out, scratch), None))
    bad.append(("a null map", raw_args(H, W, image, out, scratch), remap(None)))
    bad.append(("a map at 4 mod 8", raw_args(H, W, image, out, scratch), remap(good + 4)))
    a = raw_args(H, W, image, out, scratch)
    a.image = image.data_ptr()
    bad.append(("image == image_in", a, remap(good)))
    a = raw_args(H, W, image, out, scratch)
    a.image = None
    bad.append(("a null image", a, remap(good)))
    bad.append(("depth_mode 2", raw_args(H, W, image, out, scratch), remap(good, 2)))
    bad.append(("depth_mode 1 without depth", raw_args(H, W, image, out, scratch),
                remap(good, _cabi.FRAME_REMAP_DEPTH_NEAREST)))
    a = raw_args(H, W, image, out, scratch)
    a.depth_format, a.depth_in, a.gt_depth = _cabi.FRAME_DEPTH_F32, depth.data_ptr(), depth.data_ptr()
    bad.append(("depth_mode 1 in place", a, remap(good, _cabi.FRAME_REMAP_DEPTH_NEAREST)))
    a = raw_args(H, W, image, out, scratch)
    a.grad_mask = None                                                       # what mgs_frame_prepare checks still applies
    bad.append(("a null grad_mask", a, remap(good)))
    before = image.clone()
    for name, a, r in bad:
        assert call(a, r) == -1, name
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t == SENTINEL).all()), k
    assert torch.equal(image, before) and not bool(scratch.any())
    # ... and the same arguments with nothing wrong run
    assert call(raw_args(H, W, image, out, scratch), remap(good)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out["image"].reshape(3, H, W), image) and float(out["median"][0]) != SENTINEL
    # the map builder's own checks
    b = _cabi.RemapBuildArgs()
    b.width, b.height, b.map_q5 = W, H, good + 4
    assert L.mgs_remap_build(C.byref(b), stream) == -1 and L.mgs_remap_build(None, stream) == -1
    b.map_q5 = None
    assert L.mgs_remap_build(C.byref(b), stream) == -1
    assert L.mgs_remap_build_args_size() == C.sizeof(_cabi.RemapBuildArgs) == 8 + 18 * 8 + 8
    assert L.mgs_frame_remap_args_size() == C.sizeof(_cabi.FrameRemapArgs) == 16


# ---- 13: the Python plumbing -------------------------------------------------------------------------------------------------
def test_preparer_builds_its_map_from_the_config(built):
    from monogs_amd.slam_loops import ViewCamera
    from monogs_amd import synthetic as S
    import math
    H, W = 45, 70
    cal = RC.calibration_for(H, W)
    _, want = RC.distorted_map(H, W)
    P = FP.FramePreparer(H, W, DEV, config("tum", calibration=cal))
    assert torch.equal(P.map_q5.cpu(), torch.from_numpy(want))
    assert FP.FramePreparer(H, W, DEV, config("tum", calibration=RC.calibration_for(H, W, distorted=False))).map_q5 is None
    assert FP.FramePreparer(H, W, DEV, config("tum"), calibration=cal).map_q5 is not None
    with pytest.raises(ValueError, match="remap_depth"):
        FP.FramePreparer(H, W, DEV, config("tum"), remap_depth=True)
    img = RC.make_image(H, W, 8).to(DEV)
    cam = S.make_camera(W, H, intrinsics=RC.intrinsics(cal))
    v = ViewCamera(0, img, torch.eye(4), cam.projmatrix_raw, 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy),
                   H, W, DEV)
    res = P.prepare_into(v)
    torch.cuda.synchronize()
    want_img = FP.remap_torch(img, P.map_q5)
    assert torch.equal(v.original_image, want_img) and v.original_image.data_ptr() != img.data_ptr()
    assert v.original_image.data_ptr() != P.buffers["image"].data_ptr() and res["image"] is v.original_image


def test_run_sequence_with_a_zero_coefficient_calibration(built):
    from monogs_amd import slam_surrogate as SS
    H, W, n = 120, 160, 3
    cal = RC.calibration_for(H, W, dist=(0.0,) * 5)
    frames, cam, _ = SS.load_sequence(n, W, H, DEV, world_gaussians=3000, calibration=cal)
    assert (cam.fx, cam.cy) == (cal["fx"], cal["cy"])
    base = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01},
            "Dataset": {"type": "tum", "pcd_downsample": 4, "pcd_downsample_init": 2}}
    with_cal = {"Training": dict(base["Training"]), "Dataset": dict(base["Dataset"], Calibration=cal)}
    kw = dict(native_frame_prepare=True, init_iters=20, mapping_iters=5, first_order_iters=5, second_order_iters=0)
    plain = SS.run_sequence(frames, cam, DEV, config=base, **kw)
    remapped = SS.run_sequence(frames, cam, DEV, config=with_cal, **kw)
    torch.cuda.synchronize()
    assert sorted(remapped["cameras"]) == list(range(n))
    for k in range(n):
        a, b = plain["cameras"][k], remapped["cameras"][k]
        assert a.original_image.data_ptr() == frames[k].image.data_ptr() != b.original_image.data_ptr()
        assert torch.equal(a.original_image.view(torch.int32), b.original_image.view(torch.int32)), k
        for key in ("grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping"):
            assert torch.equal(getattr(a, key), getattr(b, key)), (k, key)


def test_run_sequence_seeds_and_scores_from_the_undistorted_image(built, monkeypatch):
    """With real coefficients the raw frame and the camera's image differ: what keyframe insertion (both paths) and
    evaluate() consume must be the camera's undistorted image."""
    from monogs_amd import eval_metrics as E
    from monogs_amd import slam_surrogate as SS
    from monogs_amd.gaussian_model import GaussianModel
    H, W, n = 120, 160, 3
    cal = RC.calibration_for(H, W)
    _, m = RC.distorted_map(H, W)
    m = torch.from_numpy(m).to(DEV)
    frames, cam, _ = SS.load_sequence(n, W, H, DEV, world_gaussians=3000, calibration=cal)   # rendered: taken as raw
    cfg = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01},
           "Dataset": {"type": "tum", "pcd_downsample": 4, "pcd_downsample_init": 2, "Calibration": cal}}
    want = [FP.remap_torch(f.image, m) for f in frames]
    assert all(not torch.equal(w, f.image) for w, f in zip(want, frames))
    seen = {"depth": [], "seed": [], "psnr": []}
    keyframe_depth, extend, psnr = SS.keyframe_depth, GaussianModel.extend_from_keyframe, E.psnr

    def spy_depth(image, *a, **k):
        seen["depth"].append(image)
        return keyframe_depth(image, *a, **k)

    def spy_seed(self, seeder, view, image, *a, **k):
        seen["seed"].append(image)
        return extend(self, seeder, view, image, *a, **k)

    def spy_psnr(img, gt, *a, **k):
        seen["psnr"].append(gt)
        return psnr(img, gt, *a, **k)

    monkeypatch.setattr(SS, "keyframe_depth", spy_depth)
    monkeypatch.setattr(GaussianModel, "extend_from_keyframe", spy_seed)
    monkeypatch.setattr(E, "psnr", spy_psnr)
    kw = dict(native_frame_prepare=True, init_iters=20, mapping_iters=5, first_order_iters=5, second_order_iters=0,
              config=cfg)
    for seeded in (False, True):                                  # kf_interval 1: every frame is inserted
        res = SS.run_sequence(frames, cam, DEV, native_keyframe_seed=seeded, kf_interval=1, **kw)
        torch.cuda.synchronize()
        got = seen["seed" if seeded else "depth"]
        assert len(got) == n and not seen["depth" if seeded else "seed"]
        for k, img in enumerate(got):
            assert img.data_ptr() == res["cameras"][k].original_image.data_ptr(), (seeded, k)
            assert torch.equal(img.view(torch.int32), want[k].view(torch.int32)), (seeded, k)
        if seeded:
            assert sorted(res["seed_records"]) == list(range(n))
        got.clear()
    res = SS.run_sequence(frames, cam, DEV, kf_interval=5, **kw)   # frames 1 and 2 are no keyframes: scored
    out = SS.evaluate(res, frames, DEV)
    assert out["psnr_frames"] == 2 and len(seen["psnr"]) == 2
    for k, gt in zip((1, 2), seen["psnr"]):
        assert torch.equal(gt[0], want[k])


def test_run_sequence_raw_inputs(built):
    from monogs_amd import slam_surrogate as SS
    H, W, n = 120, 160, 2
    cal = RC.calibration_for(H, W)
    _, m = RC.distorted_map(H, W)
    m = torch.from_numpy(m).to(DEV)
    frames, cam, _ = SS.load_sequence(n, W, H, DEV, world_gaussians=3000, calibration=cal)
    cfg = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01},
           "Dataset": {"type": "tum", "pcd_downsample": 4, "pcd_downsample_init": 2, "Calibration": cal}}
    kw = dict(init_iters=20, mapping_iters=5, first_order_iters=5, second_order_iters=0, config=cfg)
    # uint8 [H,W,3], what TUMSequence.image_u8 hands over
    u8 = [SS.Frame(f.uid, f.image.mul(255).round().to(torch.uint8).permute(1, 2, 0).contiguous(), None, f.T_gt)
          for f in frames]
    res = SS.run_sequence(u8, cam, DEV, native_frame_prepare=True, **kw)
    torch.cuda.synchronize()
    for k in range(n):
        want = FP.convert_image_torch(FP.remap_torch(u8[k].image, m))
        assert torch.equal(res["cameras"][k].original_image, want)
    with pytest.raises(ValueError, match="uint8"):
        SS.run_sequence(u8, cam, DEV, **kw)
    # frames a reader already undistorted are not remapped a second time
    done = [SS.Frame(f.uid, f.image, None, f.T_gt, undistorted=True) for f in frames]
    with pytest.raises(ValueError, match="undistorted"):
        SS.run_sequence(done, cam, DEV, native_frame_prepare=True, **kw)
    plain = dict(kw, config={k: dict(v) for k, v in cfg.items()})
    plain["config"]["Dataset"].pop("Calibration")
    assert sorted(SS.run_sequence(done, cam, DEV, native_frame_prepare=True, **plain)["cameras"]) == [0, 1]
    # set_remap(None) on a preparer whose depth follows the map is refused like the constructor refuses it
    P = FP.FramePreparer(H, W, DEV, cfg, remap_depth=True)
    with pytest.raises(ValueError, match="remap_depth"):
        P.set_remap(None)
