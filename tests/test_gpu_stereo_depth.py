"""mgs_stereo_depth (stereo_depth.hip) on the MI355X against the NumPy mirror, bit for bit - every step is integer
arithmetic and one correctly rounded double division, so there is no tolerance anywhere in this file - and the Python
surface: StereoMatcher's input formats, its maps, compute_into, run_sequence(stereo_matcher=...)."""
import ctypes as C

import numpy as np
import pytest
import torch

from monogs_amd import _cabi
from monogs_amd import frame_prepare as FP
from monogs_amd import stereo_depth as SD
import stereo_cases as SC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D = 64


def t(a):
    return torch.from_numpy(np.array(a))


def snapshot(res):
    return {k: v.clone() for k, v in res.items()}


def same_bits(a, b):
    return (torch.equal(a["disp16"], b["disp16"]) and torch.equal(a["image"], b["image"])
            and torch.equal(a["depth"].view(torch.int32), b["depth"].view(torch.int32)))


def assert_equals_mirror(res, disp16, depth, left=None):
    got_d, got_z = res["disp16"].cpu(), res["depth"].cpu()
    assert tuple(got_z.shape) == (1,) + tuple(disp16.shape) and got_z.dtype == torch.float32
    bad = (got_d != t(disp16)).sum().item()
    print("disp16 entries that differ:", bad, "of", disp16.size)
    assert torch.equal(got_d, t(disp16))
    assert torch.equal(got_z[0].view(torch.int32), t(depth).view(torch.int32))
    if left is not None:
        want = (t(left).to(torch.float64) / 255.0).to(torch.float32)
        assert torch.equal(res["image"].cpu(), want.expand(3, *want.shape))


# ---- mirror agreement ---------------------------------------------------------------------------------------------------
# 1x65: one valid column, one row.  3x66.  23x87: just past the block in both directions.  33x129: the smallest image
# with a second 64-column segment of k_sd_hsum (W - 64 = 65) and a second 32-row segment of k_sd_vsum (H = 33) - the two
# sizes at which those kernels take another trip (DESIGN.md "Stereo depth on the device", thresholds).
@pytest.mark.parametrize("name,H,W", [("ramp", 1, 65), ("ramp", 3, 66), ("noise", 3, 66), ("ramp", 23, 87),
                                      ("noise", 23, 87), ("ramp", 33, 129)])
def test_native_equals_the_mirror_at_the_smallest_shapes(built, name, H, W):
    left, right = SC.pair(name, H, W)
    disp16, depth = SC.mirror(name, H, W)[:2]
    res = SD.StereoMatcher(H, W, DEV).compute(left, right)
    assert_equals_mirror(res, disp16, depth, left)


def test_native_equals_the_mirror_on_the_planes_pair_and_has_its_property(built):
    left, right, d = SC.planes_pair()
    H, W = left.shape
    res = SD.StereoMatcher(H, W, DEV).compute(left, right)
    assert_equals_mirror(res, *SC.mirror("planes")[:2], left)
    inside = SC.planes_interior(d)                              # the planes property, natively
    disp = res["disp16"].cpu().numpy().astype(np.int64)
    assert inside.sum() == 2312 and (disp[inside] >= 0).all() and (np.abs(disp - 16 * d)[inside] <= 8).all()
    assert (disp[:, :D] == -16).all() and (res["depth"][0, :, :D] == 0).all()


def test_native_equals_the_mirror_on_the_ramp_with_every_branch_taken(built):
    """37x203, odd sizes: sub-pixel disparities, occlusions, uniqueness and left-right failures - asserted to occur."""
    left, right = SC.pair("ramp")
    disp16, depth, not_unique, failed = SC.mirror("ramp")
    assert left.shape == (37, 203)
    valid = disp16 >= 0
    assert valid.sum() > 1000 and not_unique.sum() > 100 and failed.sum() > 20
    assert (valid & (disp16 % 16 != 0)).sum() > 500 and np.unique(disp16[valid] >> 4).size > 10
    assert_equals_mirror(SD.StereoMatcher(37, 203, DEV).compute(left, right), disp16, depth, left)


def test_identical_images_natively(built):
    img = SC.noise(23, 87, 3)
    res = SD.StereoMatcher(23, 87, DEV, bf=2.5).compute(img, img)
    assert (res["disp16"][:, D:] == 0).all() and (res["disp16"][:, :D] == -16).all()
    assert (res["depth"][0, :, D:] == float(np.float32(2.5 / 1e10))).all() and (res["depth"][0, :, :D] == 0).all()


# ---- behaviour ------------------------------------------------------------------------------------------------------------
def test_two_runs_a_reused_matcher_and_a_side_stream(built):
    H, W = 37, 203
    left, right = (t(a).to(DEV) for a in SC.pair("ramp"))
    other = tuple(t(a).to(DEV) for a in SC.pair("noise", H, W))
    M = SD.StereoMatcher(H, W, DEV)
    a1 = snapshot(M.compute(left, right))
    a2 = snapshot(M.compute(left, right))
    assert same_bits(a1, a2)
    b = snapshot(M.compute(*other))                             # another pair through the same scratch
    assert_equals_mirror(b, *SC.mirror("noise", H, W)[:2])
    a3 = snapshot(M.compute(left, right))                       # and back: nothing of the other pair is left behind
    assert same_bits(a1, a3)
    side = torch.cuda.Stream(device=DEV)
    Q = SD.StereoMatcher(H, W, DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = snapshot(Q.compute(left, right))
    side.synchronize()
    assert same_bits(got, a1)
    assert_equals_mirror(got, *SC.mirror("ramp")[:2])


def test_input_formats(built):
    H, W = 23, 87
    left, right = SC.pair("ramp", H, W)
    M = SD.StereoMatcher(H, W, DEV)
    want = snapshot(M.compute(left, right))                                     # uint8 grey, NumPy
    hwc = [t(np.stack([a] * 3, -1)) for a in (left, right)]                     # uint8 HWC, host tensors
    assert same_bits(snapshot(M.compute(*hwc)), want)
    chw = [(t(np.stack([a] * 3)).to(torch.float64) / 255.0).to(torch.float32).to(DEV) for a in (left, right)]
    assert same_bits(snapshot(M.compute(*chw)), want)                           # float CHW, device tensors
    # three different channels: the fixed-point grey of the module docstring
    rng = np.random.default_rng(9)
    rgb = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
    grey = [SD.to_grey_numpy(a) for a in rgb]
    assert_equals_mirror(M.compute(*rgb), *SD.stereo_sgbm_numpy(*grey), grey[0])
    flt = [rng.random((3, H, W)).astype(np.float32) for _ in range(2)]
    grey = [SD.to_grey_numpy(a) for a in flt]
    assert_equals_mirror(M.compute(*flt), *SD.stereo_sgbm_numpy(*grey), grey[0])
    with pytest.raises(ValueError):
        M.compute(left, hwc[1])
    with pytest.raises(ValueError):
        M.compute(left[:, :-1], right[:, :-1])


def test_arguments(built):
    with pytest.raises(ValueError, match="numDisparities"):
        SD.StereoMatcher(23, 87, DEV, numDisparities=32)
    with pytest.raises(ValueError, match="refused"):
        SD.StereoMatcher(23, 64, DEV)
    H, W = 3, 66
    M = SD.StereoMatcher(H, W, DEV)
    left, right = (t(a).to(DEV) for a in SC.pair("noise", H, W))
    depth = torch.full((H, W), -7.0, device=DEV)
    a = _cabi.StereoDepthArgs()
    a.width, a.height, a.image_format = W, H, _cabi.STEREO_IMAGE_U8_GREY
    a.num_disparities, a.block_size, a.uniqueness_ratio, a.bf = 64, 20, 40, 1.0
    a.left_in, a.right_in, a.depth, a.scratch = left.data_ptr(), right.data_ptr(), depth.data_ptr(), M.scratch.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    call = lambda: _cabi.lib().mgs_stereo_depth(C.byref(a), stream)
    for field, value, status in (("num_disparities", 32, -3), ("block_size", 31, -3), ("block_size", 0, -1),
                                 ("uniqueness_ratio", 101, -1), ("image_format", 3, -1), ("width", 64, -1),
                                 ("scratch", M.scratch.data_ptr() + 4, -1), ("map_left", M.scratch.data_ptr() + 4, -1)):
        keep = getattr(a, field)
        setattr(a, field, value)
        assert call() == status, field
        setattr(a, field, keep)
    torch.cuda.synchronize()
    assert (depth == -7.0).all()                                 # refused before anything was written
    assert call() == 0                                           # disp16 and image are optional
    torch.cuda.synchronize()
    want = SD.stereo_sgbm_numpy(*SC.pair("noise", H, W), bf=1.0)[1]
    assert torch.equal(depth.cpu().view(torch.int32), t(want).view(torch.int32))


# ---- remapped pair ----------------------------------------------------------------------------------------------------------
def stereo_calibration(H, W):
    """A synthetic distorted stereo calibration in the reference's layout (cam0 / cam1: raw, opt, R)."""
    def rot_y(deg):
        a = np.deg2rad(deg)
        return [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]

    def cam(fx, cx, k1, deg):
        raw = {"fx": fx, "fy": fx * 1.01, "cx": cx, "cy": 0.52 * H, "k1": k1, "k2": 0.07, "p1": 1e-3, "p2": -5e-4,
               "k3": 0.0}
        opt = {"fx": 0.7 * W, "fy": 0.7 * W, "cx": 0.5 * W, "cy": 0.5 * H}
        return {"raw": raw, "opt": opt, "R": {"rows": 3, "cols": 3, "data": np.ravel(rot_y(deg)).tolist()}}

    return {"cam0": cam(0.95 * W, 0.49 * W, -0.28, 0.6), "cam1": cam(0.94 * W, 0.51 * W, -0.27, -0.4),
            "distorted": True, "width": W, "height": H}


@pytest.mark.parametrize("fmt", ["u8", "hwc", "f32"])
def test_raw_pair_through_a_distorted_calibration(built, fmt):
    """The native result on a RAW pair equals the mirror on frame_prepare.remap_torch's rectified greys: a uint8 gather
    rounds to a byte ((.. + 512) >> 10), a float gather is quantised by the grey rule afterwards."""
    H, W = 45, 150
    cal = stereo_calibration(H, W)
    left, right = SC.pair("ramp", H, W)
    M = SD.StereoMatcher(H, W, DEV, {"Dataset": {"Calibration": cal}})
    maps = []
    for (K, dist, R, new_K), got in zip(SD.stereo_calibration_remaps(cal), (M.map_left, M.map_right)):
        m = FP.remap_build_numpy(H, W, K, dist, R, new_K)[1]
        assert torch.equal(got.cpu(), t(m))
        maps.append(t(m))
    if fmt == "f32":
        raw = [(t(np.stack([a] * 3)).to(torch.float32) / 255.0) * torch.tensor([1.0, 0.9, 0.8]).view(3, 1, 1)
               for a in (left, right)]
    else:
        raw = [t(np.stack([a] * 3, -1)) for a in (left, right)]
    grey = [SD.to_grey_numpy(FP.remap_torch(a, m)) for a, m in zip(raw, maps)]
    assert any((g == 0).any() for g in grey) and not np.array_equal(grey[0], left)      # the border and the warp are there
    disp16, depth = SD.stereo_sgbm_numpy(*grey)
    assert (disp16 >= 0).sum() > 200
    given = [t(a) for a in (left, right)] if fmt == "u8" else raw
    assert_equals_mirror(M.compute(*given), disp16, depth, grey[0])
    # without the calibration's `distorted` no map is built
    assert SD.StereoMatcher(H, W, DEV, calibration=dict(cal, distorted=False)).map_left is None
    # caller-made maps
    Q = SD.StereoMatcher(H, W, DEV, remap_left=maps[0], remap_right=maps[1])
    assert_equals_mirror(Q.compute(*given), disp16, depth, grey[0])


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_run_sequence_with_a_matcher_equals_sensor_depth_fed_the_matchers_depths(built):
    """Two routes through the same arithmetic (not an accuracy claim): the pair handed to run_sequence with the matcher,
    and the matcher's image and depth precomputed and handed over as an RGB-D sequence."""
    from monogs_amd import slam_surrogate as SS
    H, W, n = 96, 160, 3
    frames, cam, _ = SS.load_sequence(n, W, H, DEV, world_gaussians=30000, stereo_baseline=0.05)
    assert all(f.image.dtype == torch.uint8 and tuple(f.image_right.shape) == (H, W) for f in frames)
    M = SD.StereoMatcher(H, W, DEV, bf=cam.fx * 0.05)
    pre = []
    for f in frames:
        res = M.compute(f.image, f.image_right)
        pre.append(SS.Frame(f.uid, res["image"].clone(), res["depth"][0].clone(), f.T_gt))
    print("share of frame 0 with a depth:", (pre[0].depth > 0).float().mean().item())
    assert (pre[0].depth > 0).float().mean() > 0.2               # disparities of 1 .. 13 pixels: most of it is matched
    cfg = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01},
           "Dataset": {"type": "tum", "pcd_downsample": 4, "pcd_downsample_init": 2}}
    kw = dict(config=cfg, native_frame_prepare=True, kf_interval=1, init_iters=20, mapping_iters=5, first_order_iters=5,
              second_order_iters=0)
    a = SS.run_sequence(frames, cam, DEV, stereo_matcher=M, **kw)
    b = SS.run_sequence(pre, cam, DEV, sensor_depth=True, **kw)
    torch.cuda.synchronize()
    assert sorted(a["cameras"]) == sorted(b["cameras"]) == list(range(n))
    assert len(a["gaussians"]) == len(b["gaussians"]) > 0 and a["kf_ids"] == b["kf_ids"]
    for k in range(n):
        va, vb = a["cameras"][k], b["cameras"][k]
        assert torch.equal(va.original_image, vb.original_image) and torch.equal(va.gt_depth, vb.gt_depth), k
        print("frame", k, "max |dT|", (va.T - vb.T).abs().max().item())
        assert torch.isfinite(va.T).all() and torch.equal(va.T, vb.T), k
    with pytest.raises(ValueError, match="image_right"):
        SS.run_sequence(pre, cam, DEV, stereo_matcher=M, **kw)


# ---- full size --------------------------------------------------------------------------------------------------------------
def test_the_euroc_size_twice(built):
    H, W = 480, 752
    left, right, d = SC.planes_pair(H, W, seed=4, split_x=400)
    M = SD.StereoMatcher(H, W, DEV)
    a = snapshot(M.compute(left, right))
    b = snapshot(M.compute(left, right))
    assert same_bits(a, b)
    assert torch.isfinite(a["depth"]).all() and (a["depth"] >= 0).all()
    assert (a["disp16"] >= -16).all() and (a["disp16"] <= 16 * 63).all()
    inside = np.zeros((H, W), bool)                             # far from every edge of a plane: the true disparity
    inside[30:210, 100:370] = inside[270:450, 100:370] = inside[30:210, 430:720] = inside[270:450, 430:720] = True
    disp = a["disp16"].cpu().numpy().astype(np.int64)
    assert (np.abs(disp - 16 * d)[inside] <= 8).all()
