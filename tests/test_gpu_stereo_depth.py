"""mgs_stereo_depth (stereo_depth.hip) on the MI355X against the NumPy mirror, bit for bit - every step is integer
arithmetic and one correctly rounded double division, so there is no tolerance anywhere in this file - at the reference's
block 20 / ratio 40 and across the block sizes 1..29 and uniqueness ratios 0..100 the device accepts; and the Python
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


# ---- every block size and uniqueness ratio ------------------------------------------------------------------------------
# The cases above run at the reference's one setting, block 20 and ratio 40.  Below, the device against the mirror at the
# other settings it accepts.  Each case first asserts ON THE MIRROR that the branches it is named for occur (thresholds
# well below the counts measured with the mirror, which are quoted), prints the counts, then asks the device.
def mirror_case(name, H, W, b, u):
    """The mirror's (disp16, depth) of a pair at block b and ratio u, and its counts - printed, so that the log shows
    which branches a case took."""
    disp16, depth, not_unique, failed = SC.mirror(name, H, W, blockSize=b, uniquenessRatio=u)
    C_ = SC.mirror_block_cost(name, H, W, b // 2)
    valid = disp16 >= 0
    above = C_[:, D:] > 32767
    n = {"valid": int(valid.sum()), "columns": H * (W - D), "not_unique": int(not_unique.sum()),
         "left_right": int(failed.sum()), "sub_pixel": int((valid & (disp16 % 16 != 0)).sum()),
         "distinct": int(np.unique(disp16[valid] >> 4).size), "c_min": int(C_[:, D:].min()), "c_max": int(C_.max()),
         "share_above_32767": float(above.mean()),
         "pixels_on_both_sides_of_32768": int((above.any(-1) & ~above.all(-1)).sum())}
    print(f"mirror {name} {H}x{W} block {b} ratio {u}:", n)
    assert C_.max() + 5 <= 65535                                 # the header's bound: what the 16-bit volumes rely on
    return disp16, depth, n


def device_case(name, H, W, b, u, disp16, depth):
    left = SC.pair(name, H, W)[0]
    res = SD.StereoMatcher(H, W, DEV, blockSize=b, uniquenessRatio=u).compute(*SC.pair(name, H, W))
    assert_equals_mirror(res, disp16, depth, left)
    return snapshot(res)


@pytest.mark.parametrize("b", [1, 2, 3, 5, 28, 29])
def test_block_sizes_on_the_ramp(built, b):
    """r = 0 and r = 1: the start-up loop of k_sd_hsum and the -r..r loop of k_sd_vsum degenerate, the running sums add
    and subtract adjacent columns and rows.  r = 2, and r = 14, the largest.  Measured on the mirror (valid, not_unique,
    left-right): block 1: 4121, 214, 808; 2 and 3: 4123, 190, 830; 5: 4088, 247, 808; 28 and 29: 742, 4383, 18."""
    disp16, depth, n = mirror_case("ramp", 37, 203, b, 40)
    assert n["valid"] > 500 and n["not_unique"] > 100 and n["left_right"] > 10
    device_case("ramp", 37, 203, b, 40, disp16, depth)


@pytest.mark.parametrize("even,odd", [(2, 3), (28, 29)])
def test_the_device_reads_the_half_block_not_the_parity(built, even, odd):
    left, right = SC.pair("ramp", 37, 203)
    a, b = (snapshot(SD.StereoMatcher(37, 203, DEV, blockSize=k).compute(left, right)) for k in (even, odd))
    assert same_bits(a, b)
    assert (a["disp16"] >= 0).sum().item() > 500                 # and they are not the same for being empty


@pytest.mark.parametrize("u", [0, 1, 99, 100])
def test_uniqueness_ratios_on_the_ramp(built, u):
    """s * (100 - ratio) < sb * 100 at its ends.  At 0 nothing is rejected and the left-right vote sees every pixel
    (measured: left-right 899, valid 4244); at 1, 22 pixels are; at 99 and 100 every pixel is (sb > 0 everywhere)."""
    disp16, depth, n = mirror_case("ramp", 37, 203, 20, u)
    if u == 0:
        assert n["not_unique"] == 0 and n["left_right"] > 300 and n["valid"] > 3000
    elif u == 1:
        assert 0 < n["not_unique"] < 200
    else:
        assert n["valid"] == 0 and n["not_unique"] == n["columns"] and (depth == 0).all()
    res = device_case("ramp", 37, 203, 20, u, disp16, depth)
    if u >= 99:
        assert (res["depth"] == 0).all() and (res["disp16"] == -16).all()


def test_identical_images_at_ratio_100_and_block_29(built):
    """sb == 0 at d = 0 in every valid column: the one way through ratio 100."""
    img = SC.noise(23, 87, 3)
    disp16, depth = SD.stereo_sgbm_numpy(img, img, blockSize=29, uniquenessRatio=100)
    z = np.float32(SD.BF_REFERENCE / 1e10)
    assert (disp16[:, D:] == 0).all() and (disp16[:, :D] == -16).all()             # the mirror says so
    assert z > 0 and (depth[:, D:] == z).all() and (depth[:, :D] == 0).all()
    res = SD.StereoMatcher(23, 87, DEV, blockSize=29, uniquenessRatio=100).compute(img, img)
    assert_equals_mirror(res, disp16, depth, img)
    assert (res["disp16"][:, D:] == 0).all() and (res["depth"][0, :, D:] == float(z)).all()
    assert (res["depth"][0, :, :D] == 0).all()


# The upper half of the 16-bit volumes.  C, hs and the five L are uint16_t, and bit 15 can be set only from r = 11
# (23 * 23 * 70 = 37 030; at block 20 the cap is 441 * 70 = 30 870, so no case above sets it).  A brightness offset
# between the images (stereo_cases.OFFSET_LIFT) makes every pixel cost about 40 to 50, at block 29 and ratio 0, where no
# pixel is hidden by the uniqueness test and disp16 exposes each pixel's argmin and sub-pixel value.  Two kinds of pair:
#   "straddle_low", "straddle_high"   C from about 30 000 to 35 000: most pixels have disparities on both sides of
#       32 768.  A signed read of C or L (L = C + 0..5), or a store that dropped bit 15, would move those costs by 65 536
#       or 32 768 against their neighbours in the same pixel: the path minimum, every L, the argmin of S and the
#       sub-pixel term move.  Simulated on the mirror (tests/test_cpu_stereo_depth.py,
#       test_the_straddling_pairs_show_a_wrong_read_of_bit_15): either fault changes 4387 and 4669 of disp16's 7511
#       entries at 37x203, 1837 and 1785 of 4257 at 33x129.  These are the cases that would catch it.
#   "offset"   every valid entry of C above 32 767, up to 42 393.  Either fault would shift a pixel's 64 costs ALIKE,
#       which disp16 does not show (simulated there too: no entry changes).  What this pair does exercise is size:
#       k_sd_vsum's packed adds near their 16-bit halves' capacity (a carry into the neighbouring disparity changes
#       its C by one), L up to C + 5, S of 19 bits in k_sd_select's (S << 6 | d) key.
def upper_half_case(name, H, W):
    disp16, depth, n = mirror_case(name, H, W, 29, 0)
    if name == "offset":
        assert n["c_max"] > 40000 and n["c_min"] > 32767 and n["share_above_32767"] == 1.0
    else:
        assert 0.1 < n["share_above_32767"] < 0.9 and 2 * n["pixels_on_both_sides_of_32768"] > n["columns"]
    return disp16, depth, n


@pytest.mark.parametrize("name", ["offset", "straddle_low", "straddle_high"])
def test_upper_half_of_the_16_bit_volumes(built, name):
    """37x203 at block 29 and ratio 0.  Measured on the mirror, offset: C 37 763 .. 42 393, valid 3670, sub-pixel 3040, 48
    distinct integer disparities, left-right failures 1473.  straddle_low: C 30 312 .. 34 921, share above 0.206, 4573
    of 5143 pixels on both sides, valid 3619.  straddle_high: C 30 810 .. 35 254, share 0.778, 4997 pixels, valid 3657."""
    disp16, depth, n = upper_half_case(name, 37, 203)
    assert n["valid"] > 2000 and n["sub_pixel"] > 1500 and n["distinct"] > 30 and n["left_right"] > 500
    device_case(name, 37, 203, 29, 0, disp16, depth)


@pytest.mark.parametrize("name", ["offset", "straddle_low", "straddle_high"])
def test_upper_half_with_a_second_segment_and_a_second_trip(built, name):
    """33x129: the second 64-column segment of k_sd_hsum and the second 32-row trip of k_sd_vsum.  Measured on the
    mirror, offset: C 37 060 .. 42 347, valid 1130.  straddle_low: C 29 819 .. 34 931, share 0.290, 2039 of 2145 pixels
    on both sides, valid 1117.  straddle_high: C 30 193 .. 35 463, share 0.775, 1946 pixels, valid 1110."""
    disp16, depth, n = upper_half_case(name, 33, 129)
    assert n["valid"] > 500
    device_case(name, 33, 129, 29, 0, disp16, depth)


def test_upper_half_through_a_reused_scratch(built):
    """hs lives in the first direction's L volume: what one call leaves there, bit 15 set or not, must not reach the
    next.  The offset pair twice, then a straddling pair (bit 15 set in a fifth of the entries) and the ramp pair
    (measured C.max() 14 298: bit 15 nowhere, valid 4219), and the offset pair again, through one matcher: each call
    equals the mirror."""
    H, W = 37, 203
    offset = upper_half_case("offset", H, W)[:2]
    straddle = upper_half_case("straddle_low", H, W)[:2]
    ramp = mirror_case("ramp", H, W, 29, 0)
    assert ramp[2]["c_max"] < 32768 and ramp[2]["valid"] > 2000
    M = SD.StereoMatcher(H, W, DEV, blockSize=29, uniquenessRatio=0)
    left, right = SC.pair("offset", H, W)
    a1 = snapshot(M.compute(left, right))
    assert_equals_mirror(a1, *offset, left)
    a2 = snapshot(M.compute(left, right))
    assert same_bits(a1, a2)
    assert_equals_mirror(M.compute(*SC.pair("straddle_low", H, W)), *straddle, SC.pair("straddle_low", H, W)[0])
    assert_equals_mirror(M.compute(*SC.pair("ramp", H, W)), *ramp[:2], SC.pair("ramp", H, W)[0])
    a3 = snapshot(M.compute(left, right))
    assert same_bits(a1, a3)
    assert_equals_mirror(a3, *offset, left)


# Tall and narrow: H up to 65 times the valid width Wv = W - 64, three and four 32-row trips of k_sd_vsum, sd_path's
# diagonals that start from the side (p >= Wv) at every length n = min(Wv - xv, H - y), and at block 29 a window ten
# times as wide as the valid region.  Measured on the mirror (valid of valid-column pixels): 70x67 179 of 210 at 20 / 40,
# 208 at 29 / 0, 195 at 1 / 0; 100x66 169 of 200 and 200; 41x70 174 of 246 and 240; 65x65 54 of 65 and 65.
@pytest.mark.parametrize("H,W,b,u", [(H, W, b, u) for H, W in ((70, 67), (100, 66), (41, 70), (65, 65))
                                     for b, u in ((20, 40), (29, 0))] + [(70, 67, 1, 0)])
def test_tall_and_narrow(built, H, W, b, u):
    disp16, depth, n = mirror_case("ramp", H, W, b, u)
    assert 2 * n["valid"] >= n["columns"] and n["sub_pixel"] > 0
    device_case("ramp", H, W, b, u, disp16, depth)


# ---- behaviour ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,status", [({"blockSize": 30}, -3), ({"blockSize": 31}, -3), ({"uniquenessRatio": 101}, -1),
                                       ({"uniquenessRatio": -1}, -1)])
def test_the_matcher_refuses_what_the_device_does_not_take(built, kw, status):
    """MGS_ERR_UNSUPPORTED past block 29, MGS_ERR_BAD_ARGUMENT outside ratio 0..100: raised by compute, as _cabi.check
    raises every status, before anything is launched - the outputs keep what they held."""
    H, W = 3, 66
    M = SD.StereoMatcher(H, W, DEV, **kw)                        # the constructor takes them: the device decides
    fill = {"depth": -7.0, "disp16": -1234, "image": -7.0}
    for k, v in fill.items():
        M.buffers[k].fill_(v)
    with pytest.raises(RuntimeError, match=rf"mgs_stereo_depth failed: .*\(status {status}\)"):
        M.compute(*SC.pair("noise", H, W))
    torch.cuda.synchronize()
    for k, v in fill.items():
        assert (M.buffers[k] == v).all(), k
    assert set(M.buffers) == set(fill)


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
