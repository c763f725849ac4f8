"""The NumPy mirror of stereo depth (monogs_amd/stereo_depth.py, DESIGN.md "Stereo depth on the device") without a GPU:
the planes property, the quirks of the reference's depth lines, the steps against hand-written loops at shapes smaller
than the block, and the host-only side of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from monogs_amd import stereo_depth as SD
import stereo_cases as SC

D = 64
BF = SD.BF_REFERENCE


# ---- planes -------------------------------------------------------------------------------------------------------------
def test_planes_interior_is_valid_and_within_half_a_pixel():
    """In the interior C(p, d_true) = 0, so S(d_true) <= 5 * P2 = 25 while wrong disparities cost thousands: every
    interior pixel must be valid with |disp16 - 16 d| <= 8.  No cap: every interior pixel counts."""
    _, _, d = SC.planes_pair()
    inside = SC.planes_interior(d)
    assert inside.sum() == 2312                      # 56x176: the four blocks' interiors
    disp = SC.mirror("planes")[0].astype(np.int64)
    print("interior pixels", inside.sum(), "invalid", (disp[inside] < 0).sum(), "max |disp16 - 16 d|",
          np.abs(disp - 16 * d)[inside].max())
    assert (disp[inside] >= 0).all()
    assert (np.abs(disp - 16 * d)[inside] <= 8).all()


# ---- quirks -------------------------------------------------------------------------------------------------------------
def test_left_columns_are_invalid_with_depth_zero():
    for name in ("planes", "ramp"):
        disp, depth = SC.mirror(name)[:2]
        assert disp.dtype == np.int16 and depth.dtype == np.float32
        assert (disp[:, :D] == -16).all() and (depth[:, :D] == 0).all()


def test_identical_images_give_disparity_zero_and_the_reference_depth_of_it():
    img = SC.noise(23, 87, 3)
    disp, depth = SD.stereo_sgbm_numpy(img, img)
    assert (disp[:, D:] == 0).all()
    assert (depth[:, D:] == np.float32(BF / 1e10)).all() and np.float32(BF / 1e10) > 0
    assert (depth[:, :D] == 0).all()


def test_unrelated_noise_fails_uniqueness_and_gets_depth_zero():
    disp, depth, not_unique, _ = SC.mirror("noise", 23, 87)
    assert not_unique[:, D:].any()
    assert (disp[not_unique] == -16).all() and (depth[not_unique] == 0).all()
    assert (depth[disp < 0] == 0).all() and (depth[disp > 0] > 0).all()


def test_depth_lines_to_the_letter():
    disp16 = np.array([[-16, 0, 1, 16, 1008]], np.int16)
    want = np.array([[0.0, BF / 1e10, BF / (1 / 16.0), BF / 1.0, BF / 63.0]]).astype(np.float32)
    assert np.array_equal(SD.depth_numpy(disp16), want)
    assert np.array_equal(SD.depth_numpy(disp16, bf=2.0)[0, 3:], np.array([2.0, 2.0 / 63.0], np.float32))


def test_keyword_arguments_are_read():
    left, right = SC.pair("noise", 5, 40)
    with pytest.raises(ValueError):
        SD.stereo_sgbm_numpy(left, right)                                   # W <= 64
    disp, depth = SD.stereo_sgbm_numpy(left, right, numDisparities=16, blockSize=5, uniquenessRatio=0, bf=3.0)
    assert (disp[:, :16] == -16).all() and disp.max() <= 16 * 15
    assert (disp[:, 16:] >= 0).any()
    v = disp > 0
    assert np.array_equal(depth[v], (3.0 / (disp[v] / 16.0)).astype(np.float32))


def test_grey_rule():
    k = SC.noise(4, 70, 1)
    assert np.array_equal(SD.to_grey_numpy(k), k)
    assert np.array_equal(SD.to_grey_numpy(np.stack([k] * 3, -1)), k)                    # equal channels: the channel
    assert np.array_equal(SD.to_grey_numpy(np.stack([k] * 3).astype(np.float64) / 255.0), k)
    rgb = np.zeros((1, 3, 3), np.uint8)
    rgb[0, 0, 0] = rgb[0, 1, 1] = rgb[0, 2, 2] = 255
    assert SD.to_grey_numpy(rgb).tolist() == [[76, 150, 29]]                              # 0.299, 0.587, 0.114


# ---- by hand ------------------------------------------------------------------------------------------------------------
def hand_prefilter(I):
    H, W = I.shape
    g = np.full((H, W), 15, np.int64)
    for y in range(H):
        for x in range(1, W - 1):
            up, dn = max(y - 1, 0), min(y + 1, H - 1)
            v = 2 * (int(I[y, x + 1]) - int(I[y, x - 1])) + (int(I[up, x + 1]) - int(I[up, x - 1])) \
                + (int(I[dn, x + 1]) - int(I[dn, x - 1]))
            g[y, x] = min(max(v, -15), 15) + 15
    return g


def hand_bt(a, b, y, x, d):
    W = a.shape[1]

    def bounds(A, i):
        u = int(A[y, i])
        ul, ur = (u + int(A[y, max(i - 1, 0)])) // 2, (u + int(A[y, min(i + 1, W - 1)])) // 2
        return u, min(u, ul, ur), max(u, ul, ur)

    u, u0, u1 = bounds(a, x)
    v, v0, v1 = bounds(b, x - d)
    return min(max(0, u - v1, v0 - u), max(0, v - u1, u0 - v)) >> 2


def hand_pixel_cost(L, R):
    H, W = L.shape
    gl, gr = hand_prefilter(L), hand_prefilter(R)
    pc = np.zeros((H, W, D), np.int64)
    for y in range(H):
        for x in range(D, W):
            for d in range(D):
                pc[y, x, d] = hand_bt(gl, gr, y, x, d) + hand_bt(L, R, y, x, d)
    return pc


def hand_block_cost(pc, r=10):
    H, W, _ = pc.shape
    C_ = np.zeros_like(pc)
    for y in range(H):
        for x in range(D, W):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    C_[y, x] += pc[min(max(y + dy, 0), H - 1), min(max(x + dx, D), W - 1)]
    return C_


def hand_path(C_, y, xs):
    """L along the pixels (y, x) for x in xs, each one's predecessor being the one before it."""
    out, prev = [], None
    for x in xs:
        c = C_[y, x]
        if prev is None:
            cur = c.copy()
        else:
            m = prev.min()
            cur = np.empty_like(c)
            for d in range(D):
                best = min(prev[d], m + 5)
                if d > 0:
                    best = min(best, prev[d - 1] + 2)
                if d < D - 1:
                    best = min(best, prev[d + 1] + 2)
                cur[d] = c[d] + best - m
        out.append(cur)
        prev = cur
    return out


@pytest.mark.parametrize("H,W", [(1, 66), (3, 67)])
def test_steps_against_hand_written_loops(H, W):
    """Fewer rows than the block and two or three valid columns: every clamp is in play."""
    L, R = SC.noise(H, W, 21), SC.noise(H, W, 22)
    pc = hand_pixel_cost(L, R)
    assert pc.max() <= 70 and pc[:, D:].max() > 0
    assert np.array_equal(SD.pixel_cost_numpy(L, R), pc)
    C_ = hand_block_cost(pc)
    assert np.array_equal(SD.block_cost_numpy(pc.astype(np.int32)), C_)
    # one path: left to right along the last row; the sum of the five at H = 1, where the three paths from above have
    # no predecessor and the right-to-left path is the same loop backwards
    y = H - 1
    fwd = hand_path(C_, y, range(D, W))
    for k, x in enumerate(range(D, W)):
        assert np.array_equal(SD.path_step_numpy(fwd[k - 1], C_[y, x]) if k else C_[y, x], fwd[k])
    if H == 1:
        bwd = hand_path(C_, 0, range(W - 1, D - 1, -1))[::-1]
        S = SD.aggregate_numpy(C_.astype(np.int32))
        for k, x in enumerate(range(D, W)):
            assert np.array_equal(S[0, x], fwd[k] + bwd[k] + 3 * C_[0, x])
        assert (S[:, :D] == 0).all()


def test_selection_by_hand():
    """One row, three valid columns, S written by hand: the tie rule, the sub-pixel formula with C division, uniqueness
    and the left-right vote."""
    W = D + 3
    S = np.full((1, W, D), 1000, np.int32)
    S[0, D, 7:10] = (140, 100, 120)          # b = 8: den = 60, num = 20*16 + 60 = 380, 380 // 120 = 3
    S[0, D + 1, 9:12] = (100, 90, 131)       # b = 10: den = 51, num = -31*16 + 51 = -445, C division: -(445 // 102) = -4
    S[0, D + 2, 5] = 90
    S[0, D + 2, 30] = 149                    # 149 * 60 < 90 * 100: not unique
    disp, not_unique, failed = SD.select_numpy(S, 40, return_flags=True)
    assert disp[0, D:].tolist() == [16 * 8 + 3, 16 * 10 - 4, -16]
    assert not_unique[0, D:].tolist() == [False, False, True] and not failed.any()
    S[0, D + 2, 30] = 150                    # 150 * 60 == 9000: unique again
    S[0, D + 2, 5:7] = 90                    # a tie: the smaller d; den = max(1000 + 90 - 180, 1), num = 910*16 + 910
    assert SD.select_numpy(S)[0, D + 2] == 16 * 5 + (910 * 17) // (2 * 910)
    # left-right: columns D and D + 2 vote into D - 8 and D - 6; give D + 1 the disparity 9 so that it votes into D - 8
    # with a smaller S and takes the column from D, whose candidates 8 and 9 (disp16 = 131) then face the vote 9
    S[0, D + 1] = 1000
    S[0, D + 1, 8:11] = (70, 50, 70)         # b = 9 exactly: disp16 = 144, x2 = D - 8
    disp, _, failed = SD.select_numpy(S, 40, return_flags=True)
    assert disp[0, D + 1] == 144 and disp[0, D] == 131 and not failed.any()      # candidate 9 looks at D - 9: no vote
    S[0, D, 7:10] = (140, 100, 140)          # b = 8 exactly: both candidates are 8 and face the vote 9: invalid
    disp, _, failed = SD.select_numpy(S, 40, return_flags=True)
    assert disp[0, D] == -16 and failed[0, D:].tolist() == [True, False, False]
    S[0, D, 7:10] = (100, 100, 1000)         # b = 7 by the tie rule, the parabola's minimum at 7.5: candidates 7 and 8
    disp, _, failed = SD.select_numpy(S, 40, return_flags=True)
    # D votes (100, 7) into D - 7; candidate 7 looks there and agrees: valid whatever D - 8 holds
    assert disp[0, D] == 16 * 7 + 8 and not failed.any()


# ---- the C ABI, host side -------------------------------------------------------------------------------------------------
def test_entry_points_and_argument_checks_without_a_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert {"mgs_stereo_scratch_bytes", "mgs_stereo_depth_args_size", "mgs_stereo_depth"} <= set(_cabi.EXPORTS)
    assert L.mgs_stereo_depth_args_size() == C.sizeof(_cabi.StereoDepthArgs) == 32 + 8 * 8
    assert L.mgs_stereo_scratch_bytes(480, 64) == 0 and L.mgs_stereo_scratch_bytes(0, 100) == 0
    assert L.mgs_stereo_scratch_bytes(480, 20000) == 0
    n = L.mgs_stereo_scratch_bytes(480, 752)
    vol = 480 * (752 - 64) * 64
    assert vol * 12 <= n <= vol * 12 + 480 * 752 * 32               # C and the five L in 16 bits, the rest per pixel
    assert L.mgs_stereo_depth(None, None) == -1
    a = _cabi.StereoDepthArgs()
    a.width, a.height, a.num_disparities, a.block_size, a.uniqueness_ratio = 100, 10, 64, 20, 40
    assert L.mgs_stereo_depth(C.byref(a), None) == -1               # null pointers: refused before anything is launched
    assert _cabi.ABI_VERSION == 10
