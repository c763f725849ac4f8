"""The NumPy mirror of stereo depth (monogs_amd/stereo_depth.py, DESIGN.md "Stereo depth on the device") without a GPU:
the planes property, the quirks of the reference's depth lines, the steps against hand-written loops at shapes smaller
than the block - the block cost at the half blocks 0, 1, 10, 13 and 14, the five paths pixel by pixel, the selection at
both ends of the uniqueness ratio - and the host-only side of the C ABI."""
import ctypes as C
import functools

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


def hand_step(prev, c):
    """One pixel of a path: L from the predecessor's L `prev` (None: no predecessor) and the pixel's C `c`."""
    if prev is None:
        return c.copy()
    m = prev.min()
    cur = np.empty_like(c)
    for d in range(D):
        best = min(prev[d], m + 5)
        if d > 0:
            best = min(best, prev[d - 1] + 2)
        if d < D - 1:
            best = min(best, prev[d + 1] + 2)
        cur[d] = c[d] + best - m
    return cur


def hand_path(C_, y, xs):
    """L along the pixels (y, x) for x in xs, each one's predecessor being the one before it."""
    out, prev = [], None
    for x in xs:
        cur = hand_step(prev, C_[y, x])
        out.append(cur)
        prev = cur
    return out


PRED = ((-1, 0), (1, 0), (-1, -1), (0, -1), (1, -1))         # the five predecessor offsets (dx, dy)


def hand_aggregate(C_):
    """S by five explicit loops over pixels, one per predecessor offset: each pixel's L from its predecessor's by
    `hand_path`'s recurrence; a predecessor outside [D, W) x [0, H) means L = C."""
    H, W, _ = C_.shape
    S = np.zeros_like(C_)
    for dx, dy in PRED:
        L = np.zeros_like(C_)
        for y in range(H):                                   # dy <= 0: the row above is done
            for x in (range(W - 1, D - 1, -1) if dx > 0 else range(D, W)):
                qx, qy = x + dx, y + dy
                inside = D <= qx < W and 0 <= qy < H
                L[y, x] = hand_step(L[qy, qx] if inside else None, C_[y, x])
        S += L
    return S


@functools.lru_cache(maxsize=None)
def hand_costs(H, W, bright=False):
    """(L, R, the hand-made pixel cost) of a noise pair at H x W, read-only: the loops run once per shape.  `bright`:
    the left image in 190..255 and the right in 0..65, so that most pixel costs are above 40 and a 29x29 block's sum
    passes 32 767."""
    L, R = SC.noise(H, W, 21), SC.noise(H, W, 22)
    if bright:
        L, R = ((a.astype(np.int64) * 66 // 256 + lift).astype(np.uint8) for a, lift in ((L, 190), (R, 0)))
    pc = hand_pixel_cost(L, R)
    pc.setflags(write=False)
    return L, R, pc


@pytest.mark.parametrize("r", [0, 1, 10, 14])
@pytest.mark.parametrize("H,W", [(1, 66), (3, 67), (5, 69)])
def test_steps_against_hand_written_loops(H, W, r):
    """Fewer rows than the block and two to five valid columns: every clamp is in play, at the smallest half blocks
    (r = 0: the pixel cost itself), the reference's and the largest the device takes."""
    L, R, pc = hand_costs(H, W)
    assert pc.max() <= 70 and pc[:, D:].max() > 0
    assert np.array_equal(SD.pixel_cost_numpy(L, R), pc)
    C_ = hand_block_cost(pc, r)
    got = SD.block_cost_numpy(pc.astype(np.int32), r)
    assert got.dtype == np.int32 and np.array_equal(got, C_)
    if r == 0:
        assert np.array_equal(C_, pc)
    assert (C_[:, :D] == 0).all() and C_.max() <= (2 * r + 1) ** 2 * 70
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


@pytest.mark.parametrize("r", [13, 14])
def test_block_cost_above_32767_against_hand_written_loops(r):
    """From r = 11 a block cost can pass 32 767, the half of the 16 bits the device keeps it in: on a bright left and a
    dark right image (pixel costs of about 50) a quarter of it does at r = 13 and all of it at r = 14, and the mirror
    must carry it unharmed."""
    L, R, pc = hand_costs(5, 69, bright=True)
    assert np.array_equal(SD.pixel_cost_numpy(L, R), pc)
    C_ = hand_block_cost(pc, r)
    share = (C_[:, D:] > 32767).mean()
    print("r", r, "C.max()", C_.max(), "share above 32 767", share)
    assert share > 0.2 and C_.max() + 5 <= 65535             # any entry up there shows a store that truncates
    got = SD.block_cost_numpy(pc.astype(np.int32), r)
    assert got.dtype == np.int32 and np.array_equal(got, C_)


@pytest.mark.parametrize("r", [1, 14])
@pytest.mark.parametrize("H,W,bright", [(5, 69, False), (9, 67, False), (5, 69, True)])
def test_five_paths_against_hand_written_loops(H, W, r, bright):
    """aggregate_numpy against five loops over pixels, one per predecessor offset: more rows than valid columns at
    9x67, so that the diagonal paths start from the side as well as from the top row, and the predecessors at the left
    and the right valid column are outside for one diagonal each.  `bright` at r = 14: L above 32 767."""
    C_ = SD.block_cost_numpy(hand_costs(H, W, bright)[2].astype(np.int32), r)
    if bright and r == 14:
        assert (C_[:, D:] > 32767).mean() > 0.5
    want = hand_aggregate(C_.astype(np.int64))
    # the hand loops took every branch: pixels with and without a predecessor in each of the five directions
    for dx, dy in PRED:
        has = [D <= x + dx < W and 0 <= y + dy < H for y in range(H) for x in range(D, W)]
        assert any(has) and not all(has)
    S = SD.aggregate_numpy(C_)
    assert np.array_equal(S, want) and (S[:, :D] == 0).all()
    assert (S[:, D:] >= 5 * C_[:, D:]).all() and (S[:, D:] <= 5 * (C_[:, D:] + 5)).all()


def disp16_with_a_faulty_16_bit_c(name, H, W):
    """disp16 at r = 14 and ratio 0 from the mirror's C of a pair: as it is, as a signed 16-bit read of the device's
    uint16_t volume would give it, and with bit 15 dropped; and C's valid columns."""
    C_ = SC.mirror_block_cost(name, H, W, 14)
    signed = C_.astype(np.uint16).view(np.int16).astype(np.int32)
    disp = [SD.select_numpy(SD.aggregate_numpy(c), 0) for c in (C_, signed, C_ & 0x7fff)]
    assert np.array_equal(disp[0], SC.mirror(name, H, W, blockSize=29, uniquenessRatio=0)[0])
    return disp, C_[:, D:]


@pytest.mark.parametrize("name", ["straddle_low", "straddle_high"])
@pytest.mark.parametrize("H,W", [(37, 203), (33, 129)])
def test_the_straddling_pairs_show_a_wrong_read_of_bit_15(name, H, W):
    """What makes the device's straddling cases (tests/test_gpu_stereo_depth.py) worth running, simulated on the mirror:
    with a pixel's 64 disparities on both sides of 32 768, a signed read of C, or a store without bit 15, moves the
    argmin or the sub-pixel term of most pixels.  Measured, entries of disp16 that change (the same count for both
    faults): 4387 and 4669 of 7511 at 37x203, 1837 and 1785 of 4257 at 33x129."""
    (disp, signed, dropped), Cv = disp16_with_a_faulty_16_bit_c(name, H, W)
    above = Cv > 32767
    both = above.any(-1) & ~above.all(-1)
    n = [(d != disp).sum() for d in (signed, dropped)]
    print(name, H, W, "share above 32 767", above.mean(), "pixels on both sides", both.sum(), "of", both.size,
          "disp16 entries a signed read changes", n[0], "a dropped bit 15", n[1])
    assert 0.1 < above.mean() < 0.9 and 2 * both.sum() > both.size
    assert min(n) > 1000


@pytest.mark.parametrize("H,W", [(37, 203), (33, 129)])
def test_the_all_above_pair_does_not(H, W):
    """At lift 190 every valid entry of C has bit 15 set, so either fault shifts a pixel's 64 costs alike: the path
    recurrence adds C to a difference of L's, the selection compares S within a pixel, ratio 0 rejects nothing - disp16
    does not move.  That pair exercises large values (carries of the packed adds, 19-bit S), not the sign."""
    (disp, signed, dropped), Cv = disp16_with_a_faulty_16_bit_c("offset", H, W)
    assert Cv.min() > 32767
    assert np.array_equal(signed, disp) and np.array_equal(dropped, disp)


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
    # the ends of the ratio, S[d] * (100 - ratio) < S[b] * 100 for a far d.  Minima at 5, 20 and 40 with both neighbours
    # at 1000 (sub-pixel term 0) vote into three different columns, so the left-right check passes everything
    S = np.full((1, W, D), 1000, np.int32)
    S[0, D, 5], S[0, D, 30] = 100, 101       # ratio 1: 101 * 99 = 9999 < 10000, not unique; ratio 0: 10100 < 10000 never
    S[0, D + 1, 20], S[0, D + 1, 50] = 99, 100       # ratio 1: 100 * 99 == 99 * 100, unique
    S[0, D + 2, 40], S[0, D + 2, 60] = 0, 0  # sb == 0: 0 < 0 at every ratio, unique; the tie goes to the smaller d
    for ratio, want, flags in ((0, [80, 320, 640], [False, False, False]), (1, [-16, 320, 640], [True, False, False]),
                               (99, [-16, -16, 640], [True, True, False]), (100, [-16, -16, 640], [True, True, False])):
        disp, not_unique, failed = SD.select_numpy(S, ratio, return_flags=True)
        assert disp[0, D:].tolist() == want and not_unique[0, D:].tolist() == flags and not failed.any(), ratio
    S[0, D:, :] = 1                          # ratio 100 rejects every pixel with sb > 0, however flat its S is ...
    disp, not_unique, _ = SD.select_numpy(S, 100, return_flags=True)
    assert (disp == -16).all() and not_unique[0, D:].all()
    assert SD.select_numpy(S, 0)[0, D:].tolist() == [0, 0, 0]          # ... and ratio 0 none: b = 0 by the tie rule


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
