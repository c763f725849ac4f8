"""CPU tests of the RGB-D alignment's contract (monogs_amd/icp.py: intensity_planes_torch, icp_rows_numpy(photo=),
align_numpy(image=, photo_weight=) - the mirrors of k_icp_intensity and k_icp_rows_rgbd): the textured plane moves from
degenerate to converged, the textured wavy scene is no worse than geometry alone, the photometric Jacobian against finite
differences of the residual, the guards with their counters, the int64 bound, the defaults against the bytes of the commit
before, and the C ABI's refusals.  No test needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import icp_cases as IC
import icp_rgbd_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_parent_defaults.npz")
EYE = np.eye(4, dtype=np.float32)

# what align_numpy(image=, photo_weight=1) measured on the textured plane (one stride-1 level): 1.19e-4 m, 9.9e-3 degrees;
# on the textured wavy scene 8.8e-5 m, below 1e-6 degrees (geometry alone: 1.66e-4 m, 8.6e-3 degrees)
PLANE_T, PLANE_R_DEG = 1.19e-4, 9.9e-3
WAVY_T, WAVY_R_DEG = 8.9e-5, 1e-3


# ---- 1. the textured plane: degenerate -> converged -------------------------------------------------------------------
def test_textured_plane_moves_from_degenerate_to_converged():
    """The allowed pose error is twice what the mirror measured, under icp_cases' caps (half a voxel, half a degree), which
    lie below the start error by construction."""
    from monogs_amd import icp
    start = IC.pose_error(np.eye(4), RC.plane_pose())
    print(f"start: {start[0]:.4f} m, {start[1]:.3f} degrees")
    assert start[0] > IC.CAP_T and start[1] > IC.CAP_R_DEG and abs(start[0] - 0.0361) < 1e-4 and abs(start[1] - 2.005) < 0.01
    geo = RC.plane_mirror(0.0, ((1, 10),))
    info = geo["info"]
    print("photo_weight 0:", info["status_name"], info["pivots"], info["counts"])
    assert info["status"] == icp.DEGENERATE and not info["ok"] and info["iterations_run"] == 1
    assert [float(p) == 0.0 for p in info["pivots"]] == [True, True, False, False, False, True]          # exactly three, exactly 0
    assert "photo" not in info and np.array_equal(geo["T_w2c"], EYE) and not geo["record"][52:].any()
    for levels in (((1, 10),), icp.LEVELS):
        one = RC.plane_mirror(RC.PHOTO_WEIGHT, levels)
        info = one["info"]
        et, er = IC.pose_error(one["T_w2c"], RC.plane_pose())
        h = icp.read_history(one["history"], rgbd=True)
        ran = info["iterations_run"]
        diag = max(int(info["sums"][icp.tri(i, i)]) / 2.0 ** 30 for i in range(6))
        print(f"photo_weight {RC.PHOTO_WEIGHT}, {levels}: {info['status_name']} after {ran}, {et:.3e} m, {er:.3e} degrees, geometric "
              f"{info['counts']}, photometric {info['photo']}, pivots {info['pivots']}, sum r_I^2 {h['sum_ri2'][h['ran'] == 1]}")
        assert info["status"] == icp.CONVERGED and info["ok"]
        assert np.all(info["pivots"] > 1e-6 * diag)                                                      # all six pass
        assert et <= 2 * PLANE_T and er <= 2 * PLANE_R_DEG and et <= IC.CAP_T and er <= IC.CAP_R_DEG
        assert info["photo"]["accepted"] > 2500 and info["photo"]["bound"] == 0
        # every pixel that passed steps 1 - 4 is in exactly one photometric counter, whatever steps 5 - 7 said of it
        passed = IC.H * IC.W - info["counts"]["invalid"] - info["counts"]["range"] - info["counts"]["outside"]
        assert sum(info["photo"].values()) == passed and sum(info["counts"].values()) == IC.H * IC.W
        first = np.flatnonzero(h["ran"] == 1)
        assert h["sum_ri2"][first[-1]] < 0.01 * h["sum_ri2"][first[0]] and info["sum_ri2"] == h["sum_ri2"][first[-1]]
        assert not h["sum_ri2"][h["ran"] == 0].any()


# ---- 2. the textured wavy scene ---------------------------------------------------------------------------------------
def test_textured_wavy_scene_is_no_worse_than_geometry_alone():
    from monogs_amd import icp
    geo = IC.recovery_mirror(((1, 10),))
    gt, gr = IC.pose_error(geo["T_w2c"], IC.true_pose())
    both = RC.wavy_mirror(RC.PHOTO_WEIGHT, ((1, 10),))
    et, er = IC.pose_error(both["T_w2c"], IC.true_pose())
    info = both["info"]
    print(f"geometry alone {gt:.3e} m, {gr:.3e} degrees; RGB-D {et:.3e} m, {er:.3e} degrees, {info['status_name']} after "
          f"{info['iterations_run']}, geometric {info['counts']}, photometric {info['photo']}")
    assert info["status"] == icp.CONVERGED and et <= gt and er <= gr
    assert et <= 2 * WAVY_T and er <= 2 * WAVY_R_DEG and et <= IC.CAP_T and er <= IC.CAP_R_DEG
    # the geometric row and its seven counters are today's: the first iteration starts from the same D
    s0, c0 = icp.icp_rows_numpy(IC.model_planes(), IC.frame_depth(), IC.sensor_normal(), np.eye(4)[:3], IC.INTR)
    photo = {"sensor": both["intensity"], "model": both["model_intensity"], "weight": RC.PHOTO_WEIGHT}
    s1, c1, extra = icp.icp_rows_numpy(RC.wavy_model(), IC.frame_depth(), IC.sensor_normal(), np.eye(4)[:3], IC.INTR, photo=photo)
    s2, c2, extra2 = icp.icp_rows_numpy(RC.wavy_model(), IC.frame_depth(), IC.sensor_normal(), np.eye(4)[:3], IC.INTR,
                                        photo=dict(photo, weight=0.0))
    assert np.array_equal(c0, c1) and np.array_equal(c0, c2) and np.array_equal(s0, s2) and not np.array_equal(s0, s1)
    assert extra[0] > 2000 and extra2[0] == extra[0] and extra2[3] == extra[3]      # lambda = 0: rows of zeros, still counted


# ---- 3. the photometric Jacobian ---------------------------------------------------------------------------------------
def _one_pixel(v, u, D, model, image, intr=IC.INTR):
    """The photometric row of the single sensor pixel (v, u) out of the mirror: every other depth is 0 (INVALID) and the
    model normals are 0 (NO_MODEL: no geometric row), so with lambda = 1 the sums ARE w_i w_j of that one row."""
    from monogs_amd import icp
    depth = torch.zeros(IC.H, IC.W)
    depth[v, u] = RC.PLANE_Z
    bare = {"depth": model["depth"], "normal": torch.zeros(IC.H, IC.W, 3), "color": model["color"]}
    photo = {"sensor": icp.intensity_planes_torch(image), "model": icp.intensity_planes_torch(model["color"], valid=model["depth"]),
             "weight": 1.0}
    sums, counts, extra = icp.icp_rows_numpy(bare, depth, IC.plane_sensor_normal(), D, intr, photo=photo)
    assert counts[0] == 0 and counts[4] == 1 and extra[0] == 1, (counts, extra)
    return np.array([int(sums[icp.tri(i, 6)]) for i in range(7)]) / 2.0 ** 30, photo      # J_i r (i < 6), r^2


def _residual_fp64(xi, v, u, D, photo, intr=IC.INTR):
    """r_I of pixel (v, u) after D <- Exp(xi) D, in fp64: the bilinear sample of the mirror's model plane minus I_s."""
    E = IC.pose(xi)[:3]
    fx, fy, cx, cy = intr
    X = np.array([(u - cx) / fx * RC.PLANE_Z, (v - cy) / fy * RC.PLANE_Z, RC.PLANE_Z])
    p = D[:, :3] @ X + D[:, 3]
    p = E[:, :3] @ p + E[:, 3]
    x, y = fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    I = photo["model"][0].numpy().astype(np.float64)
    ax, ay = x - x0, y - y0
    top, bot = I[y0, x0] + ax * (I[y0, x0 + 1] - I[y0, x0]), I[y0 + 1, x0] + ax * (I[y0 + 1, x0 + 1] - I[y0 + 1, x0])
    return top + ay * (bot - top) - float(photo["sensor"][0][v, u]), (ax, ay)


def test_photometric_jacobian_against_finite_differences():
    """On an intensity RAMP I = 0.2 + 0.006 x + 0.004 y (in model pixels) the bilinear sample and the central difference are
    exact, so the finite difference of the fp64 residual and the mirror's fp32 row differ by roundings alone.  The
    allowance, relative to the largest |J_i| of the row: the ramp's fp32 values are off by 2^-25 each, which a slope over
    one pixel returns as 2 * 2^-25 / 0.004 = 1.5e-5 of the slope; the row's own chain of about ten fp32 roundings adds 10 *
    2^-24 = 6e-7; the fixed-point truncation of J_i r at r >= 0.02 adds 2^-30 / 0.02 = 5e-8 absolute, below 2e-7 of |J| >=
    0.3; the central difference with h = 1e-5 is off by h^2 |r'''| / 6, nothing here.  1.5e-5 + 6e-7 + 2e-7, taken as 2e-5.
    The sensor image is a constant 0.25 in both cases, so |r| >= 0.02 everywhere.
    On the smooth texture the two differ by the discretisation (the central difference over two pixels against the slope
    of one cell): at most one pixel times the largest second derivative, 0.2 * 0.587 * (5.6 * 0.025)^2 + ... < 0.2 *
    (6.9 * 0.025)^2 = 6e-3 per pixel^2 against slopes of up to 0.2 * 6.9 * 0.025 = 0.035 per pixel - so there only the
    sign and the size are held, to 25 % of the largest |J_i|."""
    from monogs_amd import icp
    vv, uu = np.meshgrid(np.arange(IC.H, dtype=np.float64), np.arange(IC.W, dtype=np.float64), indexing="ij")
    ramp = np.repeat((0.2 + 0.006 * uu + 0.004 * vv)[..., None], 3, -1).astype(np.float32)
    model = {"depth": torch.full((IC.H, IC.W), RC.PLANE_Z), "color": torch.from_numpy(ramp)}
    image = torch.full((3, IC.H, IC.W), 0.25)
    D = IC.pose((0.011, -0.007, 0.004, 0.01, -0.008, 0.02))[:3]
    h = 1e-5
    for name, model_, image_, tol in (("ramp", model, image, 2e-5), ("texture", RC.plane_model(), image, 0.25)):
        worst = 0.0
        for v, u in ((7, 9), (22, 34), (30, 55), (12, 61), (38, 20)):
            row, photo = _one_pixel(v, u, D, model_, image_)
            r0, (ax, ay) = _residual_fp64(np.zeros(6), v, u, D, photo)
            assert 0.02 < ax < 0.98 and 0.02 < ay < 0.98, "the finite difference must stay inside one cell"
            assert abs(r0) >= 0.02 and abs(row[6] - r0 * r0) <= 2.0 ** -30 + 4 * 2.0 ** -23 * abs(r0)
            J = row[:6] / r0
            fd = np.zeros(6)
            for i in range(6):
                e = np.zeros(6)
                e[i] = h
                fd[i] = (_residual_fp64(e, v, u, D, photo)[0] - _residual_fp64(-e, v, u, D, photo)[0]) / (2 * h)
            err = np.abs(J - fd).max() / np.abs(fd).max()
            print(f"{name} ({v},{u}): r {r0:+.4f}, J {J}, finite difference {fd}, relative difference {err:.2e}")
            worst = max(worst, err)
            assert np.abs(fd).max() > 0.1
        assert worst <= tol, (name, worst)


# ---- 4. guards and counters -------------------------------------------------------------------------------------------
def test_intensity_planes_mark_what_is_invalid():
    from monogs_amd import icp
    rgb = RC.plane_frame()[1].clone()
    rgb[0, 5, 7] = 1.5                       # a colour outside [0, 1]
    rgb[1, 20, 30] = float("nan")
    rgb[2, 31, 40] = float("inf")
    rgb[1, 10, 50] = -1e-3
    valid = torch.ones(IC.H, IC.W)
    valid[40, 3], valid[15, 15] = 0.0, float("nan")
    P = icp.intensity_planes_torch(rgb, valid).numpy()
    bad = [(5, 7), (20, 30), (31, 40), (10, 50), (40, 3), (15, 15)]
    I, gx, gy = P
    for y, x in bad:
        assert I[y, x] == icp.NO_INTENSITY and gx[y, x - 1] == gx[y, x + 1] == icp.NO_GRADIENT and gy[y - 1, x] == gy[y + 1, x] == icp.NO_GRADIENT
        assert gx[y, x] != icp.NO_GRADIENT and gy[y, x] != icp.NO_GRADIENT          # its own gradient needs its neighbours only
    assert int((I == icp.NO_INTENSITY).sum()) == len(bad)
    assert bool((gx[:, 0] == 2).all() and (gx[:, -1] == 2).all() and (gy[0] == 2).all() and (gy[-1] == 2).all())      # the border
    assert int((gx == 2).sum()) == 2 * IC.H + 2 * len(bad) and int((gy == 2).sum()) == 2 * IC.W + 2 * len(bad)
    ok = I >= 0
    assert I[ok].min() >= 0.29 and I[ok].max() <= 0.71 and np.abs(gx[gx != 2]).max() < 0.03
    # the arithmetic, and both layouts
    r, g, b = (rgb[c].numpy() for c in range(3))
    want = (np.float32(0.299) * r + np.float32(0.587) * g) + np.float32(0.114) * b
    assert np.array_equal(I[ok], want[ok]) and np.array_equal(gx[3, 4], np.float32(0.5) * (want[3, 5] - want[3, 3]))
    assert np.array_equal(icp.intensity_planes_torch(rgb.permute(1, 2, 0).contiguous(), valid).numpy(), P, equal_nan=True)
    # white is valid: I <= 1 + 2^-22, no mark
    white = icp.intensity_planes_torch(torch.ones(3, 4, 5)).numpy()
    assert 1.0 - 2.0 ** -22 <= white[0].min() and white[0].max() <= 1.0 + 2.0 ** -22 and white[1, 1, 1] == 0.0
    for shape in ((4, 5), (2, 4, 5), (4, 5, 4)):
        with pytest.raises(ValueError, match="RGB"):
            icp.intensity_planes_torch(torch.zeros(shape))


def test_photometric_guards_and_counters():
    from monogs_amd import icp
    depth, image, sn = RC.plane_frame()
    model = RC.plane_model()
    D = np.asarray(icp.initial_transform(EYE, RC.plane_pose().astype(np.float32)))
    D0 = np.eye(4)[:3].copy()

    def rows(model_=model, image_=image, depth_=depth, D_=D0, weight=1.0, **kw):
        photo = {"sensor": icp.intensity_planes_torch(image_), "model": icp.intensity_planes_torch(model_["color"], valid=model_["depth"]),
                 "weight": weight}
        sums, counts, extra = icp.icp_rows_numpy(model_, depth_, sn, D_, IC.INTR, photo=photo, **kw)
        passed = int(counts[0] + counts[4:].sum())
        assert int(extra[:3].sum()) == passed and int(counts.sum()) == IC.H * IC.W, (counts, extra)
        return sums, counts, extra

    _, c0, e0 = rows()
    print("clean", c0, e0)
    assert c0[0] == IC.H * IC.W and e0[0] == (IC.H - 2) * (IC.W - 2) - (IC.H - 2) - (IC.W - 3) and e0[2] == 0
    # a colour outside [0, 1] and a NaN in the sensor image: one photometric row each, the geometric rows stay
    bad = image.clone()
    bad[0, 10, 10], bad[2, 20, 20] = 1.01, float("nan")
    _, c, e = rows(image_=bad)
    assert np.array_equal(c, c0) and e[1] == e0[1] + 2 and e[0] == e0[0] - 2
    # a missing neighbour in the model: the hole, and the gradients beside it, take out every sample that touches them
    holed = dict(model, color=model["color"].clone())
    holed["color"][22, 33, 1] = float("nan")
    _, c, e = rows(model_=holed)
    assert np.array_equal(c, c0) and e[1] == e0[1] + 12 and e[0] == e0[0] - 12          # the 4 x 4 cells around it less the corners
    # ... and a model without depth there has neither row
    nodepth = dict(model, depth=model["depth"].clone())
    nodepth["depth"][22, 33] = 0.0
    _, c, e = rows(model_=nodepth)
    assert c[4] == 1 and c[0] == c0[0] - 1 and e[1] == e0[1] + 12
    # a steep gradient at p_z = 0.05: fx / p_z = 1200 against 16
    near = torch.full((IC.H, IC.W), 0.05)
    near_model = dict(model, depth=near)
    _, c, e = rows(model_=near_model, depth_=near, depth_max=1.0)
    print("near", c, e)
    # |gx| fx / p_z >= 16 wherever |gx| >= 0.0133 per pixel, of slopes of up to 0.035: more than a tenth of the rows
    assert e[2] > e0[0] // 10 and e[0] + e[2] == e0[0] and c[0] == IC.H * IC.W          # the geometric row still counts
    s_geo, c_geo = icp.icp_rows_numpy(near_model, near, sn, D0, IC.INTR, depth_max=1.0)
    s_both, _, _ = rows(model_=near_model, depth_=near, depth_max=1.0, weight=1e-3)
    assert c_geo[0] == c[0] and not np.array_equal(s_geo, s_both)
    # hostile D: nothing is indexed out of bounds (NumPy would raise), every pixel is counted once
    for name, edit in (("nan", lambda M: M.__setitem__((0, 1), np.nan)), ("inf", lambda M: M.__setitem__((2, 3), np.inf)),
                       ("huge", lambda M: M.__setitem__((slice(None), 3), 1e30)), ("huge_all", lambda M: M.__imul__(3e38)),
                       ("behind", lambda M: M.__setitem__((2, 2), -1.0)), ("aside", lambda M: M.__setitem__((0, 3), 1.2)),
                       ("edge", lambda M: M.__setitem__((0, 3), 0.8375))):
        M = D0.copy()
        edit(M)
        s, c, e = rows(D_=M, dist=8.0, cos_min=-1.0, depth_max=16.0)
        print(name, c, e)
        assert e[0] <= e0[0]
        if name in ("aside", "edge"):
            assert c[3] > 0 and e[0] > 0
    # a hostile photo_weight is refused, the planes must fit
    for w in (-1.0, float("nan"), 1025.0, float("inf")):
        with pytest.raises(ValueError, match="photo_weight"):
            icp.align_numpy(model, depth, IC.INTR, EYE, image=image, photo_weight=w)
        with pytest.raises(ValueError, match="photo_weight"):
            icp.align(model, depth, IC.INTR, EYE, image=image, photo_weight=w)
    for call in (icp.align_numpy, icp.align):
        with pytest.raises(ValueError, match="RGB"):
            call(model, depth, IC.INTR, EYE, image=torch.zeros(3, IC.H, IC.W + 1), photo_weight=1.0)
        with pytest.raises(ValueError, match="colour"):
            call({k: v for k, v in model.items() if k != "color"}, depth, IC.INTR, EYE, image=image, photo_weight=1.0)
        with pytest.raises(ValueError, match="RGB"):
            call(dict(model, color=torch.zeros(IC.H, IC.W)), depth, IC.INTR, EYE, image=image, photo_weight=1.0)


def test_a_volume_without_colour_is_refused():
    from monogs_amd import icp

    class Bare:
        has_color = False

        def raycast(self, *a, **k):
            raise AssertionError("refused before the ray cast")

    depth, image, _ = RC.plane_frame()
    with pytest.raises(ValueError, match="colour"):
        icp.track_against_volume(Bare(), depth, torch.eye(4), (torch.eye(4), *IC.INTR, IC.H, IC.W), image=image, photo_weight=1.0)


# ---- 5. the bound -----------------------------------------------------------------------------------------------------
def test_two_rows_per_pixel_stay_below_2_to_the_63():
    """A pixel adds at most one geometric product, below 2^10 (|J_i|, |r| < 2^5), and one photometric product, below 16 * 16
    = 2^8 by the gate: (2^10 + 2^8) 2^30 per pixel, 2^22 pixels.  The worst-case plane: p_z = 0.11 puts fx / p_z = 545 on
    a ramp of 0.029 per pixel, so |w_0| = 15.8 passes the gate in every pixel that has a row; its largest sum, scaled from
    its pixel count to 2^22 pixels, must stay below 2^63 as well."""
    from monogs_amd import icp
    assert (2 ** 10 + 2 ** 8) * 2 ** 30 * icp.MAX_PIXELS < 2 ** 63 and icp.MAX_PIXELS == 2 ** 22 and icp.PHOTO_BOUND == 16.0
    assert (2 ** 10 + 2 * 2 ** 8) * 2 ** 30 * icp.MAX_PIXELS < 2 ** 63 <= (2 ** 10 + 2 ** 10) * 2 ** 30 * icp.MAX_PIXELS      # |w| < 32 would not do
    vv, uu = np.meshgrid(np.arange(IC.H, dtype=np.float64), np.arange(IC.W, dtype=np.float64), indexing="ij")
    ramp = np.repeat((0.05 + 0.029 * uu * 0.4)[..., None], 3, -1).astype(np.float32)
    z = 0.11
    near = torch.full((IC.H, IC.W), z)
    model = {"depth": near, "normal": RC.plane_model()["normal"], "color": torch.from_numpy(ramp)}
    image = torch.zeros(3, IC.H, IC.W)
    photo = {"sensor": icp.intensity_planes_torch(image), "model": icp.intensity_planes_torch(model["color"], valid=near), "weight": 2.5}
    D = np.eye(4)[:3].copy()
    D[0, 3] = 0.3 * z / 60.0                                     # a third of a pixel: samples inside the cells
    sums, counts, extra = icp.icp_rows_numpy(model, near, IC.plane_sensor_normal(), D, IC.INTR, photo=photo, depth_max=1.0)
    w0 = np.sqrt(int(sums[0]) / 2.0 ** 30 / max(int(extra[0]), 1))      # sums[0] = sum w_0^2 (n_0 = 0)
    print(counts, extra, "rms w_0", w0, "largest sum / 2^30", np.abs(sums).max() / 2.0 ** 30)
    assert extra[2] == 0 and extra[0] == (IC.H - 3) * (IC.W - 3) and 15.0 < w0 < 16.0      # at the gate, and through it
    per_pixel = int(np.abs(sums).max()) / int(extra[0])
    assert per_pixel < (2 ** 10 + 2 ** 8) * 2 ** 30 and per_pixel * icp.MAX_PIXELS < 2 ** 63
    assert int(extra[3]) / int(extra[0]) <= (1 + 2.0 ** -21) ** 2 * 2 ** 30


# ---- 6. defaults ------------------------------------------------------------------------------------------------------
def test_defaults_are_the_old_path():
    """align_numpy and icp_rows_numpy without `image` against what they returned on the commit before (golden/
    make_icp_parent_defaults.py): the same dict keys, the same bytes - also with an image but photo_weight = 0, and with
    photo_weight but no image."""
    from monogs_amd import icp
    G = np.load(GOLDEN)
    levels = ((2, 2), (1, 3))
    for extra in ({}, dict(image=RC.wavy_image()), dict(photo_weight=2.0), dict(image=None, photo_weight=0.0)):
        r = icp.align_numpy(RC.wavy_model(), IC.frame_depth(), IC.INTR, EYE, levels=levels, sensor_normal=IC.sensor_normal(), **extra)
        assert ",".join(sorted(r)) == str(G["keys"]) and ",".join(sorted(r["info"])) == str(G["info_keys"]), extra
        for k in ("record", "history", "D", "T_w2c"):
            assert r[k].dtype == G["recovery_" + k].dtype and r[k].tobytes() == G["recovery_" + k].tobytes(), (extra, k)
    model, depth, kw, _ = IC.status_cases()["degenerate"]
    r = icp.align_numpy(model, depth, IC.INTR, EYE, levels=levels, **kw)
    for k in ("record", "history", "D", "T_w2c"):
        assert r[k].tobytes() == G["degenerate_" + k].tobytes(), k
    out = icp.icp_rows_numpy(IC.model_planes(), IC.patched_depth(), IC.sensor_normal(), np.eye(4)[:3], IC.INTR, stride=3)
    assert len(out) == 2 and out[0].tobytes() == G["rows_sums"].tobytes() and out[1].tobytes() == G["rows_counts"].tobytes()
    assert sorted(icp.read_history(r["history"])) == ["accepted", "iteration", "level", "ran", "status", "sum_r2", "xx"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_icp_rgbd_args_size() == C.sizeof(_cabi.IcpRgbdArgs) == 248 + 16 + 32
    assert L.mgs_icp_intensity_args_size() == C.sizeof(_cabi.IcpIntensityArgs) == 40
    assert L.mgs_icp_args_size() == 248 and L.mgs_struct_size(len(_cabi.struct_mirrors())) == -1      # the old list ends where it ended
    assert _cabi.ICP_RGBD_SUMS == _cabi.ICP_SUMS + 4 and _cabi.ICP_RECORD_WORDS == 56
    assert L.mgs_icp_rgbd_scratch_bytes(0) == 8 * _cabi.ICP_ROWS_BLOCKS * _cabi.ICP_RGBD_SUMS
    assert L.mgs_icp_rgbd_scratch_bytes(19) == L.mgs_icp_rgbd_scratch_bytes(0) + 19 * 8 * _cabi.ICP_HISTORY_WORDS
    assert L.mgs_icp_rgbd_scratch_bytes(-1) == 0 and L.mgs_icp_rgbd_scratch_bytes(1025) == 0
    assert L.mgs_icp_align_rgbd(None, None) == -1 and L.mgs_icp_intensity(None, None) == -1

    def args(**kw):
        r = _cabi.IcpRgbdArgs()
        a = r.icp
        a.width, a.height, a.model_width, a.model_height, a.num_levels = 70, 45, 70, 45, 1
        a.stride[0], a.iterations[0] = 1, 2
        a.fx = a.fy = a.mfx = a.mfy = 60.0
        a.dist, a.cos_min, a.depth_max, a.min_pivot_ratio, a.converged = 0.1, 0.8, 10.0, 1e-6, 1e-4
        for n in ("depth", "normal", "model_depth", "model_normal", "T_model", "scratch", "T_w2c", "D", "record"):
            setattr(a, n, 4096)                # never dereferenced: every call below is refused first
        for n in ("image", "model_color", "intensity", "model_intensity"):
            setattr(r, n, 4096)
        r.photo_weight = 1.0
        for k, v in kw.items():
            setattr(a if hasattr(a, k) else r, k, v)
        return r

    bad = [dict(image=None), dict(model_color=None), dict(intensity=None), dict(model_intensity=None), dict(image_chw=2),
           dict(model_color_chw=-1), dict(photo_weight=-0.5), dict(photo_weight=float("nan")), dict(photo_weight=1024.5),
           dict(photo_weight=float("inf")), dict(depth=None), dict(record=None), dict(width=0), dict(dist=8.5), dict(num_levels=0),
           dict(scratch=4100)]
    for kw in bad:
        assert L.mgs_icp_align_rgbd(C.byref(args(**kw)), None) == -1, kw
    assert L.mgs_icp_align_rgbd(C.byref(args(width=4096, height=1025)), None) == -3
    assert L.mgs_icp_align_rgbd(C.byref(args(model_width=40000, model_height=20000)), None) == -3

    def iargs(**kw):
        a = _cabi.IcpIntensityArgs()
        a.width, a.height, a.rgb, a.out = 70, 45, 4096, 4096
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw in (dict(rgb=None), dict(out=None), dict(width=0), dict(height=-1), dict(chw=2)):
        assert L.mgs_icp_intensity(C.byref(iargs(**kw)), None) == -1, kw
    assert L.mgs_icp_intensity(C.byref(iargs(width=40000, height=20000)), None) == -3
