"""CPU tests of the frame-to-model ICP's contract (monogs_amd/icp.py: the NumPy mirrors of csrc/icp.hip): the rows against
an independent fp64 evaluation, the solve against numpy.linalg.solve, the polynomial exponential against pose.SE3_exp,
recovery of a known motion on the wavy scene, the degenerate and failure statuses with their counters, the guards, and
the C ABI's refusals.  No test needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_cases as IC

U32 = 2.0 ** -24          # fp32 unit roundoff
EPS64 = 2.0 ** -52


# ---- 1. rows ----------------------------------------------------------------------------------------------------------
def hand_case():
    """A 4 x 5 sensor plane against a 6 x 7 model plane, every number written out."""
    depth = np.array([[1.50, 1.52, 1.49, 1.51, 1.53],
                      [1.48, 1.50, 1.52, 0.00, 1.50],
                      [1.51, 1.49, 1.50, 1.52, 1.48],
                      [1.50, 1.51, 1.53, 1.49, 9.00]], np.float32)
    sn = np.zeros((3, 4, 5), np.float32)
    sn[0], sn[1], sn[2] = 0.10, -0.05, -0.99
    sn[:, 0, 0] = 0.0                                                  # no normal: invalid
    sn[:, 2, 2] = (0.8, 0.0, 0.6)                                      # faces away: the normal gate
    md = np.full((6, 7), 1.5, np.float32)
    md[2, 3] = 0.0                                                     # no model there
    md[3, 4] = 1.9                                                     # too far: the distance gate
    mn = np.zeros((6, 7, 3), np.float32)
    mn[..., 0], mn[..., 1], mn[..., 2] = 0.12, 0.07, -0.98
    mn[1, 4] = (-0.2, 0.1, -0.97)
    c, s = 0.9992, 0.04
    D = np.array([[c, 0.0, s, 0.01], [0.0, 1.0, 0.0, -0.02], [-s, 0.0, c, 0.005]])
    return {"depth": md, "normal": mn}, depth, sn, D, (40.0, 40.0, 2.0, 1.5), (42.0, 41.0, 3.1, 2.4)


def rows_fp64(model, depth, sn, D, intr, mintr, dist, cos_min, depth_max):
    """sum [J r]^T [J r] (7 x 7, fp64), the counts, and the largest |p|, |q| and |w| met: plain loops, nothing shared with
    the mirror.  D is rounded to fp32 first, as the contract says; everything after that is fp64."""
    Df = D.astype(np.float32).astype(np.float64)
    R, t = Df[:, :3], Df[:, 3]
    fx, fy, cx, cy = intr
    mfx, mfy, mcx, mcy = mintr
    S, counts, M, Wmax = np.zeros((7, 7)), [0] * 7, 1.0, 0.0
    Hm, Wm = model["depth"].shape
    for v in range(depth.shape[0]):
        for u in range(depth.shape[1]):
            d, ns = float(depth[v, u]), sn[:, v, u].astype(np.float64)
            if not (d > 0 and np.isfinite(d) and d <= depth_max and np.any(ns != 0)):
                counts[1] += 1
                continue
            p = R @ np.array([(u - cx) / fx * d, (v - cy) / fy * d, d]) + t
            if not (p[2] > 0 and np.all(np.abs(p) < 16)):
                counts[2] += 1
                continue
            uf, vf = mfx * p[0] / p[2] + mcx, mfy * p[1] / p[2] + mcy
            assert abs(uf - np.floor(uf) - 0.5) > 0.01 and abs(vf - np.floor(vf) - 0.5) > 0.01, "a tie: fp32 may round the other way"
            um, vm = int(np.rint(uf)), int(np.rint(vf))
            if not (0 <= um < Wm and 0 <= vm < Hm):
                counts[3] += 1
                continue
            dm, n = float(model["depth"][vm, um]), model["normal"][vm, um].astype(np.float64)
            if not (dm > 0 and np.any(n != 0)):
                counts[4] += 1
                continue
            q = np.array([(um - mcx) / mfx * dm, (vm - mcy) / mfy * dm, dm])
            e = p - q
            if not e @ e <= dist * dist:
                counts[5] += 1
                continue
            if not n @ (R @ ns) >= cos_min:
                counts[6] += 1
                continue
            counts[0] += 1
            w = np.concatenate([n, np.cross(p, n), [n @ e]])
            S += np.outer(w, w)
            M, Wmax = max(M, np.abs(p).max(), np.abs(q).max()), max(Wmax, np.abs(w).max())
    return S, counts, M, Wmax


def test_rows_equal_an_independent_fp64_evaluation():
    """The bound, per entry: the n accepted pixels each add (a) the truncation to fixed point, below 2^-30, and (b) the fp32
    rounding of the product w_i w_j.  For (b): with M the largest coordinate of p and q met (at least 1), every w_i comes
    from fp32 inputs through at most 16 chained roundings of intermediates no larger than 3 M (a three-term sum of
    products of a coordinate and a value <= 1), so |dw| <= 16 u 3 M = e_w, and the product is off by at most
    2 W e_w + u W^2 with W the largest |w| met.  Nothing here comes from the result under test."""
    from monogs_amd import icp
    model, depth, sn, D, intr, mintr = hand_case()
    kw = dict(dist=0.3, cos_min=0.5, depth_max=5.0)
    sums, counts = icp.icp_rows_numpy(model, depth, sn, D, intr, mintr, 1, **kw)
    S, want_counts, M, Wmax = rows_fp64(model, depth, sn, D, intr, mintr, **kw)
    print("counts", counts, "M", M, "W", Wmax)
    assert list(counts) == want_counts and sum(want_counts) == depth.size
    assert all(c >= 1 for c in want_counts[:2] + want_counts[3:]) and want_counts[0] >= 8      # every gate but the range is met
    n = want_counts[0]
    e_w = 16 * U32 * 3 * M
    bound = n * (2.0 ** -30 + 2 * Wmax * e_w + U32 * Wmax * Wmax)
    worst = 0.0
    for i in range(7):
        for j in range(i, 7):
            worst = max(worst, abs(int(sums[icp.tri(i, j)]) / 2.0 ** 30 - S[i, j]))
    print(f"largest difference {worst:.3e}, bound {bound:.3e}, largest entry {np.abs(S).max():.3f}")
    assert worst <= bound and bound < 1e-3 * np.abs(S).max()
    # the stride grid: u, v = 0 (mod stride), and the counts cover exactly those pixels
    for stride in (2, 3, 4):
        s2, c2 = icp.icp_rows_numpy(model, depth, sn, D, intr, mintr, stride, **kw)
        on_grid = np.zeros(depth.shape, bool)
        on_grid[::stride, ::stride] = True
        S2, w2, _, _ = rows_fp64(model, np.where(on_grid, depth, np.float32(0)), sn, D, intr, mintr, **kw)
        assert int(c2.sum()) == int(on_grid.sum()) and int(c2[0]) == w2[0]
        assert abs(int(s2[icp.tri(6, 6)]) / 2.0 ** 30 - S2[6, 6]) <= bound and abs(int(s2[icp.tri(0, 3)]) / 2.0 ** 30 - S2[0, 3]) <= bound
    # the two layouts of the model normal
    chw = {"depth": model["depth"], "normal": np.ascontiguousarray(model["normal"].transpose(2, 0, 1))}
    s3, c3 = icp.icp_rows_numpy(chw, depth, sn, D, intr, mintr, 1, **kw)
    assert np.array_equal(s3, sums) and np.array_equal(c3, counts)


# ---- 2. solve ---------------------------------------------------------------------------------------------------------
def test_solve_agrees_with_numpy_linalg():
    """The allowance: LDL^T of a symmetric positive definite H is backward stable with |dH| <= gamma_(3n+1) |L||D||L^T|
    (Higham, Accuracy and Stability, Thm 10.4), i.e. a forward error of about (3n + 1) u cond(H) |x|; LAPACK's LU behind
    numpy.linalg.solve has 3 n u cond(H) |x| with a growth factor of 1 for such an H.  Both together, with n = 6 and
    u = 2^-53: (6 n + 1) u = 18.5 * 2^-52, taken as 20."""
    from monogs_amd import icp
    D0 = icp.initial_transform(np.eye(4))
    sums, counts = icp.icp_rows_numpy(IC.model_planes(), IC.frame_depth(), IC.sensor_normal(), D0, IC.INTR)
    s = icp.icp_solve_numpy(sums, counts[0], D0)
    H = np.array([[int(sums[icp.tri(min(i, j), max(i, j))]) / 2.0 ** 30 for j in range(6)] for i in range(6)])
    g = np.array([int(sums[icp.tri(i, 6)]) / 2.0 ** 30 for i in range(6)])
    want = np.linalg.solve(H, -g)
    cond = np.linalg.cond(H)
    diff = np.linalg.norm(s["x"] - want) / np.linalg.norm(want)
    print(f"cond(H) {cond:.1f}, |x - x_ref| / |x_ref| {diff:.3e}, allowance {20 * cond * EPS64:.3e}, pivots {s['pivots']}")
    assert s["status"] == icp.ITERATING and diff <= 20 * cond * EPS64
    assert np.all(s["pivots"] > 0) and np.isclose(np.prod(s["pivots"]), np.linalg.det(H), rtol=1e-9)
    # damping enters the diagonal
    sd = icp.icp_solve_numpy(sums, counts[0], D0, damping=5.0)
    wd = np.linalg.solve(H + 5.0 * np.eye(6), -g)
    assert np.linalg.norm(sd["x"] - wd) <= 20 * np.linalg.cond(H + 5.0 * np.eye(6)) * EPS64 * np.linalg.norm(wd)


# ---- 3. exponential ---------------------------------------------------------------------------------------------------
def test_polynomial_exponential_agrees_with_se3_exp():
    """Entries are at most 1 in magnitude (|rho| <= 0.2), so "a few ulps of the entries" is 4 * 2^-52 absolute.  |theta| is
    drawn from [0.1, 0.5]: below that pose.SE3_exp itself is the less accurate of the two - its (1 - cos phi) / phi^2
    loses phi^-2 ulps, which the term b W rho of the translation returns as (u / phi) |rho|."""
    from monogs_amd import icp
    from monogs_amd.pose import SE3_exp
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(400):
        th = rng.normal(size=3)
        th *= (0.5 if k < 8 else rng.uniform(0.1, 0.5)) / np.linalg.norm(th)
        x = np.concatenate([rng.uniform(-0.115, 0.115, 3), th])
        got = icp.se3_exp_poly(x)
        want = SE3_exp(torch.from_numpy(x)).numpy()[:3]
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"largest |Exp_poly - SE3_exp| over 400 draws: {worst:.3e} = {worst / EPS64:.2f} * 2^-52")
    assert worst <= 4 * EPS64
    # theta = 0 is exact, and the rotation stays orthonormal at the largest step
    assert np.array_equal(icp.se3_exp_poly([0.1, -0.2, 0.3, 0, 0, 0]), np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 0.3]]))
    R = icp.se3_exp_poly([0, 0, 0, 0.3, -0.3, 0.2645])[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 8 * EPS64
    # the constants: one division of an exact factorial each, seven terms
    assert len(icp.COEF_A) == 7 and icp.COEF_A[6] == 1.0 / 6227020800.0 and icp.COEF_C[6] == 1.0 / 1307674368000.0
    assert 0.25 ** 7 * icp.COEF_A[6] / 210.0 < 2.0 ** -53          # the first term left out of a, 0.25^7 / 15!


# ---- 4. recovery ------------------------------------------------------------------------------------------------------
# what align_numpy measured on this fixture (one stride-1 level, the analytic model): 1.7e-4 m, 8.7e-3 degrees
MEASURED_T, MEASURED_R_DEG = 1.7e-4, 8.7e-3


def test_recovery_of_a_known_motion():
    from monogs_amd import icp
    start = IC.pose_error(np.eye(4), IC.true_pose())
    print(f"start: {start[0]:.4f} m, {start[1]:.3f} degrees")
    assert abs(start[0] - 0.0439) < 1e-4 and abs(start[1] - 2.24) < 0.01
    assert start[0] > IC.CAP_T and start[1] > IC.CAP_R_DEG
    one = IC.recovery_mirror(((1, 10),))
    et, er = IC.pose_error(one["T_w2c"], IC.true_pose())
    info = one["info"]
    h = icp.read_history(one["history"])
    rms = np.sqrt(h["sum_r2"] / np.maximum(h["accepted"], 1))
    print(f"one level: {info['status_name']} after {info['iterations_run']} iterations, {et:.2e} m, {er:.2e} degrees, accepted "
          f"{info['counts']['accepted']} of {IC.H * IC.W}, residual rms {rms[:info['iterations_run']]}")
    print(f"smallest pivot / largest diagonal: {info['pivots'].min() / max(int(info['sums'][icp.tri(i, i)]) / 2.0 ** 30 for i in range(6)):.3e}")
    assert info["status"] == icp.CONVERGED and info["ok"]
    assert et <= 2 * MEASURED_T and er <= 2 * MEASURED_R_DEG and et <= IC.CAP_T and er <= IC.CAP_R_DEG
    assert rms[1] < 0.1 * rms[0]
    assert list(h["ran"][:info["iterations_run"]]) == [1] * info["iterations_run"] and not h["ran"][info["iterations_run"]:].any()
    assert sum(info["counts"].values()) == IC.H * IC.W
    # D and T_w2c say the same: T_w2c = D^-1 T_model with T_model = I
    assert np.array_equal(one["T_w2c"], icp.pose_of(one["D"], np.eye(4)))
    full = IC.recovery_mirror(icp.LEVELS)
    et, er = IC.pose_error(full["T_w2c"], IC.true_pose())
    print(f"default schedule: {full['info']['status_name']} after {full['info']['iterations_run']} of 19, {et:.2e} m, {er:.2e} degrees, "
          f"ran {icp.read_history(full['history'])['ran']}")
    assert full["info"]["status"] == icp.CONVERGED and et <= IC.CAP_T and er <= IC.CAP_R_DEG
    assert full["info"]["level"] == 2 and full["info"]["converged_level"] == 2


def test_start_pose_through_t_init():
    """T_init = T_model gives D_0 = I exactly, and a start at the answer converges at once."""
    from monogs_amd import icp
    Tm = np.eye(4, dtype=np.float32)
    assert np.array_equal(icp.initial_transform(Tm, Tm), np.eye(4)[:3])
    Tt = IC.true_pose().astype(np.float32)
    r = icp.align_numpy(IC.model_planes(), IC.frame_depth(), IC.INTR, Tm, T_init=Tt, levels=((1, 4),), sensor_normal=IC.sensor_normal())
    et, er = IC.pose_error(r["T_w2c"], IC.true_pose())
    print(r["info"]["status_name"], r["info"]["iterations_run"], et, er)
    assert r["info"]["status"] == icp.CONVERGED and r["info"]["iterations_run"] <= 2 and et <= IC.CAP_T and er <= IC.CAP_R_DEG


# ---- 5. / 6. statuses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["degenerate", "too_few", "step_too_large"])
def test_failure_statuses(name):
    from monogs_amd import icp
    model, depth, kw, status = IC.status_cases()[name]
    Tm = torch.eye(4)
    Tm[0, 3] = 0.25
    r = icp.align_numpy(model, depth, IC.INTR, Tm, levels=((2, 2), (1, 3)), **kw)
    info = r["info"]
    print(name, info["status_name"], info["counts"], info["pivots"], info["x"])
    assert info["status"] == status and not info["ok"] and info["iterations_run"] == 1
    assert np.array_equal(r["D"], np.eye(4)[:3]) and np.array_equal(r["T_w2c"], Tm.numpy())
    h = icp.read_history(r["history"])
    assert list(h["ran"]) == [1, 0, 0, 0, 0] and list(h["status"]) == [status] * 5
    if name == "degenerate":
        # columns 0, 1 and 5 of J = [n ; p x n] vanish for n = (0, 0, -1): exactly three pivots are exactly 0
        assert [float(p) == 0.0 for p in info["pivots"]] == [True, True, False, False, False, True]
        assert info["counts"]["accepted"] > 100 and not info["x"].any()
    if name == "too_few":
        assert info["counts"]["invalid"] == 23 * 35 and info["counts"]["accepted"] == 0
    if name == "step_too_large":
        print("theta_y", info["x"][4])
        assert abs(info["x"][4]) > 0.5 and np.all(info["pivots"] > 0.9e-3)


def test_rejection_counters():
    """0, NaN, inf and over-depth_max patches are INVALID (with the pixels that have no sensor normal), the one pixel at
    |p| >= 16 is RANGE, and every pixel of the stride grid lands in exactly one counter."""
    from monogs_amd import icp
    sn = IC.sensor_normal()                      # of the clean frame: the far pixel keeps a normal
    D = np.eye(4)[:3].copy()
    D[2, 3] = 0.02
    for stride in (1, 2):
        for depth_max in (16.0, 2.5):
            d = IC.patched_depth()
            d[10:14, 50:60] = 17.0 if depth_max == 16.0 else 3.0
            d[16, 24] = 15.99                      # passes depth_max = 16 only; p_z = 15.99 + 0.02 >= 16
            valid = (d > 0) & torch.isfinite(d) & (d <= depth_max) & (sn != 0).any(0)
            sub = (slice(None, None, stride), slice(None, None, stride))
            sums, counts = icp.icp_rows_numpy(IC.model_planes(), d, sn, D, IC.INTR, stride=stride, depth_max=depth_max)
            print(stride, depth_max, dict(zip(icp.COUNT_NAMES, (int(c) for c in counts))))
            assert int(counts[1]) == int((~valid)[sub].sum()) and int(counts[2]) == (1 if depth_max == 16.0 else 0)
            assert int(counts.sum()) == valid[sub].numel() and counts[0] > 600


# ---- 7. guards --------------------------------------------------------------------------------------------------------
def test_guards():
    from monogs_amd import icp
    model, depth, Tm = IC.model_planes(), IC.frame_depth(), np.eye(4, dtype=np.float32)
    run = lambda **kw: icp.align_numpy(kw.pop("model", model), kw.pop("depth", depth), IC.INTR, Tm, **kw)
    with pytest.raises(ValueError, match="2\\^22"):
        run(depth=np.zeros((2049, 2048), np.float32))
    assert icp._sensor_shape(np.zeros((2048, 2048), np.float32)) == (2048, 2048)
    with pytest.raises(ValueError, match="depth_max"):
        run(depth_max=16.5)
    with pytest.raises(ValueError, match="dist"):
        run(dist=9.0)
    for levels in ((), ((0, 3),), ((1, 0),), ((1.5, 2),), (3,), ((1, 2000),), ((1, 1),) * 9):
        with pytest.raises(ValueError, match="levels|iterations"):
            run(levels=levels)
    for normal in (torch.zeros(IC.H, IC.W), torch.zeros(IC.H, IC.W, 2), torch.zeros(3, IC.W, IC.H), torch.zeros(IC.H + 1, IC.W, 3)):
        with pytest.raises(ValueError, match="normal"):
            run(model={"depth": model["depth"], "normal": normal})
    with pytest.raises(ValueError):
        run(model={"depth": model["depth"]})
    with pytest.raises(ValueError, match="sensor_normal"):
        run(sensor_normal=torch.zeros(3, IC.H, IC.W + 1))
    with pytest.raises(ValueError):
        run(min_pivot_ratio=-1.0)
    # the device entry checks the same before it looks for a GPU
    for kw in (dict(depth_max=17.0), dict(levels=((0, 1),))):
        with pytest.raises(ValueError):
            icp.align(model, depth, IC.INTR, Tm, **kw)
    with pytest.raises(ValueError, match="2\\^22"):
        icp.align(model, torch.zeros(4096, 1025), IC.INTR, Tm)


def test_select_pose_on_the_cpu():
    from monogs_amd import icp
    T, F = torch.full((4, 4), 2.0), torch.eye(4)
    for st in range(6):
        got = icp.select_pose({"status": torch.tensor(st), "T_w2c": T}, F)
        assert torch.equal(got, T if st in (icp.CONVERGED, icp.MAX_ITERATIONS) else F), st


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_align_has_no_cpu_fallback():
    from monogs_amd import icp
    with pytest.raises(RuntimeError, match="GPU only"):
        icp.align(IC.model_planes(), IC.frame_depth(), IC.INTR, np.eye(4, dtype=np.float32))


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_icp_args_size() == C.sizeof(_cabi.IcpArgs) == 248          # checked at load, as the volumes' structs are
    assert L.mgs_struct_size(len(_cabi.struct_mirrors())) == -1               # the numbered list ends where it ended
    assert L.mgs_icp_scratch_bytes(0) == 8 * _cabi.ICP_ROWS_BLOCKS * _cabi.ICP_SUMS
    assert L.mgs_icp_scratch_bytes(19) == L.mgs_icp_scratch_bytes(0) + 19 * 8 * _cabi.ICP_HISTORY_WORDS
    assert L.mgs_icp_scratch_bytes(-1) == 0 and L.mgs_icp_scratch_bytes(1025) == 0
    assert L.mgs_icp_align(None, None) == -1

    def args(**kw):
        a = _cabi.IcpArgs()
        a.width, a.height, a.model_width, a.model_height, a.num_levels = 70, 45, 70, 45, 1
        a.stride[0], a.iterations[0] = 1, 2
        a.fx = a.fy = a.mfx = a.mfy = 60.0
        a.dist, a.cos_min, a.depth_max, a.min_pivot_ratio, a.converged = 0.1, 0.8, 10.0, 1e-6, 1e-4
        for n in ("depth", "normal", "model_depth", "model_normal", "T_model", "scratch", "T_w2c", "D", "record"):
            setattr(a, n, 4096)                # never dereferenced: every call below is refused first
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    bad = [dict(depth=None), dict(record=None), dict(scratch=None), dict(width=0), dict(model_height=0), dict(fx=0.0),
           dict(mfy=float("nan")), dict(num_levels=0), dict(num_levels=9), dict(stride=(0, 0)), dict(iterations=(0, 0)),
           dict(iterations=(0, 1025)), dict(model_normal_chw=2), dict(depth_max=16.5), dict(dist=8.5), dict(dist=float("nan")),
           dict(cos_min=1.5), dict(min_pivot_ratio=-1.0), dict(damping=float("nan")), dict(converged=-1.0), dict(min_pixels=-1),
           dict(scratch=4100)]
    for kw in bad:
        assert L.mgs_icp_align(C.byref(args(**kw)), None) == -1, kw
    assert L.mgs_icp_align(C.byref(args(width=4096, height=1025)), None) == -3
    assert L.mgs_icp_align(C.byref(args(model_width=40000, model_height=20000)), None) == -3
