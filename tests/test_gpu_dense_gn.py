"""Dense Gauss-Newton tracking on the GPU (NativeTracker.enable_second_order(exact=True), mgs_normal_equations,
mgs_tracking_iteration_gauss_newton[_rgbd]): the normal equations against an fp64 oracle, past one trip of k_normal_eq's
grid, one iteration against the Python mirror, bit reproducibility, and the sketched path left as it was.

Objective (include/monogs_raster.h): f_p = s sum_c Huber(r_pc), s = stack * sketch / (H W) = 1024 / (H W) here,
J_p = d f_p / d [rho; theta; a; b], H = sum J^T J, g = sum J^T f over all pixels.

Tolerances of the H / g comparisons.  The project holds a per-pixel or per-bucket row to its reference at 2e-3 (pose
columns, through the rasteriser) and 1e-4 (exposure columns and f), relative Frobenius.  A product of two such rows
carries the sum of their errors: pose-pose block 4e-3, pose-exposure block and g[:6] (pose row times f) 2.1e-3,
exposure block and g[6:] 2e-4.  All figures are printed before they are asserted (run with -s)."""
import math

import pytest
import torch

from conftest import oracle_settings, rel_err
import sketch_oracle as SO
from test_raster_gpu import _loop_fixture

pytestmark = pytest.mark.gpu

STACK, SKETCH = 16, 64
D = STACK * SKETCH
HUBER = 0.01
TOL_PP, TOL_PE, TOL_EE = 4e-3, 2.1e-3, 2e-4
TAU_LOOP = (0.02, -0.015, 0.01, 0.004, -0.006, 0.003)          # the start of the native-vs-Python tests
TAU_RAGGED = (0.04, -0.03, 0.08, 0.02, -0.03, 0.02)            # the moved camera of the 70x45 oracle tests


def _fixture(kind):
    """(sc, gauss, view, dev, tau).  'ragged': the construction of test_sketched_pose_jacobian_16x64_matches_the_fp64_oracle -
    500 Gaussians, 70x45 (15 tiles, none of the right column and bottom row whole), scales * 1.5, moved camera.
    'loop': _loop_fixture at 160x120."""
    from monogs_amd.slam_loops import GaussianParams
    if kind == "loop":
        return (*_loop_fixture(N=4000, W=160, H=120), TAU_LOOP)
    sc, gauss, view, dev = _loop_fixture(N=500, W=70, H=45, seed=12)
    sc = sc._replace(log_scales=sc.log_scales + math.log(1.5))
    gauss = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev), sc.opacity_logit.to(dev),
                           sc.features_dc.to(dev))
    return sc, gauss, view, dev, TAU_RAGGED


def _frame(view, uid, T0, target, depth=None, gain=0.97):
    v = view(uid, T0)
    v.original_image = target
    v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    v.gt_depth = depth
    with torch.no_grad():
        v.exposure_a.fill_(gain)
        v.exposure_b.fill_(0.01)
    return v


def _target(view, gauss, dev):
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        pkg = render(view(1, torch.eye(4)), gauss, Pipe, bg)
    return pkg["render"].clone(), pkg["depth"].clone(), bg


def channel_tangents(sc, T0):
    """d image / d tau [3, H, W, 6] and d depth / d tau [H, W, 6] of the fp64 CPU oracle's render at pose T0: the six
    forward-mode passes of sketch_oracle.per_pixel_pose_jacobian, with the contraction over the channels (its A_img /
    B_dep) left to the caller - per_pixel_pose_jacobian(A, B) = sum_c A_c dI_c + B dD, so ONE set of passes serves
    every objective of a fixture (the monocular 70x45 case checks that identity against the function itself)."""
    import torch.autograd.forward_ad as fwAD
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    cam = S.make_camera(sc.cam.W, sc.cam.H, T0.cpu())
    st = oracle_settings(cam, torch.zeros(3), dtype=torch.float64)
    ins = [SO.f64(t) for t in S.activated(sc)]
    dI, dD = [], []
    for i in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[i] = 1.0
        with fwAD.dual_level():
            tau = fwAD.make_dual(torch.zeros(6, dtype=torch.float64), e)
            img, _, dep, _, _, _ = O.rasterize(ins[0], None, ins[4], None, ins[3], ins[1], ins[2], None, st, tau[3:], tau[:3])
            ti, td = fwAD.unpack_dual(img).tangent, fwAD.unpack_dual(dep).tangent
            dI.append(torch.zeros_like(img.detach()) if ti is None else ti.clone())
            dD.append(torch.zeros_like(dep.detach()[0]) if td is None else td[0].clone())
    return torch.stack(dI, -1), torch.stack(dD, -1), (ins, st)


_TANGENTS = {}


def _tangents(kind, sc, T0):
    if kind not in _TANGENTS:                 # one set of oracle passes per fixture, shared by its cases, never modified
        _TANGENTS[kind] = channel_tangents(sc, T0)
    return _TANGENTS[kind]


def exact_residual_planes(image, depth, opacity, gt, mask, a, b, eps, scale, gt_depth=None, alpha=None):
    """fp64 planes of the exact residual pass from a render: f, df/da, df/db [H, W] and the upstream gradients
    A_img [3, H, W], B_dep [1, H, W] (d f / d image, d f / d depth), with the exposure derivatives as the reference's
    hand-written ApplyExposure.backward takes them (|a| without eps on the image, the image without sign(a) on a)."""
    def huber(x):
        ax = x.abs()
        out = ax >= HUBER
        s = torch.sqrt((2 * HUBER * ax - HUBER ** 2).clamp_min(1e-300))
        return torch.where(out, s * torch.sign(x), x), torch.where(out, HUBER / s, torch.ones_like(x))
    image, depth, opacity, gt, mask = (t.detach().double().cpu() for t in (image, depth, opacity, gt, mask))
    om = opacity * mask                                                   # [1, H, W]
    w_rgb = 1.0 if alpha is None else alpha
    r = w_rgb * om * ((abs(a) + eps) * image + b - gt)
    h, dh = huber(r)
    gup = scale * dh * om * w_rgb                                         # d f / d (gain image + b)
    f = scale * h.sum(0)
    A_img, da, db = gup * abs(a), (gup * image).sum(0), gup.sum(0)
    B_dep = torch.zeros_like(depth)
    l1 = r.abs().sum()
    if alpha is not None:
        gtd = gt_depth.detach().double().cpu().view_as(depth)
        # float32 comparisons, as the kernel makes them on the float32 render
        dm = ((gt_depth.detach().float().cpu().view_as(depth) > 0.01) & (opacity.float() > 0.95)).double()
        rd = (1.0 - alpha) * (depth * dm - gtd * dm)
        hd, dhd = huber(rd)
        f = f + scale * hd[0]
        B_dep = scale * dhd * (1.0 - alpha) * dm
        l1 = l1 + rd.abs().sum()
    return f, da, db, A_img, B_dep, l1


def reference_system(trk, vp, tangents, alpha=None, gt_depth=None):
    """(H [8, 8], g [8], J [H W, 8], f [H W], l1) in fp64: pose columns = the oracle's channel tangents contracted with
    the upstream gradients of the exact residual of the tracker's own render (trk.color / depth / opacity: written by
    the forward, which is not under test here), exposure columns analytic."""
    dI, dD, _ = tangents
    Hh, Ww = trk.H, trk.W
    mask = torch.ones(1, Hh, Ww) if trk.mask is None else trk.mask.view(1, Hh, Ww)
    f, da, db, A_img, B_dep, l1 = exact_residual_planes(
        trk.color, trk.depth, trk.opacity, trk.gt, mask, float(vp.exposure_a.detach()), float(vp.exposure_b.detach()),
        float(vp.exposure_eps), D / (Hh * Ww), gt_depth, alpha)
    Jp = (A_img[..., None] * dI).sum(0) + B_dep[0][..., None] * dD       # [H, W, 6]
    J = torch.cat([Jp.reshape(-1, 6), da.reshape(-1, 1), db.reshape(-1, 1)], 1)
    f = f.reshape(-1)
    return J.T @ J, J.T @ f, J, f, l1, (A_img, B_dep)


def block_errors(Hn, gn, Hr, gr):
    Hn, gn = Hn.double().cpu(), gn.double().cpu()
    return {"pose-pose": rel_err(Hn[:6, :6], Hr[:6, :6]), "pose-exposure": rel_err(Hn[:6, 6:], Hr[:6, 6:]),
            "exposure": rel_err(Hn[6:, 6:], Hr[6:, 6:]), "g pose": rel_err(gn[:6], gr[:6]),
            "g exposure": rel_err(gn[6:], gr[6:])}


def assert_blocks(tag, errs):
    print(f"{tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["pose-pose"] < TOL_PP, errs
    assert errs["pose-exposure"] < TOL_PE and errs["g pose"] < TOL_PE, errs
    assert errs["exposure"] < TOL_EE and errs["g exposure"] < TOL_EE, errs


@pytest.mark.parametrize("kind", ["ragged", "loop"])
@pytest.mark.parametrize("objective", ["monocular", "masked", "rgbd"])
def test_normal_equations_match_the_fp64_oracle(built, kind, objective):
    """mgs_normal_equations (exact residual pass, k_blend_bwd<true, true>, k_normal_eq, the fp64 sum of the partials)
    against H = J^T J, g = J^T f of the fp64 oracle rows, per block at the module's tolerances.  monocular: the
    viewpoint's own mask; masked: a random 0 / 1 pixel mask (30 % off) handed to the tracker; rgbd: the stacked
    objective, alpha 0.9.  Conditions: H is symmetric as returned, every diagonal entry of the reference is positive,
    lm_state / pose / exposure are untouched by the call."""
    from monogs_amd.pose import SE3_exp
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev, tau = _fixture(kind)
    T0 = SE3_exp(torch.tensor(tau))
    target, depth, bg = _target(view, gauss, dev)
    alpha = 0.9 if objective == "rgbd" else None
    vp = _frame(view, 2, T0, target, depth if alpha else None)
    mask = None
    if objective == "masked":
        g = torch.Generator().manual_seed(4)
        mask = (torch.rand(1, vp.image_height, vp.image_width, generator=g) > 0.3).float().to(dev)
    trk = NativeTracker(vp, gauss, bg, mask=mask, **(dict(gt_depth=depth, alpha=alpha) if alpha else {}))
    trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, exact=True)
    T_before, lm_before = vp.T.clone(), trk.lm_state.clone()
    Hn, gn = trk.compute_normal_equations()
    torch.cuda.synchronize()
    assert torch.equal(vp.T, T_before) and torch.equal(trk.lm_state, lm_before) and float(vp.exposure_a.detach()) == pytest.approx(0.97)
    assert torch.equal(Hn, Hn.T) and trk.check_capacity()
    tangents = _tangents(kind, sc, T0)
    Hr, gr, J, f, l1, (A_img, B_dep) = reference_system(trk, vp, tangents, alpha, depth if alpha else None)
    if kind == "ragged" and objective == "monocular":
        ins, st = tangents[2]
        Jp = SO.per_pixel_pose_jacobian(*ins, st, A_img, B_dep)
        same = rel_err(Jp.reshape(-1, 6), J[:, :6])
        print(f"contraction of the channel tangents vs per_pixel_pose_jacobian: {same:.3e}")
        assert same < 1e-12
    assert bool((torch.diagonal(Hr) > 0).all()) and float(gr.abs().min()) > 0
    if objective == "masked":
        assert float(f[mask.reshape(-1).cpu() == 0].abs().max()) == 0.0
    assert_blocks(f"{kind} {trk.W}x{trk.H} {objective}", block_errors(Hn, gn, Hr, gr))


def test_normal_equations_past_one_tile_trip(built):
    """520x512 = 33 x 32 = 1056 tiles (a partial tile column): more than the 256 workgroups x 4 tiles of one trip of
    k_normal_eq, the size test_bucket_kernel_second_tile_trip_matches_the_dense_backward chooses for k_sketch_bucket; 16 000
    Gaussians of four times the scene's footprint, so that a tile holds several backward items and its rows are the sum
    of several slabs (condition: pairs >= 4 items x 32 splats per tile on average).  266 240 pixels also make the exact
    residual pass loop (256 x 256 pixels per trip).
    g[:6] against the DENSE fp32 backward of 1/2 sum_p f_p^2 (sketch_mode 0: no slab, mask-word or normal-equation code),
    2e-3 - the project's bound for a pose gradient through the rasteriser.  H and g against the sums of the rows the
    EXISTING sketch kernels give with identity buckets (slam_loops.harvest_pixel_rows: 130 passes of 2048 pixels), at
    the block tolerances.  Condition: the rows of the last tile row (tiles 1023 .. 1055, second trip) carry a share of
    trace(H[:6, :6]) that the pose-pose tolerance cannot hide."""
    from monogs_amd import losses as Ls
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import DEFAULT_CONFIG, GaussianParams, Pipe, harvest_pixel_rows, normal_equations_from_rows
    from monogs_amd.tracking_native import NativeTracker
    N, W, H = 16000, 520, 512
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert T == 1056 and T > 256 * 4
    sc, gauss, view, dev = _loop_fixture(N=N, W=W, H=H, seed=12)
    gauss = GaussianParams(sc.means3D.to(dev), (sc.log_scales + math.log(4.0)).to(dev), sc.rot.to(dev),
                           sc.opacity_logit.to(dev), sc.features_dc.to(dev))
    T0 = SE3_exp(torch.tensor(TAU_LOOP))
    target, depth, bg = _target(view, gauss, dev)
    va, vb, vc = (_frame(view, uid, T0, target) for uid in (2, 3, 4))
    trk = NativeTracker(vb, gauss, bg)
    trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, exact=True)
    Hn, gn = trk.compute_normal_equations()
    torch.cuda.synchronize()
    pairs = trk.pairs()
    print(f"{W}x{H}: {pairs} pairs, {pairs / T:.1f} per tile")
    assert trk.check_capacity() and pairs >= 4 * 32 * T
    # dense backward of 1/2 sum f^2
    pkg = render(va, gauss, Pipe, bg)
    res = Ls.get_loss_tracking_per_pixel(DEFAULT_CONFIG, pkg["render"], pkg["depth"], pkg["opacity"], va)
    f = Ls.HuberLoss.apply(res, HUBER).sum(0) / (H * W / D)
    (0.5 * (f * f).sum()).backward()
    g_dense = torch.cat([va.cam_trans_delta.grad, va.cam_rot_delta.grad])
    e_dense = rel_err(gn[:6], g_dense)
    # the existing kernels' per-pixel rows
    l1, f_rows, J_rows, _ = harvest_pixel_rows(vc, gauss, bg, D)
    Hr, gr = normal_equations_from_rows(J_rows, f_rows)
    tail = J_rows[496 * W:, :6].double()
    share = float((tail * tail).sum() / torch.diagonal(Hr)[:6].sum())
    print(f"{W}x{H}: g[:6] vs dense backward {e_dense:.3e}; share of trace(H pose) in the image rows >= 496: {share:.3e}")
    assert share > 2 * TOL_PP
    assert e_dense < 2e-3
    assert_blocks(f"{W}x{H} vs identity-bucket rows", block_errors(Hn, gn, Hr.cpu(), gr.cpu()))


def test_native_exact_iteration_matches_the_python_mirror(built):
    """One mgs_tracking_iteration_gauss_newton against tracking_step_second_order(exact=True) (rows from the existing
    sketch kernels with identity buckets, H and g in fp64, torch.linalg.solve) at 160x120 from the same start: the step x
    at 5e-3, the stepped pose and exposure at atol 1e-4 - the numbers of
    test_native_second_order_iteration_16x64_matches_python_formulation.
    Condition: cond(H_oracle + lambda I) <= 1e4 with the fp64 oracle's H, so that the 4e-3 the two sides' H may differ by
    cannot be amplified past the bound on x.  Chosen on the CPU oracle (target and render by the oracle): eigenvalues of
    H 0.55 .. 1910, cond(H + 1e-3 I) = 3.5e3 - lambda stays the 1e-3 of the sketched test."""
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import tracking_step_second_order
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev, tau = _fixture("loop")
    T0 = SE3_exp(torch.tensor(tau))
    target, depth, bg = _target(view, gauss, dev)
    va, vb = _frame(view, 2, T0, target), _frame(view, 3, T0, target)
    lam = 1e-3
    trk = NativeTracker(vb, gauss, bg)
    trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, initial_lambda=lam, exact=True)
    state = trk.step_second_order()
    torch.cuda.synchronize()
    Hn, gn = trk.normal_equations
    # the render the iteration started from is still in the tracker's buffers: the oracle's system at T0
    ref_vp = _frame(view, 5, T0, target)
    Hr, gr, _, _, l1_ref, _ = reference_system(trk, ref_vp, _tangents("loop", sc, T0))
    cond = float(torch.linalg.cond(Hr + lam * torch.eye(8, dtype=torch.float64)))
    print(f"cond(H_oracle + {lam} I) = {cond:.3e}; eigenvalues of H_oracle {torch.linalg.eigvalsh(Hr).tolist()}")
    assert cond <= 1e4
    l1, x, J, f = tracking_step_second_order(va, gauss, bg, lambda_=lam, stack_dim=STACK, sketch_dim=SKETCH, exact=True)
    e_x = rel_err(trk.so_x, x)
    st = state.cpu()
    print(f"160x120: rel_err of the step {e_x:.3e}, |x| {float(x.norm()):.3e}, L1 {st[1].item():.6e} vs {float(l1):.6e}")
    assert float(x.abs().max()) > 0
    assert e_x < 5e-3
    assert torch.allclose(va.T, vb.T, atol=1e-4)
    assert torch.allclose(va.exposure_a, vb.exposure_a, atol=1e-4)
    assert torch.allclose(va.exposure_b, vb.exposure_b, atol=1e-4)
    assert abs(st[0].item() - lam) < 1e-9 and st[2].item() == 1.0 and st[3].item() == 0.0
    assert abs(st[1].item() - float(l1)) < 1e-4 * float(l1)
    assert abs(float(trk.last_l1) - float(l1)) < 1e-4 * float(l1) and trk.best_iteration() == 0
    assert_blocks("160x120 native iteration vs oracle", block_errors(Hn, gn, Hr, gr))
    assert trk.check_capacity()


@pytest.mark.parametrize("rgbd", [False, True])
def test_exact_iterations_are_bit_reproducible(built, rgbd):
    """Two trackers, the same start, five exact iterations each: T, exposure, lm_state, the step and (H, g) of the last
    iteration agree BIT FOR BIT (no atomics between the render and the step).  Condition: the iterations moved the pose
    and changed lambda, i.e. they were not no-ops."""
    from monogs_amd.pose import SE3_exp
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev, tau = _fixture("loop")
    T0 = SE3_exp(torch.tensor(tau))
    target, depth, bg = _target(view, gauss, dev)
    out = []
    for uid in (2, 3):
        vp = _frame(view, uid, T0, target, depth if rgbd else None)
        trk = NativeTracker(vp, gauss, bg, **(dict(gt_depth=depth, alpha=0.9) if rgbd else {}))
        trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, exact=True)
        for _ in range(5):
            trk.step_second_order()
        torch.cuda.synchronize()
        Hn, gn = trk.normal_equations
        out.append([t.detach().clone() for t in (vp.T, vp.exposure_a, vp.exposure_b, trk.lm_state, trk.so_x, Hn, gn,
                                                 trk.best)])
        assert trk.check_capacity()
    T_end, lm = out[0][0], out[0][3].cpu()
    assert not torch.allclose(T_end.cpu(), T0, atol=1e-5) and lm[0].item() != 1e-3 and lm[2].item() == 1.0
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_sketched_path_is_unchanged_by_the_exact_mode(built):
    """exact=False is today's iteration.  Three sketched iterations of a tracker built with the parent's call
    (enable_second_order without the new argument) before any exact call of this test, and of one built with exact=False
    after an exact tracker has run on the same buffers' allocator: the same launch sequence - the kernel names and
    launch counts of the three iterations, none of the new kernels among them - the same partition and signs bit for bit,
    and the same sketch, lambda and pose.  The sketched sums are float atomics (LDS and global), so two runs of the SAME
    code differ in the last bits: Sf / SJ are held to 1e-5 relative Frobenius (a bucket sums H W / 1024 = 18 terms; fp32
    reordering noise is ~1e-7 per term) and the pose to atol 3e-5, three times the 1e-5 the project already allows two
    runs of one sketched iteration (test_native_second_order_iteration_16x64_matches_python_formulation)."""
    from monogs_amd import _cabi
    from monogs_amd.pose import SE3_exp
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev, tau = _fixture("loop")
    T0 = SE3_exp(torch.tensor(tau))
    target, depth, bg = _target(view, gauss, dev)

    def sketched(uid, **kw):
        vp = _frame(view, uid, T0, target)
        trk = NativeTracker(vp, gauss, bg)
        trk.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, seed=5, keep_sketch=True, **kw)
        torch.cuda.synchronize()
        _cabi.profile_enable(True)
        try:
            for _ in range(3):
                trk.step_second_order()
            torch.cuda.synchronize()
            prof = _cabi.profile_read()
        finally:
            _cabi.profile_enable(False)
        Sf, SJ = trk.sketch
        return vp, trk, {k: n for k, (_, n) in prof.items()}, Sf.clone(), SJ.clone()

    va, ta, launches_a, Sf_a, SJ_a = sketched(2)
    ve = _frame(view, 3, T0, target)
    te = NativeTracker(ve, gauss, bg)
    te.enable_second_order(stack_dim=STACK, sketch_dim=SKETCH, exact=True)
    _cabi.profile_enable(True)
    try:
        te.step_second_order()
        torch.cuda.synchronize()
        launches_e = {k: n for k, (_, n) in _cabi.profile_read().items()}
    finally:
        _cabi.profile_enable(False)
    vb, tb, launches_b, Sf_b, SJ_b = sketched(4, exact=False)
    new = {"normal_prep_residual", "normal_prep_residual_rgbd", "normal_eq", "lm_solve_normal"}
    print(f"sketched launches {launches_a}; exact launches {launches_e}")
    assert launches_a == launches_b and not (new & set(launches_a))
    assert {"sketch_prep_residual": 3, "blend_bwd_sketch": 3, "sketch_bucket": 3, "lm_solve_step": 3}.items() <= launches_a.items()
    assert {"normal_prep_residual": 1, "blend_bwd_sketch": 1, "normal_eq": 1, "lm_solve_normal": 1}.items() <= launches_e.items()
    assert not ({"sketch_bucket", "lm_solve_step", "sketch_prep_residual"} & set(launches_e))
    assert torch.equal(ta.so_bucket, tb.so_bucket) and torch.equal(ta.so_weights, tb.so_weights)
    e_sf, e_sj = rel_err(Sf_b, Sf_a), rel_err(SJ_b, SJ_a)
    print(f"sketch of the third iteration, run to run: Sf {e_sf:.3e}, SJ {e_sj:.3e}; "
          f"pose {float((va.T - vb.T).abs().max()):.3e}")
    assert e_sf < 1e-5 and e_sj < 1e-5
    assert torch.allclose(va.T, vb.T, atol=3e-5)
    assert torch.allclose(va.exposure_a, vb.exposure_a, atol=3e-5) and torch.allclose(va.exposure_b, vb.exposure_b, atol=3e-5)
    assert torch.equal(ta.lm_state[2:], tb.lm_state[2:])
    with pytest.raises(ValueError):
        NativeTracker(_frame(view, 6, T0, target), gauss, bg).enable_second_order(exact=True, repeat_dim=2)
    with pytest.raises(RuntimeError):
        tb.normal_equations
    with pytest.raises(RuntimeError):
        te.sketch
