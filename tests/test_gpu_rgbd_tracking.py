"""RGB-D tracking on the GPU: the stacked objective (losses.get_loss_tracking_stacked: colour rows times alpha, the
masked depth row times 1 - alpha) in the HIP loss, the forward blend's epilogue, the sketched residual pass and the
native first- and second-order iterations, against the reference-shaped Python on the drop-in rasteriser."""
import math

import pytest
import torch

from conftest import rel_err
from test_raster_gpu import _loop_fixture

pytestmark = pytest.mark.gpu


def _target(view, gauss, dev, T=None):
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        pkg = render(view(1, torch.eye(4) if T is None else T), gauss, Pipe, bg)
    return pkg["render"].clone(), pkg["depth"].clone(), bg


def _frame(view, uid, T0, target, depth):
    v = view(uid, T0)
    v.original_image = target
    v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    v.gt_depth = depth
    return v


def _cfg(alpha, use_huber=True, pnorm=1):
    from monogs_amd.slam_loops import DEFAULT_CONFIG
    t = dict(DEFAULT_CONFIG["Training"])
    t.update(monocular=False, alpha=alpha, RGN={"use_huber": use_huber, "huber_delta": 0.01, "pnorm": pnorm})
    return {"Training": t}


def test_hip_rgbd_loss_matches_torch_autograd(built):
    """Value and the gradients w.r.t. image, depth, a and b of || Huber(r) ||_p against torch autograd over
    get_loss_tracking_stacked, p in {2, 1, 1.5}, Huber on and off, a > 0 and a < 0."""
    from monogs_amd import losses as Ls
    from monogs_amd.tracking_fused import tracking_loss_rgbd
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    class VP:
        pass

    # 120x160, then 363x365: an odd count past one trip of the kernel's grid
    cases = [(H, W, *c) for H, W in ((120, 160), (363, 365))
             for c in ((0.01, 0.9, 2.0, 0.95), (0.0, -1.1, 2.0, 0.9), (0.0, 0.9, 1.0, 0.95),
                       (0.01, -1.1, 1.0, 0.9), (0.0, 1.05, 1.5, 0.95), (0.01, 0.9, 1.5, 0.9))]
    for H, W, delta, a0, pn, alpha in cases:
        vp = VP()
        vp.original_image = torch.rand(3, H, W, generator=g).to(dev)
        vp.rgb_pixel_mask_mapping = (torch.rand(1, H, W, generator=g) > 0.2).to(dev)
        vp.exposure_a = torch.tensor([a0], device=dev, requires_grad=True)
        vp.exposure_b = torch.tensor([0.03], device=dev, requires_grad=True)
        vp.exposure_eps = 1e-8
        depth = (1.0 + torch.rand(1, H, W, generator=g)).to(dev)
        gtd = depth + 0.05 * torch.randn(1, H, W, generator=g).to(dev)
        gtd[torch.rand(1, H, W, generator=g).to(dev) < 0.1] = 0.0
        vp.gt_depth = gtd
        img = torch.rand(3, H, W, generator=g).to(dev).requires_grad_()
        dep = depth.clone().requires_grad_()
        opa = (0.9 + 0.1 * torch.rand(1, H, W, generator=g)).to(dev)
        res = Ls.get_loss_tracking_stacked({"Training": {"monocular": False, "alpha": alpha}}, img, dep, opa, vp)
        if delta > 0:
            res = Ls.HuberLoss.apply(res, delta)
        ref = torch.norm(res.flatten(), p=pn)
        (2.5 * ref).backward()
        want = (ref.item(), img.grad.clone(), dep.grad.clone(), vp.exposure_a.grad.clone(), vp.exposure_b.grad.clone())
        for t in (img, dep, vp.exposure_a, vp.exposure_b):
            t.grad = None
        got = tracking_loss_rgbd(img, dep, opa, vp, alpha, delta, pn)
        (2.5 * got).backward()
        tol = 1e-5 if pn != 1.5 else 1e-4
        assert abs(got.item() - want[0]) <= 1e-5 * want[0], (H, W, delta, pn)
        assert rel_err(img.grad, want[1]) < tol and rel_err(dep.grad, want[2]) < tol, (H, W, delta, pn)
        assert rel_err(vp.exposure_a.grad, want[3]) < 1e-4 and rel_err(vp.exposure_b.grad, want[4]) < 1e-4


def _python_grads(vp, gauss, bg, cfg):
    """dL/dtau, dL/da, dL/db of one first-order RGB-D step of the reference-shaped loop body (no optimiser step)."""
    from monogs_amd import losses as Ls
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe, tracking_norm
    pkg = render(vp, gauss, Pipe, bg)
    res = Ls.get_loss_tracking_stacked(cfg, pkg["render"], pkg["depth"], pkg["opacity"], vp)
    delta, p = tracking_norm(cfg)
    if delta > 0:
        res = Ls.HuberLoss.apply(res, delta)
    loss = torch.norm(res.flatten(), p=p)
    for t in (vp.cam_rot_delta, vp.cam_trans_delta, vp.exposure_a, vp.exposure_b):
        t.grad = None
    loss.backward()
    return (torch.cat([vp.cam_rot_delta.grad, vp.cam_trans_delta.grad]), vp.exposure_a.grad.clone(),
            vp.exposure_b.grad.clone(), loss.detach())


def _native_grads(trk):
    """The gradient of the tracker's first iteration, read back from Adam's first moment: m = (1 - beta1) g."""
    trk.step()
    torch.cuda.synchronize()
    g = trk.exp_avg / 0.1
    return g[:6], g[6:7], g[7:8]


@pytest.mark.parametrize("alpha,use_huber", [(0.95, True), (0.9, False), (0.0, True)])
def test_one_rgbd_first_order_step_matches_the_python_step(built, alpha, use_huber):
    """dL/dtau and the exposure gradients of ONE native RGB-D iteration against the reference-shaped Python step on
    the drop-in rasteriser (alpha = 0: depth alone - no exposure gradient at all)."""
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import tracking_norm
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    target, depth, bg = _target(view, gauss, dev)
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.03, 0.004, -0.006, 0.003]))
    cfg = _cfg(alpha, use_huber)
    va, vb = _frame(view, 2, T0, target, depth), _frame(view, 3, T0, target, depth)
    gt_tau, ga, gb, loss = _python_grads(va, gauss, bg, cfg)
    delta, p = tracking_norm(cfg)
    trk = NativeTracker(vb, gauss, bg, huber_delta=delta, pnorm=p, gt_depth=depth, alpha=alpha)
    n_tau, n_a, n_b = _native_grads(trk)
    assert trk.check_capacity()
    assert abs(trk.loss.item() - loss.item()) <= 1e-4 * loss.item()
    assert rel_err(n_tau, gt_tau) <= 2e-3, (n_tau, gt_tau)
    if alpha > 0:
        assert rel_err(n_a, ga) <= 2e-3 and rel_err(n_b, gb) <= 2e-3
    else:
        assert float(n_a.abs().max()) == 0.0 and float(n_b.abs().max()) == 0.0
        assert float(ga.abs().max()) == 0.0


def test_sketched_jacobian_sums_to_the_pose_gradient_with_depth_rows(built):
    """Every pixel lies in exactly one bucket (19200 pixels, 64 buckets of 300), so the tau columns of the sketched
    Jacobian of the native RGB-D second-order iteration add up, over the buckets, to the gradient of the sum of the
    weighted Hubered residual rows w.r.t. (trans, rot) - which the Python formulation gets by plain autograd."""
    from monogs_amd import losses as Ls
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    target, depth, bg = _target(view, gauss, dev)
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.03, 0.004, -0.006, 0.003]))
    stack, sketch, alpha = 4, 16, 0.9
    vb = _frame(view, 3, T0, target, depth)
    trk = NativeTracker(vb, gauss, bg, gt_depth=depth, alpha=alpha)
    trk.enable_second_order(stack_dim=stack, sketch_dim=sketch, seed=5, keep_sketch=True)
    trk.step_second_order()
    torch.cuda.synchronize()
    _, SJ_n = trk.sketch
    H, W = vb.image_height, vb.image_width
    assert bool((trk.so_bucket >= 0).all())
    va = _frame(view, 2, T0, target, depth)
    pkg = render(va, gauss, Pipe, bg)
    res = Ls.get_loss_tracking_stacked(_cfg(alpha), pkg["render"], pkg["depth"], pkg["opacity"], va)
    res = Ls.HuberLoss.apply(res, 0.01).sum(dim=0) / (H * W / (stack * sketch))
    (res * trk.so_weights.view(H, W)).sum().backward()
    full = torch.cat([va.cam_trans_delta.grad, va.cam_rot_delta.grad])
    assert rel_err(SJ_n[:, :6].sum(0), full) < 2e-3
    # the depth rows are in it: without them (alpha = 1) the sum is a different vector
    vc = _frame(view, 4, T0, target, depth)
    trk1 = NativeTracker(vc, gauss, bg)
    trk1.enable_second_order(stack_dim=stack, sketch_dim=sketch, seed=5, keep_sketch=True)
    trk1.step_second_order()
    assert rel_err(trk1.sketch[1][:, :6].sum(0), full) > 1e-2


def test_native_rgbd_iterations_match_track_frame(built):
    """A native RGB-D frame (first order, then sketched LM from the best first-order state) against
    track_frame(residual_fn=get_loss_tracking_stacked) fed with the native tracker's bucket partitions (fsa_fn):
    the L1 criterion and the step of every iteration of the common prefix, and the final pose."""
    from monogs_amd.losses import get_loss_tracking_stacked
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import sketch_args_from_buckets, track_frame
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    target, depth, bg = _target(view, gauss, dev)
    T0 = SE3_exp(torch.tensor([0.03, -0.02, 0.04, 0.006, -0.008, 0.004]))
    fo, so, stack, sketch, alpha = 8, 3, 4, 16, 0.9
    cfg = _cfg(alpha)
    vn = _frame(view, 3, T0, target, depth)
    H, W = vn.image_height, vn.image_width
    trk = NativeTracker(vn, gauss, bg, gt_depth=depth, alpha=alpha)
    trk.enable_second_order(stack_dim=stack, sketch_dim=sketch, seed=5)
    native, parts = [], []
    for _ in range(fo):
        trk.step()
        native.append((float(trk.last_l1), float(trk.last_step_norm)))
    trk.assign_best()
    for _ in range(so):
        trk.step_second_order()
        native.append((float(trk.last_l1), float(trk.last_step_norm)))
        parts.append((trk.so_bucket.clone(), trk.so_weights.clone()))
    assert trk.check_capacity()
    vp = _frame(view, 2, T0, target, depth)
    trace = []
    fsa_fn = lambda i: sketch_args_from_buckets(parts[i][0], parts[i][1], H, W, stack, sketch)
    track_frame(vp, gauss, bg, first_order_iters=fo, second_order_iters=so, config=cfg, stack_dim=stack,
                sketch_dim=sketch, fsa_fn=fsa_fn, trace=trace, residual_fn=get_loss_tracking_stacked,
                use_best_loss=False)
    n = min(len(trace), len(native))
    assert n == fo + so
    for i in range(n):
        (l1_p, st_p, _), (l1_n, st_n) = trace[i], native[i]
        assert abs(l1_n - l1_p) <= 2e-3 * l1_p, (i, l1_n, l1_p)
        assert abs(st_n - st_p) <= 2e-2 * st_p + 1e-6, (i, st_n, st_p)
    assert torch.allclose(vn.T, vp.T, atol=2e-4)


def test_alpha_one_with_depth_reproduces_the_monocular_tracker(built):
    """alpha = 1: the depth row is zero (w_depth = 0) and the colour rows are the monocular ones, so the RGB-D entry
    points follow the monocular trajectory (first and second order)."""
    from monogs_amd.pose import SE3_exp
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    target, depth, bg = _target(view, gauss, dev)
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.03, 0.004, -0.006, 0.003]))
    va, vb = _frame(view, 2, T0, target, depth), _frame(view, 3, T0, target, depth)
    ta = NativeTracker(va, gauss, bg)
    tb = NativeTracker(vb, gauss, bg, gt_depth=depth, alpha=1.0)
    for t in (ta, tb):
        t.enable_second_order(stack_dim=4, sketch_dim=16, seed=9)
        for _ in range(20):
            t.step()
        for _ in range(3):
            t.step_second_order()
    torch.cuda.synchronize()
    assert torch.allclose(va.T, vb.T, rtol=0, atol=1e-6)
    assert torch.allclose(va.exposure_a, vb.exposure_a, rtol=0, atol=1e-6)
    # the second order's bucket sums and L1 are float atomics (order-dependent in the last bits): the best L1 agrees
    # to float-sum precision, not bit for bit
    assert abs(float(ta.best_loss) - float(tb.best_loss)) <= 1e-4 * float(ta.best_loss)


def test_depth_drives_the_pose_along_the_optical_axis(built):
    """A texture-less scene - every Gaussian the grey of the background, so the image is one flat grey - seen from a
    pose offset 0.15 along the optical axis: colour does not constrain the pose at all, depth does.  After 100
    first-order iterations the RGB-D tracker's |t_z| error is below the monocular tracker's and at most a fifth of the
    offset.  (A grey map on a black background is not enough: its silhouettes alone brought the monocular tracker to
    0.025.)  Measured on an MI355X: |t_z| error 0.1406 monocular, 0.0265 RGB-D (bound 0.15 / 5 = 0.03)."""
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    grey = GaussianParams(gauss._xyz.detach(), gauss._scaling.detach(), gauss._rotation.detach(),
                          gauss._opacity.detach(), torch.full_like(gauss._features_dc.detach(), (0.3 - 0.5) / 0.28209479177387814))   # SH DC of grey 0.3
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    bg = torch.full((3,), 0.3, device=dev)
    with torch.no_grad():
        pkg = render(view(1, torch.eye(4)), grey, Pipe, bg)
    target, depth = pkg["render"].clone(), pkg["depth"].clone()
    off = 0.15
    T0 = SE3_exp(torch.tensor([0.0, 0.0, off, 0.0, 0.0, 0.0]))
    err = {}
    for name, kw in (("mono", {}), ("rgbd", {"gt_depth": depth, "alpha": 0.95})):
        v = _frame(view, 2, T0, target, depth)
        trk = NativeTracker(v, grey, bg, **kw)
        trk.run(max_iters=100, check_every=100, use_best_loss=False)
        err[name] = abs(float(v.T[2, 3]))
    print(f"|t_z| error after 100 iterations: mono {err['mono']:.5f}, rgbd {err['rgbd']:.5f} (offset {off})")
    assert err["rgbd"] < err["mono"]
    assert err["rgbd"] <= off / 5


def test_replica_shape_rgbd_iterations(built):
    """1200x680 and a 300 k map: first- and second-order RGB-D iterations run; dL/dtau of the first native iteration
    matches the drop-in Python step."""
    from monogs_amd import synthetic as S
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, ViewCamera
    from monogs_amd.tracking_native import NativeTracker
    dev = torch.device("cuda:0")
    W, H = 1200, 680
    sc = S.make_scene(300_000, W, H, 4)
    gauss = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev),
                           sc.opacity_logit.to(dev), sc.features_dc.to(dev))
    cam = sc.cam
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    view = lambda uid, T: ViewCamera(uid, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, dev)
    target, depth, bg = _target(view, gauss, dev)
    T0 = SE3_exp(torch.tensor([0.01, -0.01, 0.02, 0.002, -0.003, 0.002]))
    cfg = _cfg(0.95)
    va, vb = _frame(view, 2, T0, target, depth), _frame(view, 3, T0, target, depth)
    gt_tau, _, _, _ = _python_grads(va, gauss, bg, cfg)
    trk = NativeTracker(vb, gauss, bg, gt_depth=depth, alpha=0.95)
    n_tau, _, _ = _native_grads(trk)
    assert rel_err(n_tau, gt_tau) <= 2e-3
    for _ in range(4):
        trk.step()
    trk.enable_second_order()
    for _ in range(2):
        trk.step_second_order()
    assert trk.check_capacity()
    assert math.isfinite(float(trk.best_loss)) and bool(torch.isfinite(vb.T).all())


def test_rgbd_tracked_sequence_end_to_end(built):
    """run_sequence(sensor_depth=True, rgbd_tracking=True) over 20 frames: finite, and the SE(3)-aligned ATE stays
    under a bound set from the first measured run with 2x headroom (the monocular-tracked run on the same frames is
    printed beside it)."""
    from monogs_amd import slam_surrogate as SS
    dev = torch.device("cuda:0")
    frames, cam, _ = SS.load_sequence(20, 320, 240, dev, world_gaussians=40_000)
    out = {}
    for name, rgbd in (("mono", False), ("rgbd", True)):
        res = SS.run_sequence(frames, cam, dev, sensor_depth=True, rgbd_tracking=rgbd, init_iters=300,
                              mapping_iters=50, first_order_iters=40, second_order_iters=5)
        ev = SS.evaluate(res, frames, dev, every=5, monocular=False)
        out[name] = ev["ate_rmse_m"]
        assert math.isfinite(ev["ate_rmse_m"]) and all(bool(torch.isfinite(c.T).all()) for c in res["cameras"].values())
    print(f"SE(3)-aligned ATE over 20 frames: rgbd tracking {out['rgbd']:.5f} m, mono tracking {out['mono']:.5f} m")
    assert out["rgbd"] <= RGBD_ATE_BOUND


# first run on an MI355X: 0.0326 m with RGB-D tracking (0.0327 m monocular-tracked); bound = 2x
RGBD_ATE_BOUND = 0.065
