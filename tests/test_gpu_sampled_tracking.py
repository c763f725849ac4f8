"""Pixel-sampled first-order tracking on the GPU (mgs_tracking_iteration_sampled, NativeTracker(num_pixels=K)): the
sparse pose backward against the dense pose-only backward, the native iteration against the reference-shaped Python
mirror, the sampler's distribution and determinism, unbiasedness and convergence."""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_err
from test_raster_gpu import _loop_fixture

pytestmark = pytest.mark.gpu

T_OFF = (0.02, -0.015, 0.01, 0.004, -0.006, 0.003)


def _cfg(mono=True, use_huber=True, pnorm=1, alpha=0.95):
    from monogs_amd.slam_loops import DEFAULT_CONFIG
    t = dict(DEFAULT_CONFIG["Training"])
    t.update(monocular=mono, alpha=alpha, RGN={"use_huber": use_huber, "huber_delta": 0.01, "pnorm": pnorm})
    return {"Training": t}


def _setup(T0=None, rgbd=False, cfg=None, gt_noise=0.0, **kw):
    """(tracker, view, gauss, bg, cfg) on the small synthetic scene, the target rendered at the identity pose."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, tracking_norm
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        pkg = render(view(1, torch.eye(4)), gauss, Pipe, bg)
    target, depth = pkg["render"].clone(), pkg["depth"].clone()
    if gt_noise:
        target = target + gt_noise * torch.randn(target.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    cfg = cfg or _cfg(mono=not rgbd)

    def frame(uid):
        v = view(uid, SE3_exp(torch.tensor(T_OFF if T0 is None else T0)))
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
        v.gt_depth = depth if rgbd else None
        return v

    vn = frame(2)
    delta, p = tracking_norm(cfg)
    trk = NativeTracker(vn, gauss, bg, huber_delta=delta, pnorm=p, gt_depth=depth if rgbd else None,
                        alpha=cfg["Training"].get("alpha", 0.95), **kw)
    return trk, vn, frame, gauss, bg, cfg


def _dense_pose_grad(trk, vn, cfg, pix_weight):
    """The dense pose-only backward (mgs_raster_backward, every per-Gaussian pointer NULL) of the upstream
    d(sum_i pix_weight_i psi_i / p)/d(render) at the tracker's last render, and d/d(a, b) of the same sum - the
    un-normalised estimate for pix_weight = sum of 1 / (K q) over the draws of each pixel."""
    from monogs_amd import _cabi
    from monogs_amd.losses import HuberLoss, get_loss_tracking_stacked
    from monogs_amd.slam_loops import tracking_norm
    delta, p = tracking_norm(cfg)
    img = trk.color.detach().clone().requires_grad_()
    dep = trk.depth.detach().clone().requires_grad_()
    a = vn.exposure_a.detach().clone().requires_grad_()
    b = vn.exposure_b.detach().clone().requires_grad_()

    class VP:
        pass
    v = VP()
    v.exposure_a, v.exposure_b, v.exposure_eps = a, b, vn.exposure_eps
    v.original_image, v.rgb_pixel_mask_mapping, v.gt_depth = vn.original_image, vn.rgb_pixel_mask_mapping, vn.gt_depth
    res = get_loss_tracking_stacked(cfg, img, dep, trk.opacity.detach(), v)
    h = HuberLoss.apply(res, delta) if delta > 0 else res
    psi = h.abs().pow(p).sum(0).reshape(-1)
    ((psi * pix_weight).sum() / p).backward()
    lib = _cabi.lib()
    g_tau = torch.zeros(6, device=img.device)
    B = _cabi.BackwardArgs()
    C.memmove(C.byref(B.fwd), C.byref(trk.args.fwd), C.sizeof(_cabi.ForwardArgs))
    gc = img.grad.contiguous()
    gd = dep.grad.contiguous() if dep.grad is not None else None
    B.grad_color, B.grad_depth = gc.data_ptr(), (gd.data_ptr() if trk.depth_args is not None else None)
    B.bwd, B.grad_tau = trk.bwd.data_ptr(), g_tau.data_ptr()
    _cabi.check(lib.mgs_raster_backward(C.byref(B), trk._stream()), "mgs_raster_backward")
    torch.cuda.synchronize()
    return torch.cat([g_tau, a.grad, b.grad])


def _pix_weight(trk, vn, cfg, idx):
    """sum over the draws of each pixel of 1 / (K q_i), q from the tracker's last render (fp64 host arithmetic)."""
    from monogs_amd.losses import get_loss_tracking_stacked
    with torch.no_grad():
        res = get_loss_tracking_stacked(cfg, trk.color, trk.depth, trk.opacity, vn)
        v = (res.reshape(res.shape[0], -1).abs().sum(0) + 1e-8).double()
        w = torch.zeros_like(v)
        w.index_add_(0, idx.long(), v.sum() / (idx.numel() * v[idx.long()]))
    return w.float()


def _freeze(trk):
    """lr 0 for every group: the pose / exposure stay where they are, so the forward in the workspaces is that of the
    current state after a step (the Adam kernel rewrites identical camera matrices)."""
    A = trk.args.adam
    A.lr_rot = A.lr_trans = A.lr_a = A.lr_b = 0.0


@pytest.mark.parametrize("rgbd", [False, True])
def test_sparse_backward_equals_dense_backward(built, rgbd):
    """One fixed index set: duplicates, tile borders, background pixels, pixels no splat reaches, and K = 1."""
    dev = torch.device("cuda:0")
    H, W = 120, 160
    trk, vn, _, _, _, cfg = _setup(rgbd=rgbd, num_pixels=64)
    _freeze(trk)
    trk.step()                                               # a render to choose pixels from
    torch.cuda.synchronize()
    opa = trk.opacity.reshape(-1)
    bgpix = torch.nonzero(opa < 1e-6).reshape(-1)
    xs = [0, 15, 16, 31, 32, 47, 48, 159, 79, 80]
    ys = [0, 15, 16, 7, 8, 119, 60, 61, 112, 111]
    pix = [y * W + x for x, y in zip(xs, ys)]
    pix += [pix[1], pix[1], pix[2], pix[5]]                  # duplicates
    pix += bgpix[:4].tolist()                                # background (nothing reaches them), if any
    g = torch.Generator().manual_seed(7)
    pix += torch.randint(0, H * W, (64 - len(pix),), generator=g).tolist()
    idx = torch.tensor(pix[:64], dtype=torch.int32, device=dev)
    for sel in (idx, idx[3:4].contiguous()):
        if sel.numel() != trk.num_pixels:
            trk, vn, _, _, _, cfg = _setup(rgbd=rgbd, num_pixels=sel.numel())
            _freeze(trk)
        out = torch.zeros(8, device=dev)
        trk.step(replay_indices=sel, grad_out=out)
        torch.cuda.synchronize()
        assert sorted(trk.last_sample_indices.tolist()) == sorted(sel.tolist())
        want = _dense_pose_grad(trk, vn, cfg, _pix_weight(trk, vn, cfg, sel).to(dev))
        assert rel_err(out[:6], want[:6]) <= 1e-5, (out, want)
        assert rel_err(out[6:], want[6:]) <= 1e-5, (out, want)


@pytest.mark.parametrize("mode", ["mono_huber", "mono_p1", "rgbd_huber"])
def test_native_sampled_iterations_match_the_python_mirror(built, mode):
    """NativeTracker(num_pixels=K) step by step against slam_loops.tracking_step_first_order replaying the native
    draw (pixel_indices=last_sample_indices): pose, exposure and loss."""
    from monogs_amd.losses import get_loss_tracking_stacked
    from monogs_amd.slam_loops import Pipe, make_pose_optimizer, tracking_step_first_order
    rgbd = mode.startswith("rgbd")
    cfg = _cfg(mono=not rgbd, use_huber=mode != "mono_p1", pnorm=1)
    trk, vn, frame, gauss, bg, cfg = _setup(rgbd=rgbd, cfg=cfg, num_pixels=2048, sample_seed=3)
    vp = frame(3)
    opt = make_pose_optimizer(vp, cfg)
    fn = get_loss_tracking_stacked if rgbd else None
    for it in range(6):
        trk.step()
        loss_n = float(trk.loss)
        idx = trk.last_sample_indices.clone()
        loss_p, _, _ = tracking_step_first_order(vp, gauss, opt, bg, Pipe, cfg, residual_fn=fn, pixel_indices=idx)
        torch.cuda.synchronize()
        assert abs(loss_n - float(loss_p)) <= 1e-5 * abs(float(loss_p)), (it, loss_n, float(loss_p))
        assert (vn.T - vp.T).abs().max().item() <= 2e-6 * (it + 1), it
        assert abs(float(vn.exposure_a) - float(vp.exposure_a)) <= 2e-5 * (it + 1)
        assert abs(float(vn.exposure_b) - float(vp.exposure_b)) <= 2e-5 * (it + 1)


def test_sampler_is_keyed_and_deterministic(built):
    a, *_ = _setup(num_pixels=1024, sample_seed=11)
    b, *_ = _setup(num_pixels=1024, sample_seed=11)
    for t in (a, b):
        _freeze(t)
    a.step(); b.step()
    torch.cuda.synchronize()
    first = a.last_sample_indices.clone()
    assert torch.equal(first, b.last_sample_indices)          # same (seed, iteration): bit-identical draw
    a.step()
    torch.cuda.synchronize()
    assert not torch.equal(first, a.last_sample_indices)      # next iteration: another draw (same state)
    assert (a.last_sample_indices >= 0).all() and (a.last_sample_indices < 160 * 120).all()


def _draw_counts(trk, n_iter):
    counts = torch.zeros(trk.H * trk.W, dtype=torch.float64, device=trk.dev)
    for _ in range(n_iter):
        trk.step()
        counts.index_add_(0, trk.last_sample_indices.long(), torch.ones(trk.num_pixels, dtype=torch.float64,
                                                                         device=trk.dev))
    torch.cuda.synchronize()
    return counts


def _tile_sums(x, H=120, W=160):
    return x.reshape(H // 8, 8, W // 8, 8).sum((1, 3)).reshape(-1)


def test_sampler_matches_q_chi_square(built):
    """Draws pooled over iterations at a frozen state against q, on 8x8 pixel cells (300 cells)."""
    from monogs_amd.losses import get_loss_tracking_stacked
    trk, vn, _, _, _, cfg = _setup(num_pixels=4096, sample_seed=2, gt_noise=0.02)
    _freeze(trk)
    counts = _draw_counts(trk, 16)
    with torch.no_grad():
        res = get_loss_tracking_stacked(cfg, trk.color, trk.depth, trk.opacity, vn)
        v = (res.reshape(3, -1).abs().sum(0) + 1e-8).double()
    n = counts.sum()
    exp = _tile_sums(v / v.sum()) * n
    obs = _tile_sums(counts)
    keep = exp > 5
    chi2 = float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    dof = int(keep.sum()) - 1
    assert chi2 < dof + 6 * math.sqrt(2 * dof), (chi2, dof)


def test_zero_residual_pixels_are_drawn_at_the_floor_rate(built):
    """gt = the render at the current pose: every residual is 0, v = 1e-8 everywhere and the draw is uniform; with a
    residual in one 8x8 block only, zero-residual pixels are drawn at the 1e-8 rate (Poisson, expectation < 0.1)."""
    trk, vn, _, gauss, bg, cfg = _setup(num_pixels=4096, sample_seed=5)
    trk.mask = None
    trk.args.loss.mask = None
    _freeze(trk)
    trk.step()                                   # the state does not move: this is the render of every later step
    torch.cuda.synchronize()
    trk.gt.copy_(trk.color)
    counts = _draw_counts(trk, 8)
    obs = _tile_sums(counts)
    exp = obs.sum() / obs.numel()
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    dof = obs.numel() - 1
    assert chi2 < dof + 6 * math.sqrt(2 * dof), (chi2, dof)
    # one hot 8x8 block
    cell = int(torch.argmax(_tile_sums(trk.opacity.reshape(-1).double())))     # the most opaque 8x8 cell
    y0, x0 = 8 * (cell // 20), 8 * (cell % 20)
    trk.gt[:, y0:y0 + 8, x0:x0 + 8] += 0.5
    counts = _draw_counts(trk, 8)
    hot = torch.zeros(120, 160, dtype=torch.bool, device=trk.dev)
    hot[y0:y0 + 8, x0:x0 + 8] = True
    cold = float(counts[~hot.reshape(-1)].sum())
    # expected cold draws: 32768 * (19136e-8 / (64 * 0.5 * 3 * opacity ~ 50)) ~ 0.1
    assert cold <= 4, cold
    assert float(counts[hot.reshape(-1)].sum()) >= 32768 - 4


def test_sampled_gradient_is_unbiased(built):
    """Mean of the estimate over 256 draws within 4 standard errors of the dense gradient, every component."""
    dev = torch.device("cuda:0")
    trk, vn, _, _, _, cfg = _setup(num_pixels=256, sample_seed=9)
    _freeze(trk)
    outs = []
    for _ in range(256):
        o = torch.zeros(8, device=dev)
        trk.step(grad_out=o)
        outs.append(o)
    torch.cuda.synchronize()
    G = torch.stack(outs).double()
    want = _dense_pose_grad(trk, vn, cfg, torch.ones(120 * 160, device=dev)).double()
    mean, se = G.mean(0), G.std(0) / math.sqrt(G.shape[0])
    assert ((mean - want).abs() <= 4 * se + 1e-6 * want.abs().max()).all(), (mean, want, se)


def test_sampled_tracking_converges(built):
    """From a pose offset, 60 sampled iterations (K = 4096, fixed seed) reduce the pose error and end within 3x of
    the dense run's error."""
    def err(v):
        return (v.T - torch.eye(4, device=v.T.device)).abs().max().item()
    dense, vd, *_ = _setup()
    samp, vs, *_ = _setup(num_pixels=4096, sample_seed=1)
    e0 = err(vs)
    for _ in range(60):
        dense.step()
        samp.step()
    torch.cuda.synchronize()
    assert err(vs) < 0.3 * e0, (err(vs), e0)
    assert err(vs) <= 3.0 * err(vd) + 1e-3, (err(vs), err(vd))


def test_default_path_is_unchanged(built):
    a, va, *_ = _setup()
    b, vb, *_ = _setup(num_pixels=-1, sample_seed=4)
    for _ in range(8):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(va.T, vb.T) and torch.equal(va.exposure_a, vb.exposure_a)
    assert torch.equal(a.loss, b.loss) and b.last_sample_indices is None


@pytest.mark.parametrize("rgbd", [False, True])
def test_sampled_runs_are_bit_identical(built, rgbd):
    a, va, *_ = _setup(rgbd=rgbd, num_pixels=4096, sample_seed=8)
    b, vb, *_ = _setup(rgbd=rgbd, num_pixels=4096, sample_seed=8)
    for _ in range(10):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(va.T, vb.T) and torch.equal(va.exposure_a, vb.exposure_a) and torch.equal(va.exposure_b, vb.exposure_b)
    assert torch.equal(a.last_sample_indices, b.last_sample_indices) and torch.equal(a.loss, b.loss)


def test_run_and_limits(built):
    """run() takes the sampled step; K above the documented maximum is refused."""
    from monogs_amd import _cabi
    trk, vn, *_ = _setup(num_pixels=1024, sample_seed=2)
    it = trk.run(max_iters=20, check_every=10)
    assert it >= 1 and math.isfinite(float(trk.best_loss))
    with pytest.raises(ValueError):
        _setup(num_pixels=_cabi.TRACK_SAMPLE_MAX + 1)
