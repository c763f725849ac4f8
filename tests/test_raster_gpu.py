"""GPU parity tests: HIP rasteriser (through the C ABI + autograd binding) against the
autograd oracle (small sizes) and the C++ host emulation (full BASELINE sizes).

Tolerances (BASELINE.json north_star): forward image L1 <= 1e-4; backward gradients
<= 1e-3 relative (norm-wise: the alpha>=1/255 and T<1e-4 cut-offs are discontinuous, so a
handful of (pixel, splat) pairs may flip between two fp32 implementations).

These are aggregates: they do not see a few dropped pairs or wrong small gradient rows.  The per-pixel / per-row
comparison with the oracle's own flip allowance is tests/test_gpu_raster_parity.py (helper tests/raster_parity.py;
DESIGN.md section 2, "How parity is held").
"""
import pytest
import numpy as np
import torch

from conftest import gpu_settings, oracle_settings, rel_err
from map_models import _make_model, _state_of

pytestmark = pytest.mark.gpu

FWD_L1 = 1e-4
BWD_REL = 1e-3


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _inputs(sc, deg=0, seed=1):
    from monogs_amd import synthetic as S
    m, s, r, o, sh = S.activated(sc)
    if deg > 0:
        g = torch.Generator().manual_seed(seed)
        K = (deg + 1) ** 2
        sh = torch.cat([sh, 0.3 * torch.randn(sh.shape[0], K - 1, 3, generator=g)], 1)
    return m, s, r, o, sh


def _run_gpu(sc, st, m, s, r, o, sh, col=None, cov=None, backward=True, loss_fn=None):
    from monogs_amd import synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    req = lambda t: None if t is None else t.clone().to(dev).requires_grad_()
    L = dict(m=req(m), s=req(s), r=req(r), o=req(o), sh=req(sh), col=req(col), cov=req(cov))
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    m2d = torch.zeros(m.shape[0], 3, device=dev, requires_grad=True)
    out = GaussianRasterizer(st)(means3D=L["m"], means2D=m2d, shs=L["sh"], colors_precomp=L["col"],
                                 opacities=L["o"], scales=L["s"], rotations=L["r"],
                                 cov3D_precomp=L["cov"], theta=theta, rho=rho)
    img, radii, dep, opa, nt = out
    if backward:
        loss = (loss_fn or (lambda i, d: S.synthetic_loss(i, d, sc)))(img, dep)
        loss.backward()
    torch.cuda.synchronize()
    return out, L, theta, rho, m2d


def _run_oracle(sc, st, m, s, r, o, sh, col=None, cov=None, loss_fn=None):
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    req = lambda t: None if t is None else t.clone().requires_grad_()
    L = dict(m=req(m), s=req(s), r=req(r), o=req(o), sh=req(sh), col=req(col), cov=req(cov))
    theta = torch.zeros(3, requires_grad=True)
    rho = torch.zeros(3, requires_grad=True)
    m2d = torch.zeros(m.shape[0], 3, requires_grad=True)
    img, radii, dep, opa, nt, info = O.rasterize(L["m"], m2d, L["sh"], L["col"], L["o"], L["s"],
                                                 L["r"], L["cov"], st, theta, rho)
    loss = (loss_fn or (lambda i, d: S.synthetic_loss(i, d, sc)))(img, dep)
    loss.backward()
    return (img, radii, dep, opa, nt), L, theta, rho, m2d, info


def _compare(gpu, ora, check_sr=True):
    (gimg, gradii, gdep, gopa, gnt), GL, gth, grh, gm2d = gpu
    (oimg, oradii, odep, oopa, ont), OL, oth, orh, om2d = ora[:5]
    assert (gimg.cpu() - oimg).abs().mean().item() <= FWD_L1
    assert (gdep.cpu() - odep).abs().mean().item() <= 5e-4
    assert (gopa.cpu() - oopa).abs().mean().item() <= FWD_L1
    assert (gradii.cpu() != oradii).float().mean().item() <= 1e-3
    nt_bad = (gnt.cpu() != ont).float().sum().item()
    assert nt_bad <= max(2, 0.01 * (ont > 0).sum().item()), nt_bad
    assert rel_err(GL["m"].grad, OL["m"].grad) <= BWD_REL
    assert rel_err(gm2d.grad, om2d.grad) <= BWD_REL
    assert gm2d.grad[:, 2].abs().max().item() == 0.0
    assert rel_err(GL["o"].grad, OL["o"].grad) <= BWD_REL
    if GL["sh"] is not None:
        assert rel_err(GL["sh"].grad, OL["sh"].grad) <= BWD_REL
    if GL["col"] is not None:
        assert rel_err(GL["col"].grad, OL["col"].grad) <= BWD_REL
    if check_sr and GL["s"] is not None:
        assert rel_err(GL["s"].grad, OL["s"].grad) <= BWD_REL
        assert rel_err(GL["r"].grad, OL["r"].grad) <= BWD_REL
    if GL["cov"] is not None:
        assert rel_err(GL["cov"].grad, OL["cov"].grad) <= BWD_REL
    tau_g = torch.cat([grh.grad, gth.grad])
    tau_o = torch.cat([orh.grad, oth.grad])
    assert rel_err(tau_g, tau_o) <= 2e-3


def test_small_sh0(built):
    from monogs_amd import synthetic as S
    sc = S.make_scene(2000, 160, 120, seed=3)
    inp = _inputs(sc)
    bg = torch.tensor([0.1, 0.3, 0.2])
    gpu = _run_gpu(sc, gpu_settings(sc.cam, bg, _dev()), *inp)
    ora = _run_oracle(sc, oracle_settings(sc.cam, bg), *inp)
    _compare(gpu, ora)


def test_syn_a_config1(built):
    """BASELINE config 1 shape: 5k Gaussians @160x120, one fwd+bwd."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(5000, 160, 120, seed=0)
    inp = _inputs(sc)
    gpu = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev()), *inp)
    ora = _run_oracle(sc, oracle_settings(sc.cam, sc.bg), *inp)
    _compare(gpu, ora)


def test_sh_degree3_and_campos(built):
    from monogs_amd import synthetic as S
    sc = S.make_scene(1500, 128, 96, seed=5)
    inp = _inputs(sc, deg=3)
    campos = torch.tensor([0.1, -0.2, -0.5])
    bg = torch.tensor([0.0, 0.5, 1.0])
    gpu = _run_gpu(sc, gpu_settings(sc.cam, bg, _dev(), deg=3, campos=campos), *inp)
    ora = _run_oracle(sc, oracle_settings(sc.cam, bg, deg=3, campos=campos), *inp)
    _compare(gpu, ora)


def test_active_degree_below_stored(built):
    """MonoGS stores K coefficients but may render with a lower active degree."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(800, 96, 64, seed=6)
    inp = _inputs(sc, deg=2)
    campos = torch.tensor([0.0, 0.1, -0.3])
    gpu = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev(), deg=1, campos=campos), *inp)
    ora = _run_oracle(sc, oracle_settings(sc.cam, sc.bg, deg=1, campos=campos), *inp)
    _compare(gpu, ora)


def test_precomputed_cov_and_colors(built):
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    sc = S.make_scene(1200, 112, 80, seed=7)
    m, s, r, o, sh = _inputs(sc)
    Sig = O.cov3d_from_scale_rot(s, r, 1.0)
    cov6 = torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2],
                        Sig[:, 2, 2]], 1).contiguous()
    col = torch.rand(m.shape[0], 3, generator=torch.Generator().manual_seed(2))
    gpu = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev()), m, None, None, o, None, col, cov6)
    ora = _run_oracle(sc, oracle_settings(sc.cam, sc.bg), m, None, None, o, None, col, cov6)
    _compare(gpu, ora)


def test_odd_image_size_and_moved_camera(built):
    """W,H not multiples of 16 and a non-identity pose (rotation + translation)."""
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    sc = S.make_scene(1500, 150, 101, seed=8)
    T = O.se3_exp(torch.tensor([0.05, -0.03, 0.1, 0.02, -0.04, 0.03]))
    cam = S.make_camera(150, 101, T)
    sc = sc._replace(cam=cam)
    inp = _inputs(sc)
    gpu = _run_gpu(sc, gpu_settings(cam, sc.bg, _dev()), *inp)
    ora = _run_oracle(sc, oracle_settings(cam, sc.bg), *inp)
    _compare(gpu, ora)


def test_scale_modifier_and_isotropic_broadcast(built):
    """render() repeats [N,1] isotropic scales to [N,3] (gaussian_renderer/__init__.py:92-93)."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(1000, 96, 80, seed=9)
    m, s, r, o, sh = _inputs(sc)
    s = s[:, :1].repeat(1, 3).contiguous()
    gpu = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev(), scale_modifier=0.7), m, s, r, o, sh)
    ora = _run_oracle(sc, oracle_settings(sc.cam, sc.bg, scale_modifier=0.7), m, s, r, o, sh)
    _compare(gpu, ora)


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_configurations_match_the_oracle(built, seed):
    """A seeded sweep over the argument space of the rasteriser's call (gaussian_renderer/__init__.py:61-75,151-168):
    map size 1 ... 3000, image sizes that are not multiples of the tile, a moved camera, SH degree 0 ... 3 with an
    active degree at or below the stored one, scale / rotation or a precomputed covariance, SH or precomputed colours,
    isotropic scales, a scale modifier, a random background, depth gradients on or off: forward outputs and every
    gradient sink against the autograd oracle on the same inputs."""
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    g = torch.Generator().manual_seed(1000 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    rf = lambda lo, hi: float(lo + (hi - lo) * torch.rand(1, generator=g))
    W, H = ri(33, 200), ri(17, 150)
    N = [1, 2, 37, 300, 1000, 3000][seed % 6] if seed < 6 else ri(1, 3000)
    sc = S.make_scene(N, W, H, seed=50 + seed)
    tau = torch.tensor([rf(-0.08, 0.08), rf(-0.08, 0.08), rf(-0.1, 0.1), rf(-0.05, 0.05), rf(-0.05, 0.05), rf(-0.05, 0.05)])
    cam = S.make_camera(W, H, O.se3_exp(tau))
    sc = sc._replace(cam=cam)
    stored = ri(0, 3)
    active = ri(0, stored)
    m, s_, r_, o, sh = _inputs(sc, deg=stored, seed=seed)
    bg = torch.rand(3, generator=g)
    mod = [1.0, 0.7, 1.3][ri(0, 2)]
    campos = torch.linalg.inv(cam.viewmatrix.T)[:3, 3].contiguous() if ri(0, 1) else None     # true centre or MonoGS's quirk
    use_cov, use_col, iso = ri(0, 3) == 0, ri(0, 3) == 0, ri(0, 3) == 0
    col = cov6 = None
    if iso:
        s_ = s_[:, :1].repeat(1, 3).contiguous()
    if use_cov:
        Sig = O.cov3d_from_scale_rot(s_, r_, mod)
        cov6 = torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], 1).contiguous()
        s_ = r_ = None
    if use_col:
        col, sh = torch.rand(N, 3, generator=g), None
    deg = 0 if use_col else active
    gi, gd = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g) * (0.0 if seed % 4 == 3 else 0.3)
    loss_fn = lambda i, d: (i * gi.to(i.device)).sum() / (H * W) + (d * gd.to(d.device)).sum() / (H * W)
    gpu = _run_gpu(sc, gpu_settings(cam, bg, _dev(), deg=deg, campos=campos, scale_modifier=mod), m, s_, r_, o, sh, col, cov6,
                   loss_fn=loss_fn)
    ora = _run_oracle(sc, oracle_settings(cam, bg, deg=deg, campos=campos, scale_modifier=mod), m, s_, r_, o, sh, col, cov6,
                      loss_fn=loss_fn)
    _compare(gpu, ora)


def test_everything_culled_and_single_gaussian(built):
    from monogs_amd import synthetic as S
    dev = _dev()
    sc = S.make_scene(64, 64, 48, seed=1)
    m, s, r, o, sh = _inputs(sc)
    behind = m.clone()
    behind[:, 2] = -1.0
    (img, radii, dep, opa, nt), L, th, rh, m2d = _run_gpu(
        sc, gpu_settings(sc.cam, torch.tensor([0.2, 0.4, 0.6]), dev), behind, s, r, o, sh)
    assert (radii == 0).all() and (nt == 0).all()
    assert torch.allclose(img.cpu(), torch.tensor([0.2, 0.4, 0.6])[:, None, None].expand(3, 48, 64))
    assert (dep == 0).all() and (opa == 0).all()
    assert L["m"].grad.abs().max().item() == 0 and rh.grad.abs().max().item() == 0
    one = lambda t: t[:1].contiguous()
    gpu = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, dev), one(m), one(s) * 4, one(r), one(o), one(sh))
    ora = _run_oracle(sc, oracle_settings(sc.cam, sc.bg), one(m), one(s) * 4, one(r), one(o), one(sh))
    _compare(gpu, ora)


def test_backward_is_reentrant(built):
    """slam_frontend.py:654-666 calls backward repeat_dim times with retain_graph=True."""
    from monogs_amd import synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    sc = S.make_scene(1500, 128, 96, seed=4)
    m, s, r, o, sh = [t.to(dev).requires_grad_() for t in _inputs(sc)]
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    m2d = torch.zeros(1500, 3, device=dev, requires_grad=True)
    img, radii, dep, opa, nt = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))(
        means3D=m, means2D=m2d, shs=sh, opacities=o, scales=s, rotations=r, theta=theta, rho=rho)
    loss = S.synthetic_loss(img, dep, sc)
    loss.backward(retain_graph=True)
    g1, t1 = m.grad.clone(), theta.grad.clone()
    m.grad = None
    theta.grad = None
    loss.backward()
    torch.cuda.synchronize()
    assert rel_err(g1, m.grad) < 1e-5 and rel_err(t1, theta.grad) < 1e-5


def test_capacity_retry_gives_identical_result(built):
    from monogs_amd import rasterizer as R
    from monogs_amd import synthetic as S
    dev = _dev()
    sc = S.make_scene(3000, 160, 120, seed=2)
    inp = _inputs(sc)
    st = gpu_settings(sc.cam, sc.bg, dev)
    a = _run_gpu(sc, st, *inp)
    pairs = R.last_stats["pairs"]
    R._capacity_hint[dev.index] = 1024          # far too small -> stage 2 must be re-run
    b = _run_gpu(sc, st, *inp)
    assert R.last_stats["retried"] and R.last_stats["pairs"] == pairs
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][4], b[0][4])
    assert rel_err(a[1]["m"].grad, b[1]["m"].grad) < 1e-5


def test_pair_count_matches_exact_culling_emulation(built):
    from monogs_amd import rasterizer as R
    from monogs_amd import synthetic as S
    from oracle.host_emul import HostEmul
    sc = S.make_scene(5000, 160, 120, seed=0)
    inp = _inputs(sc)
    _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev()), *inp, backward=False)
    em = HostEmul()
    m, s, r, o, sh = inp
    em.forward(oracle_settings(sc.cam, sc.bg), m, sh, None, o, s, r, None, exact_cull=True)
    assert abs(R.last_stats["pairs"] - em.pairs) <= max(2, em.pairs // 1000)


@pytest.mark.parametrize("N,backward", [(100_000, False), (300_000, True)])
def test_full_size_against_host_emulation(built, N, backward):
    """BASELINE configs 2 and 3: 640x480, 100k forward / 300k forward+backward, checked
    against the multi-threaded C++ host emulation (itself pinned to the autograd oracle
    by the CPU tests)."""
    from monogs_amd import synthetic as S
    from oracle.host_emul import HostEmul
    sc = S.make_scene(N, 640, 480, seed=0)
    inp = _inputs(sc)
    m, s, r, o, sh = inp
    gpu = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev()), *inp, backward=backward)
    (img, radii, dep, opa, nt), L, th, rh, m2d = gpu
    em = HostEmul()
    eimg, eradii, edep, eopa, ent = em.forward(oracle_settings(sc.cam, sc.bg), m, sh, None, o, s,
                                               r, None, exact_cull=False)
    assert (img.cpu() - eimg).abs().mean().item() <= FWD_L1
    assert (dep.cpu() - edep).abs().mean().item() <= 5e-4
    assert (opa.cpu() - eopa).abs().mean().item() <= FWD_L1
    assert (radii.cpu() != eradii).float().mean().item() <= 1e-4
    assert (nt.cpu() != ent).float().mean().item() <= 1e-3
    if backward:
        gi = img.detach().cpu().requires_grad_()
        gd = dep.detach().cpu().requires_grad_()
        S.synthetic_loss(gi, gd, sc).backward()
        out = em.backward(gi.grad, gd.grad)
        assert rel_err(L["m"].grad, out["means3D"]) <= BWD_REL
        assert rel_err(m2d.grad, out["means2D"]) <= BWD_REL
        assert rel_err(L["sh"].grad, out["colors"]) <= BWD_REL
        assert rel_err(L["o"].grad.reshape(-1), out["opacities"]) <= BWD_REL
        assert rel_err(L["s"].grad, out["scales"]) <= BWD_REL
        assert rel_err(L["r"].grad, out["rotations"]) <= BWD_REL
        assert rel_err(torch.cat([rh.grad, th.grad]), out["tau"]) <= 2e-3


def test_no_gradient_through_opacity_output(built):
    """The extension's backward receives only grad_out_color and grad_out_depth: a loss on
    the `opacity` output alone produces zero gradients."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(500, 64, 48, seed=11)
    inp = _inputs(sc)
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    m, s, r, o, sh = [t.to(dev).requires_grad_() for t in inp]
    img, radii, dep, opa, nt = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))(
        means3D=m, means2D=torch.zeros(500, 3, device=dev, requires_grad=True), shs=sh,
        opacities=o, scales=s, rotations=r)
    (opa.sum() + 0 * img.sum()).backward()
    assert m.grad.abs().max().item() == 0 and o.grad.abs().max().item() == 0


def test_argument_validation(built):
    from monogs_amd import synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    sc = S.make_scene(16, 32, 32)
    m, s, r, o, sh = [t.to(dev) for t in _inputs(sc)]
    ras = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))
    z = torch.zeros(16, 3, device=dev)
    with pytest.raises(Exception):
        ras(means3D=m, means2D=z, opacities=o, shs=sh, colors_precomp=z, scales=s, rotations=r)
    with pytest.raises(Exception):
        ras(means3D=m, means2D=z, opacities=o, shs=sh)
    with pytest.raises(RuntimeError):
        ras(means3D=m.cpu(), means2D=z.cpu(), opacities=o.cpu(), shs=sh.cpu(), scales=s.cpu(),
            rotations=r.cpu())
    # the fork's num_backward_gaussians keyword: -1 (every shipped configuration) is accepted, a limit is refused
    # loudly - its semantics live in the absent CUDA source
    ras(means3D=m, means2D=z, opacities=o, shs=sh, scales=s, rotations=r, num_backward_gaussians=-1)
    with pytest.raises(NotImplementedError):
        ras(means3D=m, means2D=z, opacities=o, shs=sh, scales=s, rotations=r, num_backward_gaussians=300)


def test_backward_with_a_pair_count_bound_below_the_true_count_is_flagged(built):
    """mgs_backward_args.pair_count_bound sizes the blend grid; a value below the forward's pair count would lose
    work items silently.  The kernel flags it in counters[2] of the geom workspace, and the binding - which passes the
    exact count - raises in debug mode (raster_settings.debug, as the upstream extension checks only then)."""
    from monogs_amd import synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    sc = S.make_scene(3000, 160, 120, seed=2)
    for debug in (False, True):
        st = gpu_settings(sc.cam, sc.bg, dev)._replace(debug=debug)
        m, s, r, o, sh = [t.to(dev).requires_grad_() for t in _inputs(sc)]
        m2d = torch.zeros(3000, 3, device=dev, requires_grad=True)
        img, radii, dep, opa, nt = GaussianRasterizer(st)(means3D=m, means2D=m2d, opacities=o, shs=sh, scales=s, rotations=r)
        ctx = img.grad_fn                     # the autograd Function's ctx
        geom = ctx.saved_tensors[12]
        D = int(ctx.pairs)
        assert D > 2000
        from monogs_amd.rasterizer import _sizes
        from monogs_amd import _cabi
        N, W, H, deg, K, cap = ctx.shape_tuple
        off = int(_sizes(_cabi.RasterShape(N, W, H, deg, K, cap, float(st.tanfovx), float(st.tanfovy), 1.0)).off_counters)
        flag = lambda: int(geom[off + 8:off + 12].view(torch.int32).item())
        img.sum().backward(retain_graph=True)
        assert flag() == 0                    # the exact count covers every item
        good = m.grad.clone()
        m.grad = None
        ctx.pairs = 64                        # a bound far below D: grid of 64 / 32 + T items
        if debug:
            with pytest.raises(RuntimeError, match="pair_count_bound"):
                img.sum().backward()
        else:
            img.sum().backward()
            # (the gradients themselves may even look right here: the unwalked items' pair records still hold what the
            # complete backward above left in the per-stream scratch - which is why the flag exists)
            assert flag() > 64 // 32 + 80


def test_knn_dist2(built):
    from monogs_amd.knn import distCUDA2
    from oracle import torch_raster as O
    g = torch.Generator().manual_seed(0)
    for P in (4, 257, 4800):
        pts = torch.rand(P, 3, generator=g) * torch.tensor([4.0, 3.0, 6.0])
        got = distCUDA2(pts.to(_dev())).cpu()
        want = O.dist2_knn3(pts)
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-7), P
    # fewer than four points: a missing neighbour counts as FLT_MAX (see the oracle's docstring)
    for P in (1, 2, 3):
        pts = torch.rand(P, 3, generator=g)
        got = distCUDA2(pts.to(_dev())).cpu()
        want = O.dist2_knn3(pts)
        assert got.shape == (P,) and torch.equal(torch.isinf(got), torch.isinf(want)), (P, got, want)
        fin = torch.isfinite(want)
        assert torch.allclose(got[fin], want[fin], rtol=1e-6) and bool((got > 1e37).all()), (P, got, want)
    assert distCUDA2(torch.zeros(0, 3, device=_dev())).shape == (0,)


# ---------------------------------------------------------------------------------------
# sketched pose Jacobian (row a9) and the loop bodies (rows a12 / a13)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,W,H,repeat,stack,sketch,moved", [(600, 64, 48, 2, 2, 4, False), (500, 70, 45, 1, 3, 5, True)])
def test_sketched_pose_jacobian_matches_oracle(built, N, W, H, repeat, stack, sketch, moved):
    """Same construction as the reference's only hot-path self check
    (utils/slam_frontend.py:1031-1127): the sketched Jacobian row of every bucket must equal
    the plain autograd gradient of that bucket's summed residual w.r.t. (trans, rot).  Here
    the right-hand side comes from the CPU oracle instead of the extension itself.
    Second case: an image that is not a whole number of tiles (the per-tile slabs of Jacobian rows at the image
    border), a pixel count that the buckets do not divide (left-over pixels belong to no bucket) and a moved camera."""
    from monogs_amd import synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    from monogs_amd.slam_loops import gen_forward_sketch_args
    from oracle import torch_raster as O
    dev = _dev()
    sc = S.make_scene(N, W, H, seed=12)
    if moved:
        sc = sc._replace(cam=S.make_camera(W, H, O.se3_exp(torch.tensor([0.04, -0.03, 0.08, 0.02, -0.03, 0.02]))))
    m, s, r, o, sh = _inputs(sc)
    s = s * 1.5
    g = torch.Generator().manual_seed(3)
    Aimg = torch.randn(3, H, W, generator=g)
    Bdep = torch.randn(1, H, W, generator=g)
    fsa = gen_forward_sketch_args(H, W, repeat, stack, sketch, "cpu", generator=g)
    idx = fsa["sketch_indices"]                       # [repeat, stack, H, W]
    wts = fsa["rand_weights"]                         # [repeat, H, W]

    # HIP
    L = [t.to(dev).requires_grad_() for t in (m, s, r, o, sh)]
    theta = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    sk = torch.empty(stack, sketch, 6, device=dev, requires_grad=True)
    img, radii, dep, opa, nt = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))(
        means3D=L[0], means2D=torch.zeros(N, 3, device=dev, requires_grad=True), shs=L[4],
        opacities=L[3], scales=L[1], rotations=L[2], theta=theta, rho=rho, sketch_mode=1,
        sketch_dim=sketch, stack_dim=stack, sketch_dtau=sk, sketch_indices=idx.to(dev))
    res = (img * Aimg.to(dev)).sum(0) + (dep * Bdep.to(dev))[0]
    weighted = res[None] * wts.to(dev)
    SJ = []
    for i in range(repeat):
        sk.grad = None
        theta.grad = None
        rho.grad = None
        weighted[i].backward(gradient=torch.ones_like(weighted[i]), retain_graph=True)
        SJ.append(sk.grad.clone().cpu())
        full = torch.cat([rho.grad, theta.grad]).cpu()
        # every pixel of the permutation prefix is in exactly one bucket per repeat, so the
        # rows of ALL stacks together add up to the pose gradient over the covered pixels
        covered = (idx[i] >= 0).any(0)
        if bool(covered.all()):
            assert rel_err(SJ[-1].sum((0, 1)), full) < 2e-3

    # oracle
    Lc = [t.clone().requires_grad_() for t in (m, s, r, o, sh)]
    th_c = torch.zeros(3, requires_grad=True)
    rh_c = torch.zeros(3, requires_grad=True)
    oimg, _, odep, _, _, _ = O.rasterize(Lc[0], None, Lc[4], None, Lc[3], Lc[1], Lc[2], None,
                                         oracle_settings(sc.cam, sc.bg), th_c, rh_c)
    ores = (oimg * Aimg).sum(0) + (odep * Bdep)[0]
    worst = 0.0
    scale = max(x.abs().max().item() for x in SJ)
    for i in range(repeat):
        ow = ores * wts[i]
        for st_ in range(stack):
            for k in range(sketch):
                th_c.grad = None
                rh_c.grad = None
                ow[idx[i, st_] == k].sum().backward(retain_graph=True)
                want = torch.cat([rh_c.grad, th_c.grad])
                worst = max(worst, (SJ[i][st_, k] - want).abs().max().item())
    assert worst <= 2e-3 * scale, (worst, scale)


def _loop_fixture(N=4000, W=160, H=120, seed=21):
    from monogs_amd import synthetic as S
    from monogs_amd.slam_loops import GaussianParams, ViewCamera
    import math
    dev = _dev()
    sc = S.make_scene(N, W, H, seed)
    gauss = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev),
                           sc.opacity_logit.to(dev), sc.features_dc.to(dev))
    cam = sc.cam
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)

    def view(uid, T):
        return ViewCamera(uid, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, dev)

    return sc, gauss, view, dev


def test_tracking_first_order_recovers_a_perturbed_pose(built):
    """Row a12: render -> per-pixel residual -> Huber/L2 -> backward -> Adam -> update_pose
    must pull a perturbed camera back towards the pose the target image was rendered from."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, make_pose_optimizer, tracking_step_first_order
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    gt_cam = view(1, torch.eye(4))
    with torch.no_grad():
        target = render(gt_cam, gauss, Pipe, bg)["render"].clone()
    vp = view(2, SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003])))
    vp.original_image = target
    vp.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    opt = make_pose_optimizer(vp)
    err0 = (vp.T - torch.eye(4, device=dev)).norm().item()
    losses = []
    for _ in range(60):
        loss, conv, _ = tracking_step_first_order(vp, gauss, opt, bg)
        losses.append(loss.item())
    err1 = (vp.T - torch.eye(4, device=dev)).norm().item()
    assert losses[-1] < 0.6 * losses[0] and err1 < 0.5 * err0, (losses[0], losses[-1], err0, err1)
    assert vp.cam_rot_delta.abs().sum() == 0     # deltas are zeroed by update_pose


def test_tracking_second_order_sketched_step_reduces_the_residual(built):
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, tracking_step_second_order
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    vp = view(2, SE3_exp(torch.tensor([0.006, -0.004, 0.003, 0.001, -0.002, 0.001])))
    vp.original_image = target
    vp.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    gen = torch.Generator(device=dev).manual_seed(0)
    err0 = (vp.T - torch.eye(4, device=dev)).norm().item()
    for _ in range(6):
        tracking_step_second_order(vp, gauss, bg, lambda_=1e-3, repeat_dim=1, stack_dim=4,
                                   sketch_dim=16, generator=gen)
    err1 = (vp.T - torch.eye(4, device=dev)).norm().item()
    assert err1 < 0.5 * err0, (err0, err1)


def test_mapping_step_over_a_keyframe_window(built):
    """Row a13: several renders, one summed loss, one backward; the statistics consumed by
    densification must agree with per-view recomputation."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.parallel import view_pose
    from monogs_amd.slam_loops import Pipe, mapping_step
    sc, gauss, view, dev = _loop_fixture(N=3000)
    bg = torch.zeros(3, device=dev)
    window = []
    for i in range(3):
        v = view(i, view_pose(i))
        v.original_image = sc.gt_image.to(dev)
        v.rgb_pixel_mask_mapping = torch.ones(1, 120, 160, dtype=torch.bool, device=dev)
        window.append(v)
    opt = torch.optim.Adam([{"params": [gauss._xyz], "lr": 1e-4}, {"params": [gauss._features_dc], "lr": 2.5e-3},
                            {"params": [gauss._opacity], "lr": 0.05}, {"params": [gauss._scaling], "lr": 1e-3},
                            {"params": [gauss._rotation], "lr": 1e-3}])
    kf_opt = torch.optim.Adam([p for v in window for p in (v.cam_rot_delta, v.cam_trans_delta)], lr=1e-3)
    l0, stat, denom, radii = mapping_step(window, gauss, opt, kf_opt, bg)
    vis = torch.zeros_like(denom)
    rad = torch.zeros_like(radii)
    with torch.no_grad():
        for v in window:
            pkg = render(v, gauss, Pipe, bg)
            # poses moved by at most one tiny Adam step: visibility counts agree up to a few splats
            vis += pkg["visibility_filter"].float()
            rad = torch.maximum(rad, pkg["radii"])
    assert (vis - denom).abs().sum() <= 0.01 * denom.sum()
    assert stat.isfinite().all() and (stat >= 0).all() and stat.max() > 0
    for _ in range(10):
        l1, *_ = mapping_step(window, gauss, opt, kf_opt, bg)
    assert l1 < l0


# ---------------------------------------------------------------------------------------
# stress shapes: every alternative code path of the binning / sort / blend kernels
# ---------------------------------------------------------------------------------------
def _against_emulation(sc, m, s, r, o, sh, bg=None, bwd_tol=BWD_REL):
    from monogs_amd import synthetic as S
    from oracle.host_emul import HostEmul
    bg = sc.bg if bg is None else bg
    (img, radii, dep, opa, nt), L, th, rh, m2d = _run_gpu(sc, gpu_settings(sc.cam, bg, _dev()), m, s, r, o, sh)
    em = HostEmul()
    eimg, eradii, edep, eopa, ent = em.forward(oracle_settings(sc.cam, bg), m, sh, None, o, s, r, None,
                                               exact_cull=False)
    assert (img.cpu() - eimg).abs().mean().item() <= FWD_L1
    assert (dep.cpu() - edep).abs().mean().item() <= 5e-4
    assert (radii.cpu() != eradii).float().mean().item() <= 1e-3
    assert (nt.cpu() != ent).float().mean().item() <= 5e-3
    gi = img.detach().cpu().requires_grad_()
    gd = dep.detach().cpu().requires_grad_()
    S.synthetic_loss(gi, gd, sc).backward()
    out = em.backward(gi.grad, gd.grad)
    assert rel_err(L["m"].grad, out["means3D"]) <= bwd_tol
    assert rel_err(L["sh"].grad, out["colors"]) <= bwd_tol
    assert rel_err(L["o"].grad.reshape(-1), out["opacities"]) <= bwd_tol
    assert rel_err(L["s"].grad, out["scales"]) <= bwd_tol
    assert rel_err(L["r"].grad, out["rotations"]) <= bwd_tol
    assert rel_err(torch.cat([rh.grad, th.grad]), out["tau"]) <= 2 * bwd_tol


def test_crowded_tiles_use_the_in_memory_sort_path(built):
    """> 4096 pairs in a tile: k_tile_sort sorts in HBM instead of LDS, many segments/tile."""
    from monogs_amd import rasterizer as R
    from monogs_amd import synthetic as S
    sc = S.make_scene(24000, 32, 32, seed=31)          # 4 tiles, ~6k+ splats each
    m, s, r, o, sh = _inputs(sc)
    o = o * 0.15                                        # keep pixels from saturating early
    _against_emulation(sc, m, s, r, o, sh)
    assert R.last_stats["pairs"] > 4 * 4096


@pytest.mark.parametrize("N", [3, 7, 20, 45, 90, 180, 350, 700, 1200, 2400])
def test_register_sort_merge_sizes(built, N):
    """One 16 x 16 tile holding ~0.7 N splats: every merge size of k_tile_sort_reg (4 ... 1024 keys: in-thread
    compare-exchanges, DPP lane distances 1 / 2 / 3 / 4 / 7 / 8 / 15, ds_bpermute 16 / 31 / 32 / 63, LDS across
    waves) and, at 2400, the in-place HBM network.  The blend is order-sensitive, the emulation sorts with
    std::sort; low opacity keeps every splat of the list contributing."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(N, 16, 16, seed=300 + N)
    m, s, r, o, sh = _inputs(sc)
    from monogs_amd import rasterizer as R
    _against_emulation(sc, m, s, r, o * (0.6 if N < 50 else 0.02), sh)
    if N == 2400:
        assert R.last_stats["pairs"] > 1024          # the HBM network of the first launch
    if N == 1200:
        assert 512 < R.last_stats["pairs"] <= 1024   # the full 1024-key register network


def test_screen_filling_splats_use_the_wave_cooperative_binning(built):
    from monogs_amd import synthetic as S
    sc = S.make_scene(1500, 160, 120, seed=32)
    m, s, r, o, sh = _inputs(sc)
    s = s.clone()
    s[::3] *= 25.0                                      # every third splat covers dozens of tiles
    o = o * 0.3
    _against_emulation(sc, m, s, r, o, sh)


def test_more_tiles_than_the_lds_table_falls_back_to_global_atomics(built):
    from monogs_amd import synthetic as S
    W, H = 2048, 1600                                   # 128 x 100 = 12800 tiles > 12288
    sc = S.make_scene(20000, W, H, seed=33)
    m, s, r, o, sh = _inputs(sc)
    s = s * 4.0
    _against_emulation(sc, m, s, r, o, sh)


def test_unpacked_keys_with_the_lds_binning(built):
    """4096 < T <= 12288 tiles: the LDS-privatised binning with UNPACKED sort keys (the pair index
    travels in the payload array beside the key: kPackBits only covers T <= 4096) - 1600 x 1088 =
    100 x 68 = 6800 tiles."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(20000, 1600, 1088, seed=36)
    m, s, r, o, sh = _inputs(sc)
    _against_emulation(sc, m, s * 3.0, r, o, sh)


def test_replica_sized_image_and_background(built):
    """BASELINE config 5 image size (1200 x 680: 75 x 43 tiles, 680 is not a multiple of 16)."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(60000, 1200, 680, seed=34)
    m, s, r, o, sh = _inputs(sc)
    _against_emulation(sc, m, s * 1.5, r, o, sh, bg=torch.tensor([1.0, 1.0, 1.0]))


def test_degenerate_inputs_do_not_fault(built):
    """Zero opacity, huge and tiny scales, points exactly on the near plane, duplicated
    Gaussians (densify_and_clone makes exact copies, gaussian_model.py:525-560)."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(512, 96, 64, seed=35)
    m, s, r, o, sh = _inputs(sc)
    m, s, o = m.clone(), s.clone(), o.clone()
    o[:32] = 0.0
    s[32:64] = 1e-9
    s[64:96] = 50.0
    m[96:128, 2] = 0.2
    m[128:256] = m[256:384]
    s[128:256] = s[256:384]
    r = r.clone()
    r[128:256] = r[256:384]
    (img, radii, dep, opa, nt), L, th, rh, m2d = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev()), m, s, r, o, sh)
    for t in (img, dep, opa, L["m"].grad, L["s"].grad, L["r"].grad, L["o"].grad, L["sh"].grad, th.grad, rh.grad):
        assert torch.isfinite(t).all()
    assert (radii[96:128] == 0).all()                   # z <= 0.2 is culled
    assert (L["m"].grad[:32] == 0).all()                # opacity 0 never reaches 1/255


# ---------------------------------------------------------------------------------------
# fused tracking-loop glue
# ---------------------------------------------------------------------------------------
def test_fused_tracking_loss_matches_torch_reference(built):
    """|| Huber(residual) ||_p against autograd of torch.norm(res.flatten(), p) - the reference's expression
    (slam_frontend.py:596-600: p = 2 with Huber, RGN.pnorm without; base_config.yaml:249 ships pnorm 1)."""
    from monogs_amd import losses as Ls
    from monogs_amd.tracking_fused import tracking_loss
    dev = _dev()
    g = torch.Generator().manual_seed(0)

    class VP:
        pass

    # 120x160; 363x365 (odd, past one trip of the scalar kernels' grid) and 76x132 (whole float4s) after it
    cases = [(H, W, *c) for H, W in ((120, 160), (363, 365), (76, 132))
             for c in ((0.01, 0.9, 2.0), (0.0, -1.1, 2.0), (0.0, 0.9, 1.0), (0.0, -1.1, 1.0), (0.0, 1.05, 1.5),
                       (0.01, 0.9, 1.0))]
    for H, W, delta, a0, pn in cases:
        vp = VP()
        vp.original_image = torch.rand(3, H, W, generator=g).to(dev)
        vp.rgb_pixel_mask_mapping = (torch.rand(1, H, W, generator=g) > 0.2).to(dev)
        vp.exposure_a = torch.tensor([a0], device=dev, requires_grad=True)
        vp.exposure_b = torch.tensor([0.03], device=dev, requires_grad=True)
        vp.exposure_eps = 1e-8
        img = torch.rand(3, H, W, generator=g).to(dev).requires_grad_()
        opa = torch.rand(1, H, W, generator=g).to(dev)
        cfg = {"Training": {"monocular": True}}
        res = Ls.get_loss_tracking_per_pixel(cfg, img, None, opa, vp)
        if delta > 0:
            res = Ls.HuberLoss.apply(res, delta)
        ref = torch.norm(res.flatten(), p=pn)
        (2.5 * ref).backward()
        want = (ref.item(), img.grad.clone(), vp.exposure_a.grad.clone(), vp.exposure_b.grad.clone())
        img.grad = None
        vp.exposure_a.grad = None
        vp.exposure_b.grad = None
        got = tracking_loss(img, opa, vp, delta, pn)
        (2.5 * got).backward()
        assert abs(got.item() - want[0]) <= 1e-5 * want[0], (H, W, delta, pn)
        assert rel_err(img.grad, want[1]) < (1e-5 if pn != 1.5 else 1e-4), (H, W, delta, pn)
        assert rel_err(vp.exposure_a.grad, want[2]) < 1e-4 and rel_err(vp.exposure_b.grad, want[3]) < 1e-4


def test_fused_pose_optimizer_matches_adam_plus_update_pose(built):
    from monogs_amd.pose import SE3_exp, update_pose
    from monogs_amd.tracking_fused import FusedPoseOptimizer
    dev = _dev()

    class Cam:
        pass

    def make():
        c = Cam()
        c.T = SE3_exp(torch.tensor([0.1, 0.2, -0.1, 0.05, 0.0, 0.02])).to(dev).contiguous()
        c.cam_rot_delta = torch.nn.Parameter(torch.zeros(3, device=dev))
        c.cam_trans_delta = torch.nn.Parameter(torch.zeros(3, device=dev))
        c.exposure_a = torch.nn.Parameter(torch.tensor([1.0], device=dev))
        c.exposure_b = torch.nn.Parameter(torch.tensor([0.0], device=dev))
        return c

    ca, cb = make(), make()
    opt = torch.optim.Adam([{"params": [ca.cam_rot_delta], "lr": 0.003}, {"params": [ca.cam_trans_delta], "lr": 0.001},
                            {"params": [ca.exposure_a], "lr": 0.02}, {"params": [ca.exposure_b], "lr": 0.02}])
    fused = FusedPoseOptimizer(cb)
    g = torch.Generator().manual_seed(1)
    for it in range(12):
        grads = [torch.randn(3, generator=g) * 10 ** float(torch.randint(-4, 1, (1,), generator=g)),
                 torch.randn(3, generator=g), torch.randn(1, generator=g), torch.randn(1, generator=g) * 1e-3]
        if it == 11:
            grads = [torch.zeros_like(x) for x in grads]
        for c in (ca, cb):
            for p, gr in zip((c.cam_rot_delta, c.cam_trans_delta, c.exposure_a, c.exposure_b), grads):
                p.grad = gr.to(dev).clone()
        opt.step()
        conv_ref = update_pose(ca)
        conv = fused.step()
        assert torch.allclose(ca.T, cb.T, atol=2e-6), it
        assert torch.allclose(ca.exposure_a, cb.exposure_a, atol=1e-6) and torch.allclose(ca.exposure_b, cb.exposure_b, atol=1e-6)
        assert cb.cam_rot_delta.abs().sum() == 0 and cb.cam_trans_delta.abs().sum() == 0
        assert bool(conv.item()) == conv_ref


def test_fused_tracking_iteration_converges_like_the_reference_loop(built):
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, make_pose_optimizer, tracking_step_first_order, tracking_step_first_order_fused
    from monogs_amd.tracking_fused import FusedPoseOptimizer
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    va, vb = view(2, T0), view(3, T0)
    for v in (va, vb):
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    oa, ob = make_pose_optimizer(va), FusedPoseOptimizer(vb)
    for _ in range(15):
        la, _, _ = tracking_step_first_order(va, gauss, oa, bg)
        lb, _, _ = tracking_step_first_order_fused(vb, gauss, ob, bg)
    assert abs(la.item() - lb.item()) <= 1e-3 * abs(la.item())
    assert torch.allclose(va.T, vb.T, atol=1e-4)


@pytest.mark.parametrize("pnorm", [1.0, 2.0, 1.5])
def test_native_tracking_honours_pnorm_without_huber(built, pnorm):
    """use_huber: False -> the reference optimises torch.norm(residual, p=RGN.pnorm) (slam_frontend.py:596-600;
    shipped pnorm 1).  The native iteration (p = 1 / 2 in the forward blend's epilogue, any other p through the
    one-pass loss kernel) against the reference-shaped Python body, whose objective is that torch expression,
    and the fused-glue form: same loss / pose / exposure trajectory; and p = 1 is NOT p = 2."""
    import copy
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import (DEFAULT_CONFIG, Pipe, make_pose_optimizer, tracking_norm, tracking_step_first_order,
                                       tracking_step_first_order_fused)
    from monogs_amd.tracking_fused import FusedPoseOptimizer
    from monogs_amd.tracking_native import NativeTracker
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["Training"]["RGN"].update(use_huber=False, pnorm=pnorm)
    assert tracking_norm(cfg) == (0.0, pnorm) and tracking_norm(DEFAULT_CONFIG) == (0.01, 2.0)
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    va, vb, vc = view(2, T0), view(3, T0), view(4, T0)
    for v in (va, vb, vc):
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    oa, oc = make_pose_optimizer(va, cfg), FusedPoseOptimizer(vc)
    delta, p = tracking_norm(cfg)
    trk = NativeTracker(vb, gauss, bg, huber_delta=delta, pnorm=p)
    for i in range(12):
        la, _, pkg = tracking_step_first_order(va, gauss, oa, bg, config=cfg)
        lc, _, _ = tracking_step_first_order_fused(vc, gauss, oc, bg, config=cfg)
        trk.step()
        if i == 0:      # the Python body's objective IS the torch expression of the reference
            from monogs_amd import losses as Ls
            with torch.no_grad():
                pk = render(view(5, T0), gauss, Pipe, bg)
                v5 = view(5, T0); v5.original_image = target; v5.rgb_pixel_mask_mapping = va.rgb_pixel_mask_mapping
                r = Ls.get_loss_tracking_per_pixel(cfg, pk["render"], pk["depth"], pk["opacity"], v5)
                assert abs(torch.norm(r.flatten(), p=pnorm).item() - la.item()) <= 1e-5 * la.item()
            assert abs(la.item() - trk.loss.item()) <= 1e-4 * abs(la.item())
    assert trk.check_capacity()
    assert abs(la.item() - trk.loss.item()) <= 1e-3 * abs(la.item())
    assert abs(la.item() - lc.item()) <= 1e-3 * abs(la.item())
    for other in (vb, vc):
        assert torch.allclose(va.T, other.T, atol=1e-4)
        assert torch.allclose(va.exposure_a, other.exposure_a, atol=1e-4)
        assert torch.allclose(va.exposure_b, other.exposure_b, atol=1e-4)
    if pnorm == 1.0:    # and it is a different objective from the L2 one: the L2 tracker's loss value differs
        vd = view(6, T0)
        vd.original_image, vd.rgb_pixel_mask_mapping = target, va.rgb_pixel_mask_mapping
        t2 = NativeTracker(vd, gauss, bg, huber_delta=0.0, pnorm=2.0)
        t2.step()
        t1v = view(7, T0)
        t1v.original_image, t1v.rgb_pixel_mask_mapping = target, va.rgb_pixel_mask_mapping
        t1 = NativeTracker(t1v, gauss, bg, huber_delta=0.0, pnorm=1.0)
        t1.step()
        assert t1.loss.item() > 5.0 * t2.loss.item()       # ||r||_1 >> ||r||_2 over ~58 k samples
    with pytest.raises(ValueError):
        NativeTracker(view(8, T0), gauss, bg, pnorm=0.5)


@pytest.mark.parametrize("W,H", [(160, 120), (150, 101)])
def test_native_tracking_matches_python_loop(built, W, H):
    """mgs_tracking_iteration (one C-ABI call per iteration, pose-only backward) follows the
    same pose / exposure / loss trajectory as the reference-shaped Python loop body.  (150x101: the
    pixel count is not a multiple of 4 - the scalar form of the one-pass tracking objective - and the
    image is not a whole number of tiles.)"""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, make_pose_optimizer, tracking_step_first_order
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture(W=W, H=H)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    va, vb = view(2, T0), view(3, T0)
    for v in (va, vb):
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    oa = make_pose_optimizer(va)
    trk = NativeTracker(vb, gauss, bg)
    for _ in range(15):
        la, _, _ = tracking_step_first_order(va, gauss, oa, bg)
        trk.step()
    assert trk.check_capacity()
    assert abs(la.item() - trk.loss.item()) <= 1e-3 * abs(la.item())
    assert torch.allclose(va.T, vb.T, atol=1e-4)
    assert torch.allclose(va.exposure_a, vb.exposure_a, atol=1e-4)
    assert torch.allclose(va.exposure_b, vb.exposure_b, atol=1e-4)
    # the perturbed pose is being recovered and the loop terminates on the device flag
    err0 = (T0 - torch.eye(4)).abs().max().item()
    n = trk.run(max_iters=200, check_every=5)
    assert n <= 200 and (vb.T.cpu() - torch.eye(4)).abs().max().item() < 0.5 * err0
    # pose-only backward through the plain C ABI: per-Gaussian gradients all NULL or all set
    assert trk.pairs() > 0


def test_hip_splat_and_alpha_match_the_reference_viewer_shader(built):
    """End-to-end pin of the HIP path against the reference's own in-tree restatement
    (gau_vert.glsl:60-154 projection + EWA, gau_frag.glsl:20-26 alpha rule; followed line by
    line in oracle/glsl_ewa.py): one Gaussian on a black background, so the rasteriser's
    `opacity` output is the per-pixel alpha; inside the viewer's +-3 sigma quad it must equal
    the fragment shader's value.  fp32 tolerance 1e-4 (the north-star's image tolerance);
    pixels within 1e-3 relative of the 1/255 cut-off may fall on either side."""
    from oracle import glsl_ewa as G
    from monogs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from test_cpu_oracle import _glsl_scene
    dev = _dev()
    st64, T, p_w, scales, q, f, tanx, tany = _glsl_scene(seed=5, n=24)
    st = GaussianRasterizationSettings(st64.image_height, st64.image_width, tanx, tany,
                                       torch.zeros(3, device=dev), 1.0, st64.viewmatrix.float().to(dev),
                                       st64.projmatrix.float().to(dev), st64.projmatrix_raw.float().to(dev),
                                       0, st64.viewmatrix.float().to(dev), False, False)
    ras = GaussianRasterizer(st)
    checked = capped = cut = 0
    for i in range(24):
        for op in (0.9999, 0.3):
            m, s_, q_ = p_w[i:i + 1], scales[i:i + 1] * 6.0, q[i:i + 1]
            with torch.no_grad():
                img, radii, dep, opa, nt = ras(
                    means3D=m.float().to(dev), means2D=torch.zeros(1, 3, device=dev),
                    colors_precomp=torch.ones(1, 3, device=dev),
                    opacities=torch.tensor([[op]], device=dev), scales=s_.float().to(dev),
                    rotations=q_.float().to(dev))
            if int(radii[0]) == 0:
                continue
            opa = opa[0].cpu().numpy()
            cov2d, conic = G.splat(m[0].numpy(), s_[0].numpy(), q_[0].numpy(), T.numpy(), f, tanx, tany)
            hx, hy = G.quad_half_extent(cov2d)
            pc = T.numpy() @ np.append(m[0].numpy(), 1.0)
            cx = f * pc[0] / pc[2] + (st.image_width - 1) * 0.5
            cy = f * pc[1] / pc[2] + (st.image_height - 1) * 0.5
            for py in range(max(0, int(cy - hy)), min(st.image_height, int(cy + hy) + 2)):
                for px in range(max(0, int(cx - hx)), min(st.image_width, int(cx + hx) + 2)):
                    dx, dy = px - cx, py - cy
                    if abs(dx) > hx or abs(dy) > hy:
                        continue
                    power = -0.5 * (conic[0] * dx * dx + conic[2] * dy * dy) + conic[1] * dx * dy
                    raw = op * np.exp(power)
                    if abs(raw * 255.0 - 1.0) < 1e-3 or abs(power) < 1e-6:
                        continue
                    want = G.fragment_alpha(conic, (dx, -dy), op)
                    assert abs(float(opa[py, px]) - want) <= 1e-4, (i, op, px, py, float(opa[py, px]), want)
                    checked += 1
                    capped += want == 0.99
                    cut += want == 0.0
    assert checked > 1000 and capped > 0 and cut > 0


def test_fused_lm_solve_matches_damped_lstsq(built):
    import math
    from monogs_amd.pose import SE3_exp
    from monogs_amd.tracking_fused import lm_solve_step
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    for rows, lam in ((1024, 1e-3), (37, 0.5)):
        SJ = torch.randn(rows, 8, generator=g) * torch.tensor([3.0, 2.0, 1.0, 5.0, 4.0, 6.0, 0.5, 0.2])
        Sf = torch.randn(rows, generator=g)
        A = torch.cat((SJ, torch.eye(8) * math.sqrt(lam)), 0).double()
        b = torch.cat((Sf, torch.zeros(8)), 0).double()
        want = torch.linalg.lstsq(A, -b).solution.float()

        class Cam:
            pass

        c = Cam()
        c.T = SE3_exp(torch.tensor([0.1, 0.2, -0.1, 0.05, 0.0, 0.02])).to(dev).contiguous()
        T0 = c.T.clone().cpu()
        c.exposure_a = torch.tensor([1.0], device=dev)
        c.exposure_b = torch.tensor([0.0], device=dev)
        x = lm_solve_step(SJ.to(dev), Sf.to(dev), lam, c).cpu()
        assert torch.allclose(x, want, rtol=1e-4, atol=1e-6)
        assert torch.allclose(c.T.cpu(), SE3_exp(want[:6]) @ T0, atol=1e-5)
        assert abs(c.exposure_a.item() - (1.0 + want[6].item())) < 1e-5
        assert abs(c.exposure_b.item() - want[7].item()) < 1e-5


def test_wave_reduce_scatter_unit(built, tmp_path):
    """Kernel-level unit test of csrc/wave_reduce.h (permlane32/16 swap + DPP tree)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_wave_reduce")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-w",
                           os.path.join(root, "tests", "hip", "test_wave_reduce.hip"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=60)
    assert out.returncode == 0 and "PASS" in out.stdout, out.stdout


def test_fused_mapping_loss_matches_torch_reference(built):
    from monogs_amd import losses as Ls
    from monogs_amd.tracking_fused import l1_image_depth_loss, mapping_loss
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    H, W = 90, 130

    class VP:
        pass

    for mono, init in ((True, False), (False, False), (True, True)):
        vp = VP()
        vp.original_image = torch.rand(3, H, W, generator=g).to(dev)
        vp.rgb_pixel_mask_mapping = (torch.rand(1, H, W, generator=g) > 0.2).to(dev)
        vp.gt_depth = (torch.rand(1, H, W, generator=g) * 4).to(dev)
        vp.gt_depth[vp.gt_depth < 0.5] = 0.0
        vp.exposure_a = torch.tensor([-0.8], device=dev, requires_grad=True)
        vp.exposure_b = torch.tensor([0.07], device=dev, requires_grad=True)
        vp.exposure_eps = 1e-8
        cfg = {"Training": {"monocular": mono, "alpha": 0.9}}
        img = torch.rand(3, H, W, generator=g).to(dev).requires_grad_()
        dep = (torch.rand(1, H, W, generator=g) * 4).to(dev).requires_grad_()
        ref = Ls.get_loss_mapping(cfg, img, dep, vp, None, initialization=init)
        (3.0 * ref).backward()
        want = [ref.item(), img.grad.clone(), None if dep.grad is None else dep.grad.clone(),
                None if vp.exposure_a.grad is None else vp.exposure_a.grad.clone(),
                None if vp.exposure_b.grad is None else vp.exposure_b.grad.clone()]
        for t in (img, dep, vp.exposure_a, vp.exposure_b):
            t.grad = None
        got = mapping_loss(cfg, img, dep, vp, initialization=init)
        (3.0 * got).backward()
        assert abs(got.item() - want[0]) <= 1e-5 * abs(want[0])
        assert rel_err(img.grad, want[1]) < 1e-5
        if not mono:
            assert rel_err(dep.grad, want[2]) < 1e-5
        if not init:
            assert rel_err(vp.exposure_a.grad, want[3]) < 1e-4 and rel_err(vp.exposure_b.grad, want[4]) < 1e-4
    img = torch.rand(3, H, W, generator=g).to(dev).requires_grad_()
    dep = torch.rand(1, H, W, generator=g).to(dev).requires_grad_()
    gi, gd = torch.rand(3, H, W, generator=g).to(dev), torch.rand(1, H, W, generator=g).to(dev)
    ref = (img - gi).abs().mean() + 0.05 * (dep - gd).abs().mean()
    ref.backward()
    w = (ref.item(), img.grad.clone(), dep.grad.clone())
    img.grad = None
    dep.grad = None
    got = l1_image_depth_loss(img, dep, gi, gd, 0.05)
    got.backward()
    assert abs(got.item() - w[0]) < 1e-5 * w[0] and rel_err(img.grad, w[1]) < 1e-5 and rel_err(dep.grad, w[2]) < 1e-5


def test_inputs_without_grad_mixed_dtypes_and_mark_visible(built):
    """No input requires grad (eval / GUI rendering, eval_utils.py:138): forward only works,
    non-contiguous and fp64 inputs are accepted, markVisible agrees with radii > 0 on the
    near-plane criterion."""
    from monogs_amd import synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    sc = S.make_scene(700, 96, 64, seed=40)
    m, s, r, o, sh = [t.to(dev) for t in _inputs(sc)]
    m[:50, 2] = -1.0
    ras = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))
    with torch.no_grad():
        a = ras(means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=sh, scales=s, rotations=r)
        m_nc = torch.stack([m, m], 1)[:, 0]                       # non-contiguous view
        b = ras(means3D=m_nc.double(), means2D=torch.zeros_like(m), opacities=o.double(), shs=sh.double(),
                scales=s.double(), rotations=r.double())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    vis = ras.markVisible(m)
    assert not vis[:50].any() and ((a[1] > 0) <= vis).all()


def test_keyframe_insertion_on_device(built):
    """back-projection + sub-sampling + knn scale initialisation without
    leaving the GPU; checked through its invariants (reference: gaussian_model.py:131-205)."""
    from monogs_amd import synthetic as S
    from monogs_amd.keyframe_init import create_pcd_from_image_and_depth, monocular_depth_prior
    from monogs_amd.pose import SE3_exp
    from oracle import torch_raster as O
    dev = _dev()
    H, W = 120, 160
    cam0 = S.make_camera(W, H)

    class Cam:
        pass

    cam = Cam()
    cam.fx, cam.fy, cam.cx, cam.cy = cam0.fx, cam0.fy, cam0.cx, cam0.cy
    cam.T = SE3_exp(torch.tensor([0.2, -0.1, 0.3, 0.05, -0.02, 0.04])).to(dev)
    cam.exposure_a, cam.exposure_b, cam.exposure_eps = torch.tensor([1.0], device=dev), torch.tensor([0.0], device=dev), 1e-8
    g = torch.Generator(device=dev).manual_seed(0)
    image = torch.rand(3, H, W, device=dev, generator=g)
    depth = 1.0 + 3.0 * torch.rand(H, W, device=dev, generator=g)
    depth[:10] = 0.0                                            # invalid rows are never used
    xyz, feats, scales, rots, opac = create_pcd_from_image_and_depth(
        cam, image, depth, downsample_factor=8, point_size=0.01, generator=g)
    P = xyz.shape[0]
    assert P == int((depth > 0).sum().item() / 8)
    # every point re-projects onto an integer pixel with the depth it came from
    pc = xyz @ cam.T[:3, :3].t() + cam.T[:3, 3]
    u = pc[:, 0] / pc[:, 2] * cam.fx + cam.cx
    v = pc[:, 1] / pc[:, 2] * cam.fy + cam.cy
    assert (u - u.round()).abs().max() < 1e-2 and (v - v.round()).abs().max() < 1e-2
    ui, vi = u.round().long(), v.round().long()
    assert (vi >= 10).all()
    assert torch.allclose(pc[:, 2], depth[vi, ui], rtol=1e-4)
    # colours are the uint8-quantised image in SH-0 form; scales follow the knn rule
    col = torch.floor(image[:, vi, ui].t() * 255) / 255
    assert torch.allclose(feats[:, :, 0], (col - 0.5) / 0.28209479177387814, atol=1e-5)
    ps = min(0.05, 0.01 * float(torch.median(depth)))
    want = torch.log(torch.sqrt(torch.clamp_min(O.dist2_knn3(xyz.cpu()), 1e-7) * ps))
    assert torch.allclose(scales[:, 0].cpu(), want, atol=1e-4)
    assert (rots[:, 0] == 1).all() and (rots[:, 1:] == 0).all() and torch.allclose(torch.sigmoid(opac), torch.full_like(opac, 0.5))
    d = monocular_depth_prior(H, W, 2.0, dev, g)
    assert abs(d.mean().item() - 2.0 * (1 - 0.025)) < 0.01


# ---------------------------------------------------------------------------------------
# map maintenance on the device
# ---------------------------------------------------------------------------------------
def test_fused_gaussian_adam_matches_torch_adam(built):
    dev = _dev()
    ma, cpu, attr = _make_model(3001, dev, 7, fused=True, rest=3)
    mb, _, _ = _make_model(3001, dev, 7, fused=False, rest=3)
    g = torch.Generator().manual_seed(1)
    for it in range(6):
        for name, a in attr.items():
            grad = torch.randn(getattr(ma, a).shape, generator=g) * (10.0 ** -(it % 3))
            getattr(ma, a).grad = grad.clone().to(dev)
            getattr(mb, a).grad = grad.clone().to(dev)
        if it == 3:      # update_learning_rate (gaussian_model.py:287-300) edits the group in place
            for opt in (ma.optimizer, mb.optimizer):
                opt.param_groups[0]["lr"] = 3.3e-5
        if it == 4:      # a group without a gradient is skipped
            ma._features_rest.grad = None
            mb._features_rest.grad = None
        ma.optimizer.step()
        mb.optimizer.step()
    for name, a in attr.items():
        pa, pb = getattr(ma, a), getattr(mb, a)
        assert torch.allclose(pa, pb, rtol=2e-6, atol=1e-7), name
        sa, sb = ma.optimizer.state[pa], mb.optimizer.state[pb]
        assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-7), name   # lerp rounding
        assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-10), name


@pytest.mark.parametrize("fused,max_screen_size,rest", [(True, 20, 0), (False, None, 3)])
def test_densify_and_prune_matches_the_reference_restatement(built, fused, max_screen_size, rest):
    """monogs_amd.map_update.densify_and_prune (plan + one gather launch) against the PyTorch
    restatement of gaussian_model.py:598-691: same rows in the same order, parameters, Adam
    moments, keyframe ids, observation counts and zeroed statistics."""
    from monogs_amd import map_update as MU
    from oracle import map_update_ref as REF
    dev = _dev()
    n = 5000
    m, cpu, attr = _make_model(n, dev, 11, fused=fused, rest=rest)
    g = torch.Generator().manual_seed(2)
    for a in attr.values():      # two optimiser steps so that the Adam moments are populated
        getattr(m, a).grad = torch.randn(getattr(m, a).shape, generator=g).to(dev) * 1e-2
    m.optimizer.step()
    m.optimizer.step()
    before = _state_of(m, attr, cpu)
    extent, max_grad, min_opacity = 6.0, 2e-4, 0.1
    scale = torch.exp(before["scaling"])
    grads = before["grad_accum"] / before["denom"]
    grads[grads.isnan()] = 0
    n_split = int(((grads.squeeze(-1) >= max_grad) & (scale.max(1).values > m.percent_dense * extent)).sum())
    assert n_split > 20
    noise = torch.randn(2 * n_split, 3, generator=g)
    want = REF.densify_and_prune({k: v.clone() for k, v in before.items()}, max_grad, min_opacity, extent,
                                 max_screen_size, m.percent_dense, noise)
    MU.densify_and_prune(m, max_grad, min_opacity, extent, max_screen_size, noise=noise.to(dev))
    got = _state_of(m, attr, cpu)
    assert got["xyz"].shape[0] == want["xyz"].shape[0] and got["xyz"].shape[0] != n
    for k, w in want.items():
        gk = got[k]
        assert gk.shape == w.shape, (k, gk.shape, w.shape)
        if w.dtype.is_floating_point:
            assert torch.allclose(gk, w, rtol=1e-5, atol=1e-6), k
        else:
            assert torch.equal(gk, w.to(gk.dtype)), k
    # the rebuilt parameters are leaves registered in the optimiser
    for grp in m.optimizer.param_groups:
        assert grp["params"][0] is getattr(m, attr[grp["name"]]) and grp["params"][0].requires_grad

    # prune_points(mask) alone (slam_backend.py:86,280)
    mask = torch.rand(got["xyz"].shape[0], generator=g) < 0.3
    want2 = REF.prune_points(got, mask)
    MU.prune_points(m, mask.to(dev))
    got2 = _state_of(m, attr, cpu)
    for k, w in want2.items():
        assert got2[k].shape == w.shape and torch.equal(got2[k], w.to(got2[k].dtype)), k


def test_gradient_bucket_pack_kernel_matches_torch(built):
    """FlatGradBucket.pack on the GPU (one HIP launch) against the PyTorch formulation of
    gaussian_model.py:693-697 + torch.cat."""
    from monogs_amd.parallel import FlatGradBucket
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    N = 4099
    shapes = [(N, 3), (N, 1, 3), (N, 1), (N, 3), (N, 4)]
    params = [torch.zeros(s, device=dev) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    m2d = torch.randn(N, 3, generator=g).to(dev)
    radii = torch.randint(-1, 4, (N,), generator=g).int().to(dev)
    b = FlatGradBucket(params)
    want = torch.cat([p.grad.reshape(-1) for p in params]
                     + [torch.where(radii > 0, torch.linalg.norm(m2d[:, :2], dim=-1), torch.zeros(N, device=dev)),
                        (radii > 0).float()])
    stat, denom, rad = b.all_reduce(m2d, radii)          # single process: pack + unpack
    assert torch.allclose(b.flat, want, rtol=1e-6, atol=0)
    assert torch.equal(rad, radii) and torch.equal(denom, (radii > 0).float())
    assert params[4].grad.data_ptr() == b.flat[sum(p.numel() for p in params[:4]):].data_ptr()


def test_sketched_lm_solve_meets_the_reference_bounds(built):
    """The reference's one test of its second-order path (tests/test_sketching.py:6-20 +
    tests/sketch_utils.py:58-124): CountSketch an m x 8 damped least-squares problem, solve the small
    system, assert ||x_opt - x_sketch|| below two bounds.  Here the sketch is the PRODUCT's: the keyed
    partition + the +-1 weights of mgs_sketch_assign (what replaces torch.randperm / rand_weights,
    slam_frontend.py:269-338), S A and S b formed on the device in fp32, solved by mgs_lm_solve_step
    (append-damp, lambda = 1e4).  The problems are the reference generator's (tests/golden/sketch_bound.npz
    pins the restated generator; m = 160*120 and 640*480; stack 16 / sketch 64 = the shipped tracker
    configuration base_config.yaml:258-260, and 1 / 32 = test_sketching.py:15-17).

    The second bound (sketch_utils.py:124) must hold for every key.  The first (:123) is a heuristic -
    its distortion looks at the two extreme singular values only - that the reference's OWN sketch meets in
    26 of 30 draws on the small problem (fixture: small_ref30_*; 25 of 30 whole run_test calls here): the
    product's sketch is held to the same statistics over 12 keys per configuration (>= 8 of 12, P < 1 % for
    a sketch as good as the reference's), and its median error to the reference's median."""
    import ctypes as C
    import os
    from scipy.linalg import lstsq
    from monogs_amd import _cabi
    from monogs_amd.tracking_fused import lm_solve_step
    from oracle import sketch_problem as SP
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sketch_bound.npz"))
    ref_diff, ref_ub = G["small_ref30_x_diff"], G["small_ref30_bound"]
    assert int((ref_diff < ref_ub).sum()) == 26 and bool((ref_diff < G["small_ref30_bound_hat"]).all())
    dev = _dev()
    lib = _cabi.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lam = SP.REFERENCE_TEST["lambda_"]
    for tag, configs in (("small", ((1, 32), (4, 8), (16, 64))), ("large", ((1, 32), (16, 64)))):
        m, seed = int(G[f"{tag}_m"]), int(G[f"{tag}_seed"])
        A, b, _ = SP.gen_problem(m, seed=seed, **SP.REFERENCE_TEST)
        assert np.allclose(A.T @ A, G[f"{tag}_AtA"], rtol=1e-8, atol=1e-11)      # the reference generator's problem
        Ad, bd = torch.from_numpy(A).float().to(dev), torch.from_numpy(b).float().to(dev)
        for stack, sketch in configs:
            d = stack * sketch
            diffs, first = [], 0
            for key in range(1, 13):
                bucket = torch.empty(m, dtype=torch.int32, device=dev)
                w = torch.empty(m, device=dev)
                _cabi.check(lib.mgs_sketch_assign(m, stack, sketch, C.c_uint64(key * 7919 + d), bucket.data_ptr(),
                                                  w.data_ptr(), stream), "assign")
                keep = bucket >= 0
                idx = bucket[keep].long()
                SA = torch.zeros(d, 8, device=dev).index_add_(0, idx, Ad[keep] * w[keep, None])
                Sb = torch.zeros(d, device=dev).index_add_(0, idx, bd[keep] * w[keep])
                # the solver minimises ||SJ x + Sf||: Sf = -S b
                x_sketch = lm_solve_step(SA, -Sb, lam).double().cpu().numpy()
                SAh, Sbh = SA.double().cpu().numpy(), Sb.double().cpu().numpy()
                x_opt, ub, ub_hat, st = SP.bounds(A, b, lam, SAh, Sbh, x_sketch, d)
                assert np.allclose(x_opt, G[f"{tag}_x_opt"], rtol=1e-7, atol=1e-13)
                diff = float(np.linalg.norm(x_opt - x_sketch))
                assert diff < ub_hat, (tag, stack, sketch, key, diff, ub_hat, st)       # sketch_utils.py:124
                first += diff < ub                                                      # sketch_utils.py:123
                diffs.append(diff)
                # the device solve IS the damped lstsq of the sketched system (fp64 on the host)
                At, bt = SP.damped(SAh, Sbh, lam)
                assert np.allclose(x_sketch, lstsq(At, bt)[0], rtol=1e-4, atol=1e-9)
            print(f"sketch bound {tag} stack {stack} sketch {sketch}: first bound met by {first} of 12 keys, median error {np.median(diffs):.3e}")
            assert first >= 8, (tag, stack, sketch, first, diffs)
            if tag == "small" and d == 32:       # same problem, same sketch size as the reference's 30 draws
                assert np.median(diffs) < 1.5 * np.median(ref_diff), (np.median(diffs), np.median(ref_diff))


def test_sketch_assign_is_a_random_partition_into_equal_buckets(built):
    """mgs_sketch_assign: every bucket gets exactly chunk = HW // (stack*sketch) pixels (the
    structure of slam_frontend.py:269-338), leftovers are -1, weights are +-1 and roughly
    balanced, and a different key gives a different partition."""
    import ctypes as C
    from monogs_amd import _cabi
    dev = _dev()
    lib = _cabi.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for (HW, stack, sketch) in ((640 * 480, 16, 64), (160 * 120 + 7, 4, 8), (33, 2, 3)):
        d, chunk = stack * sketch, HW // (stack * sketch)
        prev = None
        for key in (1, 2):
            bucket = torch.empty(HW, dtype=torch.int32, device=dev)
            w = torch.empty(HW, device=dev)
            _cabi.check(lib.mgs_sketch_assign(HW, stack, sketch, key, bucket.data_ptr(), w.data_ptr(), stream), "assign")
            b = bucket.cpu().long()
            assert int((b < 0).sum()) == HW - chunk * d and b.max() < d
            counts = torch.bincount(b[b >= 0], minlength=d)
            assert bool((counts == chunk).all())
            assert bool((w.abs() == 1).all())
            if HW > 1000:
                assert abs(w.mean().item()) < 0.05
                # pixels of a bucket are spread over the image, not contiguous runs
                px = torch.nonzero(b == 0).squeeze(1).float()
                assert px.std().item() > 0.15 * HW
            if prev is not None and HW > 1000:
                assert (prev != b).float().mean().item() > 0.9
            prev = b


@pytest.mark.parametrize("W,H,gain", [(160, 120, 0.97), (150, 101, 0.97), (160, 120, -0.97)])
def test_native_second_order_iteration_matches_python_formulation(built, W, H, gain):
    """mgs_tracking_iteration_second_order against tracking_step_second_order (the reference-
    shaped autograd formulation) on the SAME bucket partition and weights: Sf, the sketched
    Jacobian SJ [d, 8], the LM step and the updated pose / exposure.  (150x101: not a whole number of tiles, and
    46 pixels left over by the 64 buckets.)  gain < 0: exposure_a negative, where the reference's hand-written
    ApplyExposure.backward (slam_utils.py:145-149: no sign(a)) and the exact derivative part ways - the Python
    formulation differentiates through losses.ApplyExposure, which tests/test_cpu_map_update_golden.py pins to the
    reference's own outputs, and the native iteration must take the same (reference) step."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, sketch_args_from_buckets, tracking_step_second_order
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture(W=W, H=H)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    va, vb = view(2, T0), view(3, T0)
    for v in (va, vb):
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
        with torch.no_grad():
            v.exposure_a.fill_(gain)
            v.exposure_b.fill_(0.01)
    H, W = va.image_height, va.image_width
    stack, sketch, lam = 4, 16, 1e-3
    trk = NativeTracker(vb, gauss, bg)
    trk.enable_second_order(stack_dim=stack, sketch_dim=sketch, initial_lambda=lam, seed=5, keep_sketch=True)
    # the default form (accumulators cleared by their consumers, no memset launches) takes the same step
    vc = view(4, T0)
    vc.original_image, vc.rgb_pixel_mask_mapping = target, vb.rgb_pixel_mask_mapping
    with torch.no_grad():
        vc.exposure_a.fill_(gain)
        vc.exposure_b.fill_(0.01)
    trk_fast = NativeTracker(vc, gauss, bg)
    trk_fast.enable_second_order(stack_dim=stack, sketch_dim=sketch, initial_lambda=lam, seed=5)
    for _ in range(3):
        trk_fast.step_second_order()
    state = trk.step_second_order()
    torch.cuda.synchronize()
    Sf_n, SJ_n = trk.sketch
    fsa = sketch_args_from_buckets(trk.so_bucket, trk.so_weights, H, W, stack, sketch)
    l1, x, SJ, Sf = tracking_step_second_order(va, gauss, bg, lambda_=lam, repeat_dim=1, stack_dim=stack,
                                               sketch_dim=sketch, fused_solve=True, fsa=fsa)
    assert rel_err(Sf_n, Sf) < 1e-4
    assert rel_err(SJ_n[:, 6:], SJ[:, 6:]) < 1e-4            # exposure columns
    assert rel_err(SJ_n[:, :6], SJ[:, :6]) < 2e-3            # pose columns (through the rasteriser)
    assert rel_err(trk.so_x, x) < 5e-3
    assert torch.allclose(va.T, vb.T, atol=1e-4)
    assert torch.allclose(va.exposure_a, vb.exposure_a, atol=1e-4)
    if gain < 0:      # the step on `a` has the sign the reference's Jacobian gives it, not the exact derivative's
        assert rel_err(SJ_n[:, 6], SJ[:, 6]) < 1e-4 and float((SJ_n[:, 6] * SJ[:, 6]).sum()) > 0
        return
    st = state.cpu()
    assert abs(st[0].item() - lam) < 1e-9 and st[2].item() == 1.0
    # trust-region rule on the device: the loss decreased after a good step -> lambda / 5
    before = st[1].item()
    st2 = trk.step_second_order().cpu()
    assert st2[1].item() < before and abs(st2[0].item() - lam / 5.0) < 1e-9
    # the pose keeps improving over a few iterations
    for _ in range(6):
        trk.step_second_order()
    assert trk.check_capacity()
    # three iterations of the memset-free form = the first three of the other one (same partitions; the
    # bucket sums are float atomics, so not bit for bit)
    vd = view(5, T0)
    vd.original_image, vd.rgb_pixel_mask_mapping = target, vb.rgb_pixel_mask_mapping
    with torch.no_grad():
        vd.exposure_a.fill_(gain)
        vd.exposure_b.fill_(0.01)
    trk_ref = NativeTracker(vd, gauss, bg)
    trk_ref.enable_second_order(stack_dim=stack, sketch_dim=sketch, initial_lambda=lam, seed=5, keep_sketch=True)
    for _ in range(3):
        trk_ref.step_second_order()
    assert torch.allclose(vc.T, vd.T, atol=1e-5) and torch.allclose(vc.exposure_a, vd.exposure_a, atol=1e-5)
    assert torch.allclose(trk_fast.lm_state, trk_ref.lm_state, rtol=1e-3, atol=1e-6)
    assert float(trk_fast.so_accum.abs().max()) == 0.0           # left zero for the next iteration
    assert (vb.T.cpu() - torch.eye(4)).abs().max().item() < 0.5 * (T0 - torch.eye(4)).abs().max().item()


def test_native_second_order_repeat_dim_matches_python_formulation(built):
    """RGN.second_order.repeat_dim > 1 (base_config.yaml:258; slam_frontend.py:654-669: `repeat_dim` sketched
    backward passes over ONE render, each with its own partition and weights, rows of Sf / SJ stacked) through
    mgs_tracking_iteration_second_order, against the reference-shaped autograd formulation (which calls the
    rasteriser's backward repeat_dim times with retain_graph) on the SAME partitions."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe, sketch_args_from_buckets, tracking_step_second_order
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    T0 = SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    H, W = 120, 160
    stack, sketch, lam, R = 4, 16, 1e-3, 3

    def cam(uid):
        v = view(uid, T0)
        v.original_image = target
        v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
        with torch.no_grad():
            v.exposure_a.fill_(0.97)
            v.exposure_b.fill_(0.01)
        return v

    va, vb, vc = cam(2), cam(3), cam(4)
    trk = NativeTracker(vb, gauss, bg)
    trk.enable_second_order(stack_dim=stack, sketch_dim=sketch, initial_lambda=lam, seed=9, keep_sketch=True, repeat_dim=R)
    trk.step_second_order()
    torch.cuda.synchronize()
    Sf_n, SJ_n = trk.sketch
    assert Sf_n.shape == (R * stack * sketch,) and SJ_n.shape == (R * stack * sketch, 8)
    b = trk.so_bucket.cpu()
    assert b.shape == (R, H * W) and not torch.equal(b[0], b[1]) and not torch.equal(b[1], b[2])   # a partition per repeat
    fsa = sketch_args_from_buckets(trk.so_bucket, trk.so_weights, H, W, stack, sketch)
    assert fsa["repeat_dim"] == R
    l1, x, SJ, Sf = tracking_step_second_order(va, gauss, bg, lambda_=lam, repeat_dim=R, stack_dim=stack,
                                               sketch_dim=sketch, fused_solve=True, fsa=fsa)
    assert SJ.shape == (R * stack * sketch, 8)
    assert rel_err(Sf_n, Sf) < 1e-4
    assert rel_err(SJ_n[:, 6:], SJ[:, 6:]) < 1e-4
    assert rel_err(SJ_n[:, :6], SJ[:, :6]) < 2e-3
    assert abs(float(trk.lm_state[1]) - float(l1)) < 1e-4 * float(l1)        # the L1 criterion is counted once
    assert rel_err(trk.so_x, x) < 5e-3
    assert torch.allclose(va.T, vb.T, atol=1e-4) and torch.allclose(va.exposure_a, vb.exposure_a, atol=1e-4)
    # the memset-free form: same steps, accumulators left zero
    fast = NativeTracker(vc, gauss, bg)
    fast.enable_second_order(stack_dim=stack, sketch_dim=sketch, initial_lambda=lam, seed=9, repeat_dim=R)
    fast.step_second_order()
    assert torch.allclose(vc.T, vb.T, atol=1e-5)
    assert float(fast.so_accum.abs().max()) == 0.0


def test_failed_second_order_call_leaves_the_kept_zero_scratch_clean(built):
    """scratch_kept_zero: the accumulators are restored to zero by the LAST kernels of the sequence.  A call that
    fails in between (here: a sketch whose bucket table does not fit the bucket kernel's shared memory ->
    MGS_ERR_UNSUPPORTED from the backward, AFTER the residual pass has accumulated Sf / l1) must clear them
    itself, or the next call would silently accumulate on top."""
    import ctypes as C
    from monogs_amd import _cabi
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    v = view(2, SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003])))
    v.original_image = target
    v.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    trk = NativeTracker(v, gauss, bg)
    trk.enable_second_order(stack_dim=48, sketch_dim=64, initial_lambda=1e-3, seed=1)     # 3072 buckets x 6 x 4 B > 64 KB
    T_before = v.T.clone()
    with pytest.raises(RuntimeError):
        trk.step_second_order()
    torch.cuda.synchronize()
    assert float(trk.so_accum.abs().max()) == 0.0
    assert torch.equal(v.T, T_before)
    # ... and the tracker is still usable: a supported sketch on the same scratch takes the same step as a fresh one
    trk.enable_second_order(stack_dim=4, sketch_dim=16, initial_lambda=1e-3, seed=1)
    trk.step_second_order()
    v2 = view(3, SE3_exp(torch.tensor([0.02, -0.015, 0.01, 0.004, -0.006, 0.003])))
    v2.original_image, v2.rgb_pixel_mask_mapping = target, v.rgb_pixel_mask_mapping
    t2 = NativeTracker(v2, gauss, bg)
    t2.enable_second_order(stack_dim=4, sketch_dim=16, initial_lambda=1e-3, seed=1)
    t2.step_second_order()
    assert torch.allclose(v.T, v2.T, atol=1e-5)


def test_native_tracker_grows_an_undersized_pair_capacity(built):
    """All kernels clamp to the pair capacity (no out-of-bounds access when D > capacity); the
    tracker notices lazily, grows its workspaces and then renders completely."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe
    from monogs_amd.tracking_native import NativeTracker
    sc, gauss, view, dev = _loop_fixture()
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clone()
    vp = view(2, SE3_exp(torch.tensor([0.01, -0.01, 0.005, 0.002, -0.003, 0.001])))
    vp.original_image = target
    vp.rgb_pixel_mask_mapping = (target.sum(0) > 0.01).view(1, *target.shape[1:])
    trk = NativeTracker(vp, gauss, bg, capacity_margin=0.4)       # 40 % of the pairs fit
    D0 = trk.pairs()
    assert trk.capacity < D0
    trk.step()
    torch.cuda.synchronize()
    assert torch.isfinite(vp.T).all()
    trk.capacity_margin = 1.5
    assert not trk.check_capacity()              # overflow detected, workspaces regrown to 1.5 * D
    assert trk.capacity >= trk.pairs()
    trk.step()
    torch.cuda.synchronize()
    assert trk.check_capacity()
    with torch.no_grad():
        full = render(vp, gauss, Pipe, bg)["render"]
    # the tracker's last forward rendered the pose BEFORE its final update; render it again natively
    trk.step()
    torch.cuda.synchronize()
    assert torch.isfinite(trk.color).all() and (trk.color - full).abs().mean().item() < 0.05


def test_hip_matches_the_committed_syn_a_vectors(built):
    """The HIP path against the committed fixture tests/golden/syn_a_oracle.npz (BASELINE config
    1 shape; oracle outputs frozen by tests/golden/make_syn_golden.py): forward image L1 <= 1e-4,
    gradients <= 1e-3 relative, integer outputs equal up to the few splats whose ceil() flips."""
    import os
    from monogs_amd import synthetic as S
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "syn_a_oracle.npz"))
    sc = S.make_scene(5000, 160, 120, seed=0)
    inp = _inputs(sc)
    (img, radii, dep, opa, nt), L, th, rh, m2d = _run_gpu(sc, gpu_settings(sc.cam, sc.bg, _dev()), *inp)
    t = lambda k: torch.from_numpy(want[k])
    assert (img.cpu() - t("image")).abs().mean().item() <= FWD_L1
    assert (dep.cpu() - t("depth")).abs().mean().item() <= 1e-3
    assert (opa.cpu() - t("opacity")).abs().mean().item() <= FWD_L1
    assert (radii.cpu() != t("radii")).sum().item() <= 5
    assert (nt.cpu() - t("n_touched")).abs().sum().item() <= 0.002 * t("n_touched").sum().item() + 5
    for key, g in (("grad_means3D", L["m"].grad), ("grad_scales", L["s"].grad), ("grad_rot", L["r"].grad),
                   ("grad_opacity", L["o"].grad), ("grad_sh", L["sh"].grad)):
        assert rel_err(g, t(key)) <= BWD_REL, key
    assert rel_err(torch.cat([rh.grad, th.grad]), t("grad_tau")) <= 2e-3


def test_tile_scan_handoff_never_reads_stale_counts(built):
    """k_bin_colsum hands the tile totals to the tile scan inside the same launch (last workgroup,
    fence-free sc1 store / load).  A reordering would show as a scan over stale totals: the pair
    count D and tile_offset would disagree with the per-Gaussian pair counts the count pass wrote
    independently.  Many-workgroup shape (1200x680: 3225 tiles = 51 column workgroups), two scenes
    alternating so that a stale value is a WRONG value, 40 forwards; the last one is also compared
    tile by tile with the host emulation's exact-culling counts."""
    from monogs_amd import _cabi, rasterizer as R, synthetic as S
    from monogs_amd.rasterizer import GaussianRasterizer
    from oracle.host_emul import HostEmul
    dev = _dev()
    W, H = 1200, 680
    scenes_ = [S.make_scene(40000, W, H, seed=50), S.make_scene(52000, W, H, seed=51)]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    last = None
    for it in range(40):
        sc = scenes_[it % 2]
        m, s, r, o, sh = [t.to(dev) for t in _inputs(sc)]
        N = m.shape[0]
        m.requires_grad_()
        img, radii, dep, opa, nt = GaussianRasterizer(gpu_settings(sc.cam, sc.bg, dev))(
            means3D=m, means2D=torch.zeros(N, 3, device=dev), shs=sh, opacities=o, scales=s, rotations=r)
        geom = img.grad_fn.saved_tensors[12]
        cap = R.last_stats["capacity"]
        sz = _cabi.workspace_sizes(_cabi.RasterShape(N, W, H, 0, 1, cap, sc.cam.tanfovx, sc.cam.tanfovy, 1.0))
        pc = geom[int(sz.off_pair_count):int(sz.off_pair_count) + 4 * N].view(torch.int32)
        toff = geom[int(sz.off_tile_offset):int(sz.off_tile_offset) + 4 * (T + 1)].view(torch.int32)
        cnt = geom[int(sz.off_counters):int(sz.off_counters) + 16].view(torch.int32)
        D = int(pc.sum())
        assert int(cnt[0]) == D == int(toff[T]) == R.last_stats["pairs"], (it, int(cnt[0]), D, int(toff[T]))
        assert int(toff[0]) == 0 and bool((toff[1:] >= toff[:-1]).all())
        last = (sc, toff.cpu().clone(), _inputs(sc))
    sc, toff, (m, s, r, o, sh) = last
    em = HostEmul()
    em.forward(oracle_settings(sc.cam, sc.bg), m, sh, None, o, s, r, None, exact_cull=True)
    import ctypes as C
    from oracle import host_emul as HE
    if hasattr(HE.lib(), "emul_tile_offsets"):
        want = torch.empty(T + 1, dtype=torch.int32)
        HE.lib().emul_tile_offsets(em.h, C.cast(want.data_ptr(), C.POINTER(C.c_int32)), C.c_int(T + 1))
        # the kernels' culling is conservative by a rounding slack: a handful of borderline pairs may differ
        assert (toff - want).abs().max().item() <= max(4, em.pairs // 2000)
    assert abs(int(toff[T]) - em.pairs) <= max(2, em.pairs // 1000)


@pytest.mark.parametrize("H,W", [(75, 133), (76, 132), (1024, 516)])
def test_fused_loss_backward_helper_matches_autograd(built, H, W):
    """l1_image_depth_loss_backward: value + gradients in one launch, handed to autograd - equal to
    loss.backward() of the torch formulation incl. the exposure path and the masks.  75x133 pixels are
    not a multiple of 4 (scalar form of k_map_loss), 76x132 are (four pixels per thread), 1024x516 need a second
    trip of the four-pixel form."""
    from monogs_amd.tracking_fused import l1_image_depth_loss_backward
    dev = _dev()
    g = torch.Generator().manual_seed(5)

    class VP:
        pass
    for use_vp in (False, True):
        vp = None
        if use_vp:
            vp = VP()
            vp.exposure_a = torch.tensor([-0.9], device=dev, requires_grad=True)
            vp.exposure_b = torch.tensor([0.05], device=dev, requires_grad=True)
            vp.exposure_eps = 1e-8
        mask = (torch.rand(1, H, W, generator=g) > 0.3).float().to(dev) if use_vp else None
        gi, gd = torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 3).to(dev)
        base_i, base_d = torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 3).to(dev)
        res = {}
        for kind in ("torch", "fused"):
            x = base_i.clone().requires_grad_()
            y = base_d.clone().requires_grad_()
            img, dep = x * 1.5 + 0.1, y * 0.7          # a graph in front, as the rasteriser would be
            if vp is not None:
                vp.exposure_a.grad = None
                vp.exposure_b.grad = None
            if kind == "torch":
                im = img if vp is None else (torch.abs(vp.exposure_a) + vp.exposure_eps) * img + vp.exposure_b
                m = 1.0 if mask is None else mask
                dm = (gd > 0.5).float() if use_vp else 1.0
                loss = 0.8 * torch.abs(m * (im - gi)).mean() + 0.3 * torch.abs(dm * (dep - gd)).mean()
                loss.backward()
            else:
                loss = l1_image_depth_loss_backward(img, dep, gi, gd, 0.3, mask=mask, viewpoint=vp, w_rgb=0.8,
                                                    depth_mask_threshold=0.5 if use_vp else -1.0)
            res[kind] = (float(loss), x.grad.clone(), y.grad.clone(),
                         None if vp is None else (vp.exposure_a.grad.clone(), vp.exposure_b.grad.clone()))
        a, b = res["torch"], res["fused"]
        assert abs(a[0] - b[0]) < 1e-5 * abs(a[0])
        assert rel_err(b[1], a[1]) < 1e-5 and rel_err(b[2], a[2]) < 1e-5
        if use_vp:
            assert rel_err(b[3][0], a[3][0]) < 1e-4 and rel_err(b[3][1], a[3][1]) < 1e-4
