"""The HIP rasteriser held to the fp64 oracle pixel by pixel and Gaussian row by row, with the oracle's own flip
allowance (tests/raster_parity.py; DESIGN.md section 2, "How parity is held").  The scenes are small - the largest are
1468 splats at 150x101 and 4200 splats in one 16x16 tile - and the three fp64 oracle runs of a scene dominate a test's
time."""
import pytest
import torch

import raster_parity as P
from conftest import gpu_settings

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _run(c):
    """One forward + backward of GaussianRasterizer on a case, in the layout of raster_parity.run_oracle."""
    from monogs_amd.rasterizer import GaussianRasterizer
    dev = _dev()
    req = lambda t: None if t is None else t.clone().to(dev).requires_grad_()
    L = {k: req(getattr(c, k)) for k in ("m", "s", "r", "o", "sh", "col", "cov")}
    N = c.m.shape[0]
    m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
    theta = rho = None
    if c.pose:
        theta = torch.zeros(3, device=dev, requires_grad=True)
        rho = torch.zeros(3, device=dev, requires_grad=True)
    st = gpu_settings(c.cam, c.bg, dev, deg=c.deg, campos=c.campos)
    img, radii, dep, opa, nt = GaussianRasterizer(st)(
        means3D=L["m"], means2D=m2d, shs=L["sh"], colors_precomp=L["col"], opacities=L["o"], scales=L["s"],
        rotations=L["r"], cov3D_precomp=L["cov"], theta=theta, rho=rho)
    P.loss_of(c, img, dep).backward()
    torch.cuda.synchronize()
    grads = P.pack_grads(N, L["m"].grad, m2d.grad, L["o"].grad, (L["sh"] if L["sh"] is not None else L["col"]).grad,
                         None if L["s"] is None else L["s"].grad, None if L["r"] is None else L["r"].grad,
                         None if L["cov"] is None else L["cov"].grad)
    tau = torch.cat([rho.grad, theta.grad]).double().cpu() if c.pose else None
    return dict(image=img.detach().cpu(), depth=dep.detach().cpu(), opacity=opa.detach().cpu(), radii=radii.cpu(),
                n_touched=nt.cpu(), grads=grads, tau=tau)


def _identical(a, b):
    for k in ("image", "depth", "opacity", "radii", "n_touched"):
        assert torch.equal(a[k], b[k]), k
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert (a["tau"] is None and b["tau"] is None) or torch.equal(a["tau"], b["tau"])


@pytest.mark.parametrize("name", P.CASE_NAMES + [P.LONG] + P.DECISION_NAMES)
def test_rasteriser_matches_the_fp64_oracle_per_pixel_and_per_row(built, name):
    """The case grazing_long is the scene of long oblique needles (sigma up to 50 px at 30 / 45 / 60 degrees, blended): the
    per-quadrant box test, the polynomial exponent and the backward's reach words on the splats where the cross term
    of the conic matters most.  Its conic cancels in fp32, so it is held to constants measured on that scene alone
    (raster_parity.CONST_LONG) and its cap shares are not asserted; a pair dropped up to 5 % above 1/255 in any whole
    tile of it still fails (tests/test_cpu_raster_parity.py).
    The decision scenes put Gaussians 2 and 16 bands on either side of the near plane, the field-of-view clamp and the
    first tile boundary in play (decisions_70x45, under both treatments of the clamp in the backward), and exact depth
    ties into one tile's list of 40, 1100 and 4200 splats: the register network, the LDS class and the in-HBM class of
    the tile sort, and the reverse walk of the same lists in the backward."""
    from monogs_amd import rasterizer as R
    modes = ("upstream", "exact") if name == "decisions_70x45" else ("upstream",)
    assert R._clamp_gradient_mode == R.CLAMP_GRADIENT_MODES["upstream"]      # the product default
    try:
        for mode in modes:
            ref = P.reference(name, mode)              # asserts the scene's margins
            if name != P.LONG:
                P.check_caps(ref)
            R.set_clamp_gradient_mode(mode)
            stats = P.assert_parity(_run(ref.case), ref, f"HIP rasteriser, clamp gradient {mode}")
            print(name, mode, P.ratios(stats))
            if name in P.TIE_NAMES:      # one tile, nothing culled: its list is the whole scene, past the sort class
                assert R.last_stats["pairs"] == ref.case.m.shape[0] > P.TIE_LIST_CLASS[name], R.last_stats
    finally:
        R.set_clamp_gradient_mode("upstream")


def test_saturation_scene_is_bit_identical_run_to_run(built):
    """The gradient path is atomic-free with a fixed summation order: two runs agree in every bit."""
    c = P.case("saturation")
    _identical(_run(c), _run(c))


def test_longest_tie_scene_is_bit_identical_run_to_run(built):
    """4200 splats at 32 depths in one tile: the in-HBM sort decides every tie by the Gaussian index, so the list, the
    blend and the reverse walk agree in every bit."""
    c = P.case("ties_4200")
    _identical(_run(c), _run(c))


def test_grazing_scene_is_identical_after_the_capacity_retry(built):
    from monogs_amd import rasterizer as R
    ref = P.reference("grazing_49x33")
    a = _run(ref.case)
    pairs = R.last_stats["pairs"]
    assert pairs >= 128, pairs
    R._capacity_hint[_dev().index] = max(64, pairs // 2 // 64 * 64)      # too small: the blend stage must be re-run
    b = _run(ref.case)
    assert R.last_stats["retried"] and R.last_stats["pairs"] == pairs
    _identical(a, b)
    P.assert_parity(b, ref, "HIP rasteriser after the capacity retry")
