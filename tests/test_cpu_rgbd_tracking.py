"""RGB-D tracking on the CPU: the stacked residual of losses.get_loss_tracking_stacked reproduces the reference's
numbers (tests/golden/rgbd_tracking_ref.npz, tests/golden/make_rgbd_tracking_golden.py), a monocular config keeps
the monocular residual, and the C ABI of the RGB-D entry points is exported and mirrored."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from monogs_amd import losses as Ls

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgbd_tracking_ref.npz")


@pytest.fixture(scope="module")
def G():
    return np.load(GOLD)


def _case(G, name):
    T_ = lambda k: torch.from_numpy(G[f"{name}_{k}"])
    a, b, eps = (float(v) for v in G[f"{name}_exposure"])
    vp = types.SimpleNamespace(original_image=T_("gt"), rgb_pixel_mask_mapping=T_("mask").bool(),
                               gt_depth=T_("gt_depth"), exposure_a=torch.tensor([a]), exposure_b=torch.tensor([b]),
                               exposure_eps=eps)
    alpha = float(G[f"{name}_alpha"])
    training = {"monocular": False}
    if alpha >= 0:
        training["alpha"] = alpha
    return vp, {"Training": training}, (0.95 if alpha < 0 else alpha), T_


def test_fixture_covers_the_edges(G):
    names = [str(n) for n in G["cases"]]
    a = [float(G[f"{n}_exposure"][0]) for n in names]
    assert min(a) < 0 < max(a)
    assert {float(G[f"{n}_alpha"]) for n in names} == {-1.0, 0.9}          # -1: no "alpha" key (0.95)
    for n in names:
        gd, op = G[f"{n}_gt_depth"], G[f"{n}_opacity"]
        assert (gd == 0).any() and ((gd > 0) & (gd < 0.01)).any() and (gd == np.float32(0.01)).any()
        assert (op == np.float32(0.95)).any() and (op > 0.95).any() and ((op < 0.95) & (op > 0.9)).any()


@pytest.mark.parametrize("name", ["a_pos_alpha_default", "a_neg_alpha_0.9", "a_pos_alpha_0.9", "a_neg_alpha_default"])
def test_stacked_residual_matches_the_reference(G, name):
    vp, config, alpha, T_ = _case(G, name)
    r = Ls.get_loss_tracking_stacked(config, T_("image"), T_("depth"), T_("opacity"), vp)
    H, W = r.shape[1:]
    assert r.shape == (4, H, W) and r.dtype == torch.float32
    # colour rows: alpha x the reference's get_loss_tracking_rgb_per_pixel on the exposed image
    assert torch.allclose(r[:3], alpha * T_("rgb_pp"), rtol=0, atol=1e-6)
    # the scalar identity with the reference's get_loss_tracking (RGB-D branch): pins the depth row
    s = float(r[:3].abs().sum() / (3 * H * W) + r[3].abs().sum() / (H * W))
    assert abs(s - float(G[f"{name}_scalar"])) <= 1e-6
    # the depth row is zero wherever one of the two masks is off
    dm = (T_("gt_depth") > 0.01) & (T_("opacity") > 0.95)
    assert bool((r[3][~dm[0]] == 0).all()) and bool((r[3][dm[0]] != 0).any())


def test_stacked_residual_is_differentiable_in_image_depth_and_exposure(G):
    vp, config, alpha, T_ = _case(G, "a_neg_alpha_0.9")
    vp.exposure_a.requires_grad_()
    img, dep = T_("image").requires_grad_(), T_("depth").requires_grad_()
    r = Ls.get_loss_tracking_stacked(config, img, dep, T_("opacity"), vp)
    r.abs().sum().backward()
    dm = (T_("gt_depth") > 0.01) & (T_("opacity") > 0.95)
    assert torch.equal(dep.grad != 0, dm)
    assert abs(float(dep.grad[dm].abs().max()) - (1 - alpha)) < 1e-6
    assert float(img.grad.abs().sum()) > 0 and vp.exposure_a.grad is not None


def test_monocular_config_keeps_the_monocular_residual(G):
    vp, _, _, T_ = _case(G, "a_pos_alpha_default")
    mono = {"Training": {"monocular": True, "alpha": 0.5}}
    args = (T_("image"), T_("depth"), T_("opacity"), vp)
    assert torch.equal(Ls.get_loss_tracking_stacked(mono, *args), Ls.get_loss_tracking_per_pixel(mono, *args))
    with pytest.raises(NotImplementedError):        # unchanged: the per-pixel RGB-D form still raises
        Ls.get_loss_tracking_per_pixel({"Training": {"monocular": False}}, *args)


def test_rgbd_entry_points_are_exported_and_mirrored(built):
    from monogs_amd import _cabi
    lib = C.CDLL(_cabi.LIB_PATH)
    for name in ("mgs_tracking_iteration_rgbd", "mgs_tracking_iteration_second_order_rgbd",
                 "mgs_tracking_loss_rgbd_fused", "mgs_sketch_residual_rgbd"):
        assert hasattr(lib, name)
        assert name in _cabi.EXPORTS
    L = _cabi.lib()
    assert L.mgs_abi_version() == 10
    assert L.mgs_struct_size(22) == C.sizeof(_cabi.TrackingDepthArgs) == 40
    assert _cabi.struct_mirrors()[22] is _cabi.TrackingDepthArgs
