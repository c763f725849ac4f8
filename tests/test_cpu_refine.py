"""Colour refinement (utils/slam_backend.py:335-368) on the CPU: the fp64 restatement the GPU tests use reproduces
the reference's own numbers (tests/golden/refine_loss_ref.npz, tests/golden/make_refine_golden.py), and the C ABI
of the fused objective and the refinement iteration is exported, versioned and mirrored."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from refine_restatement import refine_loss_and_grad

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_loss_ref.npz")
CASES = ("c3_120x160", "c3_45x70", "c3_7x9", "c1_45x70", "same_45x70")


@pytest.fixture(scope="module")
def G():
    return np.load(GOLD)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference(G, case):
    img, gt = torch.from_numpy(G[f"{case}_image"]), torch.from_numpy(G[f"{case}_gt"])
    loss, l1, s, grad = refine_loss_and_grad(img, gt, float(G["lambda_dssim"]))
    assert abs(float(loss) - float(G[f"{case}_loss"])) <= 1e-12
    assert abs(float(l1) - float(G[f"{case}_l1"])) <= 1e-12
    assert abs(float(s) - float(G[f"{case}_ssim"])) <= 1e-12
    want = torch.from_numpy(G[f"{case}_grad"])
    assert grad.shape == want.shape
    if case.startswith("same"):     # gradient zero up to rounding on both sides: nothing to be relative to
        assert float(grad.abs().max()) <= 1e-15 and float(want.abs().max()) <= 1e-15
    else:
        assert float((grad - want).norm()) <= 1e-10 * float(want.norm())


def test_eval_metrics_ssim_agrees_with_the_restatement(G):
    """The scoring path's SSIM differs from the restatement only by its fp32 exp in the window."""
    from monogs_amd import eval_metrics
    from refine_restatement import ssim
    x = torch.from_numpy(G["c3_45x70_image"]).double()
    y = torch.from_numpy(G["c3_45x70_gt"]).double()
    assert abs(float(eval_metrics.ssim(x, y)) - float(ssim(x, y))) < 1e-7


def test_fixture_is_small_and_covers_the_cases(G):
    assert os.path.getsize(GOLD) < 1 << 20
    assert G["c3_7x9_image"].shape == (3, 7, 9) and G["c1_45x70_image"].shape == (1, 45, 70)
    assert np.array_equal(G["same_45x70_image"], G["same_45x70_gt"])


def test_refinement_entry_points_are_exported(built):
    from monogs_amd import _cabi
    lib = C.CDLL(_cabi.LIB_PATH)
    for name in ("mgs_ssim_loss", "mgs_ssim_loss_partial_count", "mgs_refine_view_iteration"):
        assert hasattr(lib, name)
        assert name in _cabi.EXPORTS
    assert _cabi.ABI_VERSION == 10
    assert _cabi.lib().mgs_abi_version() == 10


def test_refinement_struct_mirrors(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_struct_size(20) == C.sizeof(_cabi.SsimLossArgs)
    assert L.mgs_struct_size(21) == C.sizeof(_cabi.RefineViewArgs)
    assert _cabi.struct_mirrors()[20] is _cabi.SsimLossArgs and _cabi.struct_mirrors()[21] is _cabi.RefineViewArgs


def test_partial_count_is_host_only(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    # 640x480: 20 x 15 tiles of 32x32 per channel, two partials each, one ticket
    assert L.mgs_ssim_loss_partial_count(3, 480, 640) == 2 * 3 * 20 * 15 + 1
    assert L.mgs_ssim_loss_partial_count(3, 7, 9) == 2 * 3 + 1
    assert L.mgs_ssim_loss_partial_count(0, 7, 9) < 0


def test_color_refinement_loss_refuses_cpu_tensors(built):
    from monogs_amd.tracking_fused import color_refinement_loss
    img = torch.rand(3, 16, 16, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        color_refinement_loss(img, torch.rand(3, 16, 16))
