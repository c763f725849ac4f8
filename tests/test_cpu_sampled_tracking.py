"""Pixel-sampled first-order tracking, host side: the estimator of losses.sampled_tracking_surrogate is unbiased
(checked by exact enumeration over the draw), equals the reference's own formula for p = 1 without Huber, and the
C ABI's argument block has its ctypes mirror."""
import ctypes as C
import itertools

import pytest
import torch


def _toy(C_rows, n=37, seed=0):
    """A differentiable residual r(theta) [C, 1, n] in fp64: nonlinear, mixed signs, one exact zero pixel."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(C_rows * n, 4, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(C_rows * n, generator=g, dtype=torch.float64) * 0.05
    theta = torch.randn(4, generator=g, dtype=torch.float64).requires_grad_()

    def r():
        out = (torch.tanh(A @ theta) * 0.2 + b).view(C_rows, 1, n)
        return out * (torch.arange(n) != 5).to(out.dtype)     # pixel 5: zero residual in every row
    return theta, r


@pytest.mark.parametrize("rows,p,delta", list(itertools.product((3, 4), (1.0, 2.0, 3.0), (0.0, 0.01))))
def test_sampled_gradient_is_unbiased_by_exact_enumeration(rows, p, delta):
    """sum_i q_i g(i) = grad Phi to 1e-10, where g(i) is the K = 1 estimate for the draw i."""
    from monogs_amd.losses import HuberLoss, sampled_tracking_surrogate
    theta, r = _toy(rows, seed=rows * 10 + int(p))
    res = r()
    h = HuberLoss.apply(res, delta) if delta > 0 else res
    phi = torch.norm(h.flatten(), p=p)
    (want,) = torch.autograd.grad(phi, theta)
    with torch.no_grad():
        v = res.reshape(rows, -1).abs().sum(0) + 1e-8
        q = v / v.sum()
    n = q.numel()
    got = torch.zeros_like(want)
    for i in range(n):
        sur, phi_s = sampled_tracking_surrogate(r(), torch.tensor([i]), delta, p)
        (gi,) = torch.autograd.grad(sur, theta)
        got += q[i] * gi
        assert abs(float(phi_s) - float(phi)) <= 1e-12 * float(phi)
    assert (got - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item()), (got, want)


def test_p1_without_huber_is_the_reference_formula():
    """For p = 1 and no Huber the surrogate's gradient is that of the reference's
    loss_tracking = (1/K) sum_k vec1[i_k] / dist[i_k] (utils/slam_frontend.py:573-592)."""
    from monogs_amd.losses import sampled_tracking_surrogate
    theta, r = _toy(3, n=50, seed=3)
    g = torch.Generator().manual_seed(1)
    res = r()
    with torch.no_grad():
        v = res.reshape(3, -1).abs().sum(0) + 1e-8
    idx = torch.multinomial(v / v.sum(), 300, replacement=True, generator=g)
    sur, _ = sampled_tracking_surrogate(res, idx, 0.0, 1.0)
    (got,) = torch.autograd.grad(sur, theta)
    res = r()
    vec1 = res.reshape(3, -1).abs().sum(0)
    dist = (vec1.detach() + 1e-8) / (vec1.detach() + 1e-8).sum()
    ref = (vec1[idx] / dist[idx]).sum() / idx.numel()
    (want,) = torch.autograd.grad(ref, theta)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-15)
    assert abs(float(sur) - float(ref)) <= 1e-12 * float(ref)


def test_num_pixels_is_read_from_the_config():
    from monogs_amd.slam_loops import DEFAULT_CONFIG, sampled_num_pixels
    assert sampled_num_pixels(DEFAULT_CONFIG) == -1
    cfg = {"Training": {"RGN": {"use_huber": True, "huber_delta": 0.01, "pnorm": 1, "first_order": {"num_pixels": 300}}}}
    assert sampled_num_pixels(cfg) == 300


def test_sample_args_mirror(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_struct_size(23) == C.sizeof(_cabi.TrackingSampleArgs)
    assert _cabi.struct_mirrors()[23] is _cabi.TrackingSampleArgs
    sh = _cabi.RasterShape(1000, 640, 480, 0, 1, 10000, 0.6, 0.45, 1.0)
    n1 = L.mgs_tracking_sample_scratch_bytes(C.byref(sh), 4096)
    assert n1 >= 1200 * 256 * 4 + 4096 * 16
    assert L.mgs_tracking_sample_scratch_bytes(C.byref(sh), _cabi.TRACK_SAMPLE_MAX + 1) == 0
    assert L.mgs_tracking_sample_scratch_bytes(C.byref(sh), 0) == 0
