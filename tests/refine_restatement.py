"""The colour-refinement objective restated for the tests - the yardstick the GPU tests hold mgs_ssim_loss to,
itself held to the reference's numbers in tests/golden/refine_loss_ref.npz by tests/test_cpu_refine.py.

The SSIM is eval_metrics.ssim_map's arithmetic (pinned to the reference's loss_utils.ssim) with the window built
as loss_utils.gaussian / create_window build it: exp in double precision, stored and normalised in fp32, the
outer product in fp32.  eval_metrics._gauss_window evaluates exp in fp32, which moves the loss by ~1e-9 - within
what the scoring path needs, not within the 1e-12 this restatement is held to."""
import math

import torch
import torch.nn.functional as F


def reference_window(channels, like, size=11, sigma=1.5):
    g = torch.tensor([math.exp(-((x - size // 2) ** 2) / float(2 * sigma ** 2)) for x in range(size)],
                     dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w.expand(channels, 1, size, size).contiguous().to(like)


def ssim(img1, img2, size=11):
    """Mean SSIM of [C,H,W] images (zero padding, C1 = 0.01^2, C2 = 0.03^2)."""
    ch = img1.shape[-3]
    w = reference_window(ch, img1, size)
    pad = size // 2
    conv = lambda t: F.conv2d(t, w, padding=pad, groups=ch)
    mu1, mu2 = conv(img1), conv(img2)
    s11 = conv(img1 * img1) - mu1 * mu1
    s22 = conv(img2 * img2) - mu2 * mu2
    s12 = conv(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return m.mean()


def refine_loss_and_grad(image, gt, lambda_dssim=0.2, dtype=torch.float64):
    """(loss, l1, ssim, d loss / d image) of (1 - lambda) mean|x - y| + lambda (1 - ssim(x, y)) under autograd,
    in `dtype` on the inputs' device."""
    x = image.detach().to(dtype).clone().requires_grad_()
    y = gt.detach().to(dtype)
    l1 = torch.abs(x - y).mean()
    s = ssim(x, y)
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s)
    loss.backward()
    return loss.detach(), l1.detach(), s.detach(), x.grad
