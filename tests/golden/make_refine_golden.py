"""Golden vectors for the colour-refinement objective, produced by RUNNING the reference's own Python on the CPU
(build container only; the reference tree does not exist on the GPU box):

    python tests/golden/make_refine_golden.py      ->  tests/golden/refine_loss_ref.npz

What is run (nothing of it is copied; only arrays - inputs and what the reference returned - are stored):
  * gaussian_splatting/utils/loss_utils.py: l1_loss (:21-22) and ssim (:61-101), combined as BackEnd.color_refinement
    combines them (utils/slam_backend.py:355-358) with lambda_dssim = 0.2 (opt_params, configs/*/base_config.yaml):
    loss = 0.8 l1_loss(image, gt) + 0.2 (1 - ssim(image, gt)), on [C,H,W] tensors as the reference passes them, in
    fp64 (the reference's window is built in fp32 and cast with type_as), and its autograd gradient w.r.t. image.

Cases: 3x120x160, 3x45x70, 3x7x9 (smaller than the window), 1x45x70, and a 3x45x70 pair with gt == image.  Images
are 8-bit levels (k / 255) so the file compresses; gt is a blurred, noisy, brightened copy of image.
loss_utils imports cv2 at its top for l1_loss_weight (not installed: an EMPTY module stands in; nothing of it runs).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path[:0] = [REF]
sys.modules["cv2"] = types.ModuleType("cv2")
import gaussian_splatting.utils.loss_utils as LU  # noqa: E402

LAMBDA = 0.2
CASES = {"c3_120x160": (3, 120, 160), "c3_45x70": (3, 45, 70), "c3_7x9": (3, 7, 9), "c1_45x70": (1, 45, 70),
         "same_45x70": (3, 45, 70)}


def pair(shape, g):
    C, H, W = shape
    base = torch.rand(C, H, W, generator=g, dtype=torch.float64)
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    k = (k[:, None] * k[None, :] / 16.0).expand(C, 1, 3, 3)
    img = torch.nn.functional.conv2d(base[None], k, padding=1, groups=C)[0]         # some spatial structure
    gt = 1.1 * torch.nn.functional.conv2d(img[None], k, padding=1, groups=C)[0] + 0.05 * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    q = lambda t: (t.clamp(0, 1) * 255).round() / 255
    return q(img).float(), q(gt).float()


def main():
    g = torch.Generator().manual_seed(2024)
    out = {"lambda_dssim": np.float64(LAMBDA)}
    for name, shape in CASES.items():
        img, gt = pair(shape, g)
        if name.startswith("same"):
            gt = img.clone()
        x = img.double().requires_grad_()
        y = gt.double()
        l1 = LU.l1_loss(x, y)
        s = LU.ssim(x, y)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)
        loss.backward()
        out[f"{name}_image"], out[f"{name}_gt"] = img.numpy(), gt.numpy()
        out[f"{name}_l1"], out[f"{name}_ssim"] = l1.detach().numpy(), s.detach().numpy()
        out[f"{name}_loss"], out[f"{name}_grad"] = loss.detach().numpy(), x.grad.numpy()
    path = os.path.join(HERE, "refine_loss_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
