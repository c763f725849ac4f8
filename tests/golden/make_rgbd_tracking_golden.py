"""Golden vectors for the stacked RGB-D tracking residual, produced by RUNNING the reference's own Python on the CPU
(build container only; the reference tree does not exist on the GPU box):

    python tests/golden/make_rgbd_tracking_golden.py      ->  tests/golden/rgbd_tracking_ref.npz

What is run (nothing of it is copied; only arrays - inputs and what the reference returned - are stored):
  * utils/slam_utils.py: get_loss_tracking_rgb_per_pixel (:201-205) on the exposed image (|a| + eps) image + b, the
    colour rows the stacked residual must carry times alpha;
  * utils/slam_utils.py: get_loss_tracking (:83-113, RGB-D branch) with viewpoint.rgb_pixel_mask set to the mapping
    mask, the scalar that pins the depth row, both masks, their thresholds and alpha:
        get_loss_tracking = sum |r[:3]| / (3 H W) + sum |r[3]| / (H W).
The reference's get_loss_tracking_rgbd_per_pixel itself raises (:220), so it is not run.

Cases cover exposure a > 0 and a < 0, alpha 0.95 (the default: no "alpha" key) and 0.9 (configs/rgbd/tum), sensor depth
with zeros, values below 0.01 and values exactly 0.01, and rendered opacity around 0.95 (exactly 0.95 included).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
import utils.configs as _cfg  # noqa: E402

_cfg.cuda_device = "cpu"
from utils.slam_utils import get_loss_tracking, get_loss_tracking_rgb_per_pixel  # noqa: E402

H, W = 24, 32
CASES = {"a_pos_alpha_default": (1.15, 0.03, None), "a_neg_alpha_0.9": (-0.85, -0.02, 0.9),
         "a_pos_alpha_0.9": (0.7, 0.0, 0.9), "a_neg_alpha_default": (-1.3, 0.05, None)}


def inputs(g):
    image = torch.rand(3, H, W, generator=g)
    gt = (image + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt[:, :3, :] = 0.0                                       # rows without image content: mask 0
    mask = (gt.sum(dim=0) > 0.01).view(1, H, W)
    depth = 1.0 + 2.0 * torch.rand(1, H, W, generator=g)
    gt_depth = depth + 0.2 * torch.randn(1, H, W, generator=g)
    sel = torch.rand(1, H, W, generator=g)
    gt_depth[sel < 0.15] = 0.0                               # no measurement
    gt_depth[(sel >= 0.15) & (sel < 0.22)] = 0.005           # below the threshold
    gt_depth[(sel >= 0.22) & (sel < 0.29)] = 0.01            # exactly the threshold (masked out: strict >)
    opacity = 0.9 + 0.1 * torch.rand(1, H, W, generator=g)   # straddles 0.95
    o = torch.rand(1, H, W, generator=g)
    opacity[o < 0.1] = 0.95                                  # exactly the threshold (masked out: strict >)
    opacity[(o >= 0.1) & (o < 0.2)] = 0.3
    return image, gt, mask, depth, gt_depth, opacity


def main():
    g = torch.Generator().manual_seed(7)
    out = {"cases": np.array(list(CASES))}
    for name, (a, b, alpha) in CASES.items():
        image, gt, mask, depth, gt_depth, opacity = inputs(g)
        eps = 1e-8
        ea, eb = torch.tensor([a]), torch.tensor([b])
        vp = types.SimpleNamespace(original_image=gt, rgb_pixel_mask_mapping=mask, rgb_pixel_mask=mask,
                                   grad_mask=torch.ones(1, H, W), gt_depth=gt_depth, exposure_a=ea, exposure_b=eb,
                                   exposure_eps=eps)
        training = {"monocular": False, "rgb_boundary_threshold": 0.01}
        if alpha is not None:
            training["alpha"] = alpha
        config = {"Training": training}
        image_ab = (torch.abs(ea) + eps) * image + eb
        rgb_pp = get_loss_tracking_rgb_per_pixel(config, image_ab, depth, opacity, vp)
        scalar = get_loss_tracking(config, image, depth, opacity, vp)
        for k, v in (("image", image), ("gt", gt), ("mask", mask.float()), ("depth", depth), ("gt_depth", gt_depth),
                     ("opacity", opacity), ("rgb_pp", rgb_pp), ("scalar", scalar)):
            out[f"{name}_{k}"] = v.detach().numpy().astype(np.float32)
        out[f"{name}_exposure"] = np.array([a, b, eps], dtype=np.float64)
        out[f"{name}_alpha"] = np.float64(-1.0 if alpha is None else alpha)
    np.savez_compressed(os.path.join(HERE, "rgbd_tracking_ref.npz"), **out)


if __name__ == "__main__":
    main()
