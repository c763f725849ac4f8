"""Golden vector for tests/test_cpu_eval.py: what the reference's own PSNR helper
(gaussian_splatting/utils/image_utils.py, pure torch) returns on the test's seeded inputs.

    python tests/golden/make_psnr_golden.py <reference tree>   # -> tests/golden/reference_psnr.npz

Only arrays (inputs and the reference's output) are stored; no reference source is copied.
"""
import importlib.util
import os
import sys

import numpy as np
import torch


def inputs():
    g = torch.Generator().manual_seed(1)
    a = torch.rand(2, 3, 24, 32, generator=g)
    b = (a + 0.05 * torch.randn(2, 3, 24, 32, generator=g)).clamp(0, 1)
    return a, b


if __name__ == "__main__":
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location(
        "ref_image_utils", os.path.join(ref, "gaussian_splatting", "utils", "image_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a, b = inputs()
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_psnr.npz")
    np.savez_compressed(dst, a=a.numpy(), b=b.numpy(), psnr=mod.psnr(a, b).numpy())
    print(dst, mod.psnr(a, b).reshape(-1).tolist())
