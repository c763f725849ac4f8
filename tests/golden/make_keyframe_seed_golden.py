"""Golden vectors for the keyframe seeding path's depth prior, produced by RUNNING the reference's own Python on the CPU
(build container only; the reference tree does not exist on the GPU box):

    python tests/golden/make_keyframe_seed_golden.py      ->  tests/golden/keyframe_seed_ref.npz

What is run (nothing of it is copied; only arrays - inputs and what the reference returned - are stored):
  * utils/slam_frontend.py: FrontEnd.add_new_keyframe (:183-234), called unbound with a SimpleNamespace `self` holding
    config, cameras (.original_image, .depth), device, monocular and kf_indices; torch.randn_like is wrapped inside the
    reference module to record the noise it drew;
  * utils/slam_utils.py: get_median_depth (:286-297, return_std=True) of each monocular case's depth / opacity;
  * np.median of the returned depth map, the statistic gaussian_model.py:143 scales the point size with.
open3d is not installed, so create_pcd_from_image_and_depth itself cannot be run.
slam_frontend imports cv2, diff_gaussian_rasterization, open3d, plyfile, simple_knn, evo, torchmetrics, wandb and
lietorch at its top (not installed: empty modules stand in; nothing of them runs).

For every monocular case with rendered depth the generator also evaluates the unbiased standard deviation in fp64 and
asserts that the reference's own fp32 value, against it, leaves at most 0.1 % of the pixels inside the band where the
outlier test could flip (|d - (median +- std)| <= |std_fp32 - std_fp64|): the cap the tests give the mirror.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path[:0] = [REF]
STUBS = ("cv2", "diff_gaussian_rasterization", "open3d", "plyfile", "simple_knn", "evo", "torchmetrics", "wandb",
         "lietorch")
RGB_BOUNDARY_THRESHOLD = 0.01
BAND_CAP = 1e-3


class _Stub(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return type(n, (), {})


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        return importlib.machinery.ModuleSpec(name, self, is_package=True) if name.split(".")[0] in STUBS else None

    def create_module(self, spec):
        m = _Stub(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _StubFinder())
import utils.slam_frontend as F  # noqa: E402
import utils.slam_utils as SU  # noqa: E402


class _Recorder:
    """Stands in for the torch module inside slam_frontend: records what randn_like drew."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, n):
        return getattr(torch, n)

    def randn_like(self, x, *a, **k):
        z = torch.randn_like(x, *a, **k)
        self._log.append(z.clone())
        return z


def smooth(g, H, W, lo, hi):
    """A smooth random field in [lo, hi]: a coarse grid, bilinearly enlarged."""
    c = torch.rand(1, 1, max(2, H // 16 + 2), max(2, W // 16 + 2), generator=g)
    f = torch.nn.functional.interpolate(c, size=(H, W), mode="bilinear", align_corners=True)[0, 0]
    return lo + (hi - lo) * f


def make_inputs(kind, H, W, g):
    """Inputs on grids that store compactly: image and opacity in 1/255 steps, depth in millimetres."""
    image_u8 = torch.stack([smooth(g, H, W, 0.05, 0.95) for _ in range(3)]).mul(255).round().to(torch.uint8)
    depth = smooth(g, H, W, 1.0, 4.0) + 0.02 * torch.randn(H, W, generator=g)
    opacity_u8 = torch.randint(244, 256, (H, W), generator=g).to(torch.uint8)     # 244 / 255 = 0.957 > 0.95
    far = torch.rand(H, W, generator=g) < 0.03                    # a few far outliers
    depth[far] = depth[far] * 3.0
    if kind == "dark_border":
        b = max(2, H // 10)
        image_u8[:, :b, :] = 0
        image_u8[:, -b:, :] = 0
        image_u8[:, :, :b] = torch.tensor([1, 1, 0], dtype=torch.uint8)[:, None, None]    # sum 0.0078: below 0.01
        image_u8[:, H // 2, W // 2] = 1                                                    # sum 0.0118: above
    if kind == "holes":
        depth[H // 4:H // 3, W // 5:W // 2] = 0.0                 # no depth rendered
        depth[torch.rand(H, W, generator=g) < 0.05] = 0.0
        opacity_u8[H // 2:, : W // 3] = torch.randint(120, 243, (H - H // 2, W // 3), generator=g).to(torch.uint8)
    depth_mm = depth.mul(1000).round().clamp(0, 65535).to(torch.int32)
    return image_u8, depth_mm.to(torch.uint16), opacity_u8


def decode(image_u8, depth_mm, opacity_u8):
    """The fp32 inputs the stored integers stand for (the tests decode the same way)."""
    image = torch.from_numpy(image_u8.astype(np.float32) / np.float32(255.0))
    depth = torch.from_numpy(depth_mm.astype(np.float32) * np.float32(0.001))
    opacity = torch.from_numpy(opacity_u8.astype(np.float32) / np.float32(255.0))
    return image, depth, opacity


# name: (kind, H, W, branch)
CASES = {
    "mono_160x120": ("plain", 120, 160, "rendered"),
    "mono_off_grid": ("plain", 53, 75, "rendered"),
    "mono_dark_border": ("dark_border", 72, 96, "rendered"),
    "mono_holes_low_opacity": ("holes", 72, 96, "rendered"),
    "mono_first_keyframe": ("dark_border", 48, 64, "initial"),
    "sensor_depth": ("holes", 48, 64, "sensor"),
}


def run_case(name, spec, g):
    kind, H, W, branch = spec
    image_u8, depth_mm, opacity_u8 = (t.numpy() for t in make_inputs(kind, H, W, g))
    image, depth, opacity = decode(image_u8, depth_mm, opacity_u8)
    view = types.SimpleNamespace(original_image=image, depth=depth.numpy().copy())
    self_ = types.SimpleNamespace(config={"Training": {"rgb_boundary_threshold": RGB_BOUNDARY_THRESHOLD}},
                                  kf_indices=[], cameras={7: view}, device="cpu", monocular=branch != "sensor")
    log = []
    F.torch = _Recorder(log)
    try:
        torch.manual_seed(int(g.initial_seed()) + len(name))
        if branch == "rendered":
            out = F.FrontEnd.add_new_keyframe(self_, 7, depth=depth[None].clone(), opacity=opacity[None].clone())
        else:
            out = F.FrontEnd.add_new_keyframe(self_, 7, init=True)
    finally:
        F.torch = torch
    out = np.asarray(out, dtype=np.float32)
    assert out.shape == (H, W) and self_.kf_indices == [7]
    res = {"H": np.int32(H), "W": np.int32(W), "mode": np.int32({"rendered": 0, "initial": 1, "sensor": 2}[branch]),
           "image_u8": image_u8, "initial_depth": out,
           "median_all": np.asarray(np.median(out), dtype=np.float32)}
    msg = ""
    if branch != "initial":
        res["depth_mm"] = depth_mm
    if branch != "sensor":
        assert len(log) == 1
        res["noise"] = log[0][0].numpy()
    if branch == "rendered":
        res["opacity_u8"] = opacity_u8
        valid_rgb = (image.sum(dim=0) > RGB_BOUNDARY_THRESHOLD)[None]
        med, std, valid = SU.get_median_depth(depth[None], opacity[None], mask=valid_rgb, return_std=True)
        v64 = depth[None][valid].double()
        std64 = float(v64.std())
        band = abs(float(std) - std64)
        d64 = depth.double()
        near = ((d64 - (float(med) + float(std))).abs() <= band) | ((d64 - (float(med) - float(std))).abs() <= band)
        assert int(near.sum()) <= BAND_CAP * H * W, (name, int(near.sum()))
        res.update(median_depth=med.numpy().astype(np.float32), std=std.numpy().astype(np.float32),
                   std_fp64=np.float64(std64), valid_mask=np.packbits(valid[0].numpy()))
        msg = (f"median {float(med):.6g} std {float(std):.8g} (fp64 {std64:.10g}, |diff| {band:.3g}) "
               f"valid {int(valid.sum())} in the band {int(near.sum())}")
    print(f"{name:24s} {H}x{W} np.median {float(res['median_all']):.6g} {msg}")
    return res


def main():
    g = torch.Generator().manual_seed(20261016)
    out = {"names": np.array(list(CASES)), "rgb_boundary_threshold": np.float32(RGB_BOUNDARY_THRESHOLD)}
    for name, spec in CASES.items():
        for k, v in run_case(name, spec, g).items():
            out[f"{name}_{k}"] = v
    path = os.path.join(HERE, "keyframe_seed_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
