"""Keyframe seeding: from a tracked frame to the rows of its new Gaussians (DESIGN.md "Keyframe seeding on the device").

The reference does this in two places: FrontEnd.add_new_keyframe (utils/slam_frontend.py:183-234) prepares the depth
map a keyframe is back-projected with, GaussianModel.create_pcd_from_image_and_depth
(gaussian_splatting/scene/gaussian_model.py:137-205) turns it into points with open3d on the host.  Five steps:

  1. depth prior     mode 0 (monocular, rendered depth): outliers beyond one std of the median, and pixels that are
                     not valid, are replaced by the median; noise of 0.5 std (replaced) / 0.2 std (kept) is added.
                     mode 1 (monocular, first keyframe or reset): 2 + 0.3 noise.  mode 2: the sensor's depth.
                     Modes 0 and 2: pixels without image content (sum of the channels <= rgb_boundary_threshold)
                     get depth 0 (the reference's first-keyframe branch does not apply that mask).
  2. point size      min(0.05, point_size * np.median(depth map)): NumPy's median - all pixels, zeros included, the
                     mean of the two middle values for an even count.
  3. sub-sample      K = floor(n / downsample) of the n pixels with 0 < d <= depth_trunc: every pixel has a 32-bit key,
                     the K smallest (key, pixel index) pairs are kept, in ascending pixel order.
  4. back-projection xyz = R^T (p_cam - t), colour through the exposure and the reference's uint8 truncation, RGB2SH.
  5. scale           log(sqrt(max(dist2, 1e-7) * point_size)) with dist2 from the HIP k-nn (distCUDA2).

Two implementations:
  * `seed_torch` and the step functions below: the torch mirror, on CPU or GPU tensors - the documentation of the
    semantics and the yardstick of the native path.  `noise` / `keys` replay the random inputs.
  * `KeyframeSeeder`: one `mgs_keyframe_seed` call (keyframe_seed.hip) with a single read of the result record.

Against the older torch path (slam_surrogate.keyframe_depth + keyframe_init.create_pcd_from_image_and_depth) this one
follows the reference in two places where that one follows intent: the point size takes NumPy's median (not
torch.median's lower median), and the depth prior is pinned to add_new_keyframe's own outputs
(tests/golden/keyframe_seed_ref.npz).  Which pixels open3d's generator would keep stays unpinned in both.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional

import torch

from . import _cabi
from .sh import RGB2SH

MODE_RENDERED, MODE_INITIAL, MODE_SENSOR = 0, 1, 2
DEFAULT_DATASET = {"pcd_downsample": 64, "pcd_downsample_init": 32, "point_size": 0.01, "adaptive_pointsize": True}


# ---- the torch mirror -------------------------------------------------------------------------------------------------
def depth_prior_torch(image, depth, opacity, mode, noise=None, rgb_boundary_threshold=0.01, generator=None):
    """Step 1.  image [3,H,W]; depth / opacity [H,W] (or [1,H,W]) as the mode needs them; noise [H,W] replays the
    normal draws.  Returns (d [H,W], info) with info = {median_depth, std_depth, n_valid, n_outliers, valid_mask}
    (tensors / None outside mode 0).  std is the unbiased standard deviation evaluated in fp64 and rounded once."""
    H, W = image.shape[1:]
    dev = image.device
    valid_rgb = image.sum(dim=0) > rgb_boundary_threshold
    info = {"median_depth": None, "std_depth": None, "n_valid": 0, "n_outliers": 0, "valid_mask": None}

    def normal():
        if noise is not None:
            return noise.reshape(H, W).to(dev, torch.float32)
        return torch.randn(H, W, device=dev, generator=generator)

    if mode == MODE_SENSOR:
        d = depth.reshape(H, W).to(torch.float32).clone()
    elif mode == MODE_INITIAL:
        d = 2 * torch.ones(H, W, device=dev)
        d += normal() * 0.3
    elif mode == MODE_RENDERED:
        d = depth.detach().reshape(H, W).to(torch.float32).clone()
        valid = (d > 0) & (opacity.detach().reshape(H, W) > 0.95) & valid_rgb
        v = d[valid]
        info["n_valid"], info["valid_mask"] = int(v.numel()), valid
        if v.numel() >= 1:
            info["median_depth"] = v.median()
        if v.numel() < 2:
            d = 2 * torch.ones(H, W, device=dev)        # the reference is undefined here (std of one value is NaN)
        else:
            med = v.median()
            x = v.double() - med.double()
            n = float(v.numel())
            var = ((x * x).sum() - x.sum() ** 2 / n) / (n - 1.0)
            std = var.clamp_min(0.0).sqrt().float()
            info["std_depth"] = std
            bad = (d > med + std) | (d < med - std) | ~valid
            info["n_outliers"] = int(bad.sum())
            d[bad] = med
            d = d + normal() * torch.where(bad, std * 0.5, std * 0.2)
    else:
        raise ValueError(f"mode {mode}: 0 (rendered depth), 1 (initial) or 2 (sensor depth)")
    if mode != MODE_INITIAL:             # add_new_keyframe's first-keyframe branch returns before this mask
        d[~valid_rgb] = 0
    d[~torch.isfinite(d)] = 0            # a non-finite depth is no depth: the k-nn never sees one
    return d, info


def median_all_torch(d):
    """Step 2's statistic: np.median of every value of d, as an fp32 0-dim tensor."""
    s = d.reshape(-1).sort().values
    n = s.numel()
    if n % 2:
        return s[n // 2].clone()
    return (s[n // 2 - 1] + s[n // 2]) * 0.5


def point_size_torch(d, point_size=0.01, adaptive_pointsize=True) -> float:
    if not adaptive_pointsize:
        return float(point_size)
    return min(0.05, point_size * float(median_all_torch(d)))


def select_torch(d, keys, downsample, depth_trunc=100.0):
    """Step 3.  keys [H*W] integers in [0, 2^32).  Returns (sel, n): the flat indices of the kept pixels, ascending,
    and the number of usable pixels."""
    flat = d.reshape(-1)
    idx = torch.nonzero((flat > 0) & (flat <= depth_trunc)).reshape(-1)
    n = int(idx.numel())
    keep = int(n / downsample)
    k = keys.reshape(-1).to(flat.device, torch.int64)[idx]
    order = torch.sort(k, stable=True).indices[:keep]           # ties: the lower pixel index first
    return torch.sort(idx[order]).values, n


def backproject_torch(cam, image, d, sel):
    """Step 4, the arithmetic of keyframe_init.create_pcd_from_image_and_depth for the pixels `sel`:
    (xyz [K,3], colour [K,3], features_dc [K,3])."""
    W = d.shape[-1]
    img = (torch.abs(cam.exposure_a.detach()) + cam.exposure_eps) * image + cam.exposure_b.detach()
    rgb = torch.floor(torch.clamp(img, 0.0, 1.0) * 255.0) / 255.0
    v, u = torch.div(sel, W, rounding_mode="floor").float(), (sel % W).float()
    z = d.reshape(-1)[sel].float()
    p_cam = torch.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], dim=1)
    T = cam.T.detach().to(d.device, torch.float32)
    xyz = (p_cam - T[:3, 3]) @ T[:3, :3]
    col = rgb.reshape(3, -1)[:, sel].t().contiguous()
    return xyz, col, RGB2SH(col)


def seed_torch(cam, image, depth, opacity, mode, *, downsample, point_size=0.01, adaptive_pointsize=True,
               isotropic=True, depth_trunc=100.0, rgb_boundary_threshold=0.01, noise=None, keys=None, generator=None,
               dist2_fn: Optional[Callable] = None):
    """The five steps on torch tensors (CPU or GPU).  `dist2_fn(xyz) -> [K]`: the mean squared distance to the three
    nearest neighbours; None takes the HIP k-nn (GPU tensors only).  Returns a dict: depth, sel, n_depth, xyz, colour,
    features_dc, log_scales, rots, opacity_logit, point_size, median_all and step 1's info."""
    with torch.no_grad():
        image = image.detach().float()
        d, info = depth_prior_torch(image, depth, opacity, mode, noise, rgb_boundary_threshold, generator)
        med_all = median_all_torch(d)
        ps = point_size_torch(d, point_size, adaptive_pointsize)
        if keys is None:
            keys = torch.randint(0, 2 ** 32, (d.numel(),), device=d.device, generator=generator, dtype=torch.int64)
        sel, n = select_torch(d, keys, downsample, depth_trunc)
        xyz, col, fdc = backproject_torch(cam, image, d, sel)
        K = int(sel.numel())
        if dist2_fn is None:
            from .knn import distCUDA2
            dist2_fn = distCUDA2
        dist2 = dist2_fn(xyz.contiguous()) if K else torch.zeros(0, device=d.device)
        scales = torch.log(torch.sqrt(torch.clamp_min(dist2, 1e-7) * ps))[:, None]
        if not isotropic:
            scales = scales.repeat(1, 3)
        rots = torch.zeros(K, 4, device=d.device)
        rots[:, 0] = 1.0
        out = dict(info)
        out.update(depth=d, sel=sel, n_depth=n, xyz=xyz, colour=col, features_dc=fdc, log_scales=scales, rots=rots,
                   opacity_logit=torch.zeros(K, 1, device=d.device), point_size=ps, median_all=med_all, keys=keys)
    return out


# ---- the native path --------------------------------------------------------------------------------------------------
def _keys_as_int32(keys, dev):
    """Integers in [0, 2^32) (or int32 bit patterns) -> the int32 tensor holding the same 32 bits."""
    if keys.dtype == torch.int32:
        return keys.to(dev).reshape(-1).contiguous()
    k = keys.to(dev, torch.int64).reshape(-1)
    return ((k + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).contiguous()


class KeyframeSeeder:
    """Owns the scratch, the output rows and the result record of mgs_keyframe_seed for one image size.  `config`: a
    reference-shaped dict (Dataset.{pcd_downsample, pcd_downsample_init, point_size, adaptive_pointsize},
    Training.rgb_boundary_threshold).  The tensors `seed` returns are views of the seeder's own buffers: they hold
    until the next call (GaussianModel.extend_from_pcd copies them into the map)."""

    def __init__(self, H: int, W: int, device, config: Optional[dict] = None, *, isotropic: bool = True,
                 max_sh_degree: int = 0, depth_trunc: float = 100.0):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mgs_keyframe_seed runs on the GPU only (HIP kernels, gfx950)")
        ds = dict(DEFAULT_DATASET)
        ds.update({k: v for k, v in ((config or {}).get("Dataset") or {}).items() if k in DEFAULT_DATASET})
        self.dataset = ds
        self.rgb_boundary_threshold = float(((config or {}).get("Training") or {}).get("rgb_boundary_threshold", 0.01))
        self.H, self.W, self.device = int(H), int(W), device
        self.isotropic, self.max_sh_degree, self.depth_trunc = bool(isotropic), int(max_sh_degree), float(depth_trunc)
        smallest = min(float(ds["pcd_downsample"]), float(ds["pcd_downsample_init"]))
        if not smallest >= 1:
            raise ValueError("pcd_downsample and pcd_downsample_init must be at least 1 (1 / downsample of the usable "
                             "pixels is kept; mgs_keyframe_seed refuses a smaller value)")
        self.capacity = max(1, math.ceil(H * W / smallest))
        nbytes = int(_cabi.lib().mgs_keyframe_seed_scratch_bytes(H * W, self.capacity))
        if nbytes == 0:
            raise ValueError(f"mgs_keyframe_seed_scratch_bytes({H * W}, {self.capacity}) refused the sizes")
        P = self.capacity
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.xyz = torch.empty(P, 3, device=device)
        self.features_dc = torch.empty(P, 3, device=device)
        self.log_scales = torch.empty(P, 1 if self.isotropic else 3, device=device)
        self.rots = torch.empty(P, 4, device=device)
        self.opacity_logit = torch.empty(P, 1, device=device)
        self.pixel_index = torch.empty(P, dtype=torch.int32, device=device)
        self.depth_out = torch.empty(H, W, device=device)
        self.result = torch.zeros(C.sizeof(_cabi.KeyframeSeedResult), dtype=torch.uint8, device=device)
        self.record = _cabi.KeyframeSeedResult()

    def native_args(self, cam, image, depth, opacity, mode, init, seed, noise=None, keys=None):
        """The mgs_keyframe_seed_args of one call (and the tensors its pointers refer to)."""
        HW, dev = self.H * self.W, self.device

        def plane(t, name):
            if t is None:
                return None
            t = t.detach().to(dev, torch.float32).reshape(-1).contiguous()
            if t.numel() != HW:
                raise ValueError(f"{name} has {t.numel()} elements, the image {HW}")
            return t

        image = image.detach().to(dev, torch.float32).contiguous()
        if tuple(image.shape) != (3, self.H, self.W):
            raise ValueError(f"image is {tuple(image.shape)}, the seeder was built for (3, {self.H}, {self.W})")
        depth, opacity, noise = plane(depth, "depth"), plane(opacity, "opacity"), plane(noise, "noise")
        keys = None if keys is None else _keys_as_int32(keys, dev)
        if keys is not None and keys.numel() != HW:
            raise ValueError(f"keys has {keys.numel()} elements, the image {HW}")
        T = cam.T.detach().to(dev, torch.float32).contiguous()
        ea = cam.exposure_a.detach().to(dev, torch.float32).reshape(-1).contiguous()
        eb = cam.exposure_b.detach().to(dev, torch.float32).reshape(-1).contiguous()
        a = _cabi.KeyframeSeedArgs()
        a.width, a.height, a.row_capacity, a.mode = self.W, self.H, self.capacity, int(mode)
        a.adaptive_pointsize, a.isotropic = int(bool(self.dataset["adaptive_pointsize"])), int(self.isotropic)
        a.fx, a.fy, a.cx, a.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
        a.rgb_boundary_threshold = self.rgb_boundary_threshold
        a.downsample = float(self.dataset["pcd_downsample_init" if init else "pcd_downsample"])
        a.depth_trunc, a.exposure_eps = self.depth_trunc, float(cam.exposure_eps)
        a.point_size, a.seed = float(self.dataset["point_size"]), int(seed) & (2 ** 64 - 1)
        ptr = lambda t: None if t is None else t.data_ptr()
        a.image, a.depth, a.opacity, a.T = ptr(image), ptr(depth), ptr(opacity), ptr(T)
        a.exposure_a, a.exposure_b, a.noise, a.keys = ptr(ea), ptr(eb), ptr(noise), ptr(keys)
        a.xyz, a.features_dc, a.log_scales = ptr(self.xyz), ptr(self.features_dc), ptr(self.log_scales)
        a.rots, a.opacity_logit, a.pixel_index = ptr(self.rots), ptr(self.opacity_logit), ptr(self.pixel_index)
        a.depth_out, a.scratch, a.result = ptr(self.depth_out), ptr(self.scratch), ptr(self.result)
        a.result_host = C.pointer(self.record)
        return a, (image, depth, opacity, noise, keys, T, ea, eb)

    def seed(self, cam, image, depth, opacity, mode, init, seed, noise=None, keys=None):
        """One keyframe.  cam: fx, fy, cx, cy, T (4x4 world-to-camera), exposure_a / b / eps.  mode 0: depth and
        opacity are the tracking render's; mode 1: neither is read; mode 2: depth is the sensor's.  `init` picks
        pcd_downsample_init.  Returns (xyz [K,3], features [K,3,(max_sh_degree+1)^2], log_scales [K,1|3], rots [K,4],
        opacity_logit [K,1], record)."""
        a, keep = self.native_args(cam, image, depth, opacity, mode, init, seed, noise, keys)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(_cabi.lib().mgs_keyframe_seed(C.byref(a), stream), "mgs_keyframe_seed")
        del keep
        r = _cabi.KeyframeSeedResult.from_buffer_copy(self.record)
        K = int(r.num_points)
        n_sh = (self.max_sh_degree + 1) ** 2
        if n_sh == 1:
            feats = self.features_dc[:K].unsqueeze(-1)
        else:
            feats = torch.zeros(K, 3, n_sh, device=self.device)
            feats[:, :, 0] = self.features_dc[:K]
        return self.xyz[:K], feats, self.log_scales[:K], self.rots[:K], self.opacity_logit[:K], r
