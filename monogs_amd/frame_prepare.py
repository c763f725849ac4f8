"""Frame preparation: from the frame a dataset hands over to what tracking and mapping read from a camera
(DESIGN.md "Frame preparation on the device").

The reference does this to EVERY incoming frame: the dataset converts the image from uint8 HWC to float CHW and the
depth from uint16 to metres (utils/dataset.py:269-276), Camera.compute_grad_mask (utils/camera_utils.py:110-147, with
the stencils of utils/slam_utils.py:7-41) leaves grad_mask, rgb_pixel_mask, rgb_pixel_mask_mapping and gt_depth on the
camera.  The steps:

  1. ingest     uint8 k -> float32(k / 255.0), uint16 d -> float32(d / depth_scale): double quotients, rounded once.
  2. sum, grey  s = (r + g) + b; grey = s / 3.
  3. gradient   Scharr stencils over the reflect-padded grey, times 1 / 32; a pixel whose nine padded neighbours do not
                all have |grey| > 0.01 has both gradients zeroed; intensity I = sqrt(grad_v^2 + grad_h^2).
  4. median     every dataset type but Replica: the lower median m of all H*W intensities (torch.median's element).
                Replica: per 32x32 patch (stride 32, anchored top-left) the element of rank 511 of its 1024 intensities.
  5. masks      grad_mask = I > m * edge_threshold (Replica: inside the whole patches; every pixel no whole patch covers
                gets 0, which is what the reference's fold() leaves there - the last 8 rows and 16 columns at 1200x680);
                rgb_pixel_mask_mapping = s > rgb_boundary_threshold; rgb_pixel_mask = rgb_pixel_mask_mapping * grad_mask.

Two implementations:
  * `prepare_frame_torch`: the torch mirror, on CPU or GPU tensors - the statement of the contract (pinned to the
    reference's own outputs by tests/golden/frame_prepare_ref.npz) and the baseline of the profile.
  * `FramePreparer`: one `mgs_frame_prepare` call (frame_prepare.hip) with no host read and no synchronisation.

Both return the masks as float32 0 / 1 [1,H,W], the form the loss kernels take (the reference keeps bool in one branch
and float in the other).  NaN / Inf in the image is unspecified in both.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _cabi

PATCH = _cabi.FRAME_PATCH_SIZE
VALID_EPS = 0.01          # image_gradient_mask's eps


def is_patch_mode(dataset_type) -> bool:
    """compute_grad_mask's branch: Dataset.type == "replica" takes the per-patch medians."""
    return str(dataset_type) == "replica"


def _as_tensor(x):
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint16:               # carried as int16 bit patterns where torch has no uint16 arithmetic
            return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).view(torch.uint16)
        return torch.from_numpy(np.ascontiguousarray(x))
    return x


def convert_image_torch(image):
    """uint8 [H,W,3] -> float32 [3,H,W] as the dataset does it (image / 255.0 in double, rounded once)."""
    return (image.to(torch.float64) / 255.0).to(torch.float32).permute(2, 0, 1).contiguous()


def convert_depth_torch(depth, depth_scale):
    """uint16 [H,W] -> float32 [H,W]: float32(d / depth_scale) with the quotient in double."""
    d = depth.view(torch.int16).to(torch.int32) & 0xFFFF
    return (d.to(torch.float64) / float(depth_scale)).to(torch.float32)


def _check_shape(H, W, patch):
    if H < 2 or W < 2:
        raise ValueError(f"a {H}x{W} image cannot be reflect-padded: both sides must be at least 2")
    if patch and (H < PATCH or W < PATCH):
        raise ValueError(f"a {H}x{W} image holds no whole {PATCH}x{PATCH} patch (Replica mode; the reference's unfold "
                         "raises there)")


def intensity_torch(image):
    """Steps 2 and 3 on a float image [3,H,W]: (channel sum [H,W], gradient intensity [H,W])."""
    H, W = image.shape[1:]
    s = (image[0] + image[1]) + image[2]
    grey = s / torch.full((), 3.0, device=image.device)      # a true divide on every device (a Python scalar divisor
                                                             # becomes a multiply by the rounded 1 / 3 on the GPU)
    iy = torch.tensor([1] + list(range(H)) + [H - 2], device=image.device)
    ix = torch.tensor([1] + list(range(W)) + [W - 2], device=image.device)
    gp = grey[iy][:, ix]                                         # reflect padding, one pixel

    def n(dy, dx):
        return gp[dy:dy + H, dx:dx + W]

    gv = (3 * n(0, 0) + 10 * n(0, 1) + 3 * n(0, 2) - 3 * n(2, 0) - 10 * n(2, 1) - 3 * n(2, 2)) * (1.0 / 32.0)
    gh = (3 * n(0, 0) - 3 * n(0, 2) + 10 * n(1, 0) - 10 * n(1, 2) + 3 * n(2, 0) - 3 * n(2, 2)) * (1.0 / 32.0)
    ok = gp.abs() > VALID_EPS
    valid = torch.ones(H, W, dtype=torch.bool, device=image.device)
    for dy in range(3):
        for dx in range(3):
            valid = valid & ok[dy:dy + H, dx:dx + W]
    inten = torch.sqrt(gv * gv + gh * gh)
    return s, torch.where(valid, inten, torch.zeros_like(inten))


def prepare_frame_torch(image, depth=None, *, dataset_type, edge_threshold, rgb_boundary_threshold=0.01,
                        depth_scale=None):
    """The torch mirror.  image: float [3,H,W] or uint8 [H,W,3]; depth: None, float [H,W] or uint16 [H,W] (then
    `depth_scale` is needed); tensors on any device, or NumPy arrays.  Returns a dict: image [3,H,W], gt_depth [1,H,W]
    (None without depth), grad_mask / rgb_pixel_mask / rgb_pixel_mask_mapping float32 [1,H,W], intensity [H,W], median
    (0-dim; Replica: one per patch, row-major)."""
    image, depth = _as_tensor(image), _as_tensor(depth)
    with torch.no_grad():
        if image.dtype == torch.uint8:
            image = convert_image_torch(image)
        else:
            image = image.detach().to(torch.float32)
        H, W = image.shape[1:]
        patch = is_patch_mode(dataset_type)
        _check_shape(H, W, patch)
        gt_depth = None
        if depth is not None:
            if depth.dtype in (torch.uint16, torch.int16):
                if depth_scale is None or not float(depth_scale) > 0:
                    raise ValueError("a uint16 depth needs a positive depth_scale")
                gt_depth = convert_depth_torch(depth.view(torch.int16).to(image.device), depth_scale).reshape(1, H, W)
            else:
                gt_depth = depth.detach().to(image.device, torch.float32).reshape(1, H, W)
        s, inten = intensity_torch(image)
        et = float(edge_threshold)
        if patch:
            ny, nx = H // PATCH, W // PATCH
            blocks = inten[:ny * PATCH, :nx * PATCH].reshape(ny, PATCH, nx, PATCH).permute(0, 2, 1, 3)
            med = blocks.reshape(ny * nx, PATCH * PATCH).median(dim=1).values           # rank 511 of 1024
            inside = blocks > (med * et).reshape(ny, nx, 1, 1)
            grad = torch.zeros(H, W, dtype=torch.bool, device=image.device)
            grad[:ny * PATCH, :nx * PATCH] = inside.permute(0, 2, 1, 3).reshape(ny * PATCH, nx * PATCH)
        else:
            med = inten.reshape(-1).median()
            grad = inten > med * et
        mapping = s > float(rgb_boundary_threshold)
        f = lambda m: m.to(torch.float32).reshape(1, H, W)
        return {"image": image, "gt_depth": gt_depth, "grad_mask": f(grad), "rgb_pixel_mask": f(mapping & grad),
                "rgb_pixel_mask_mapping": f(mapping), "intensity": inten, "median": med}


# ---- the native path --------------------------------------------------------------------------------------------------
OUTPUTS = ("grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping")


class FramePreparer:
    """Owns the scratch and one set of output buffers of mgs_frame_prepare for one image size.  `config`: a MonoGS config
    dict (Training.edge_threshold, Training.rgb_boundary_threshold, Dataset.type); the keyword arguments override it.
    `prepare` returns views of the preparer's own buffers: they hold until the next `prepare` on this object - a camera
    that outlives that call (every keyframe) takes `prepare_into`, which writes into tensors of its own.  Everything is
    enqueued on the current stream; nothing is read back.  The inputs of a call are kept referenced until the next."""

    def __init__(self, H: int, W: int, device, config: Optional[dict] = None, *, dataset_type=None,
                 edge_threshold=None, rgb_boundary_threshold=None, keep_intensity: bool = False):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mgs_frame_prepare runs on the GPU only (HIP kernels, gfx950)")
        tr, ds = (config or {}).get("Training") or {}, (config or {}).get("Dataset") or {}
        self.edge_threshold = float(tr.get("edge_threshold", 1.1) if edge_threshold is None else edge_threshold)
        self.rgb_boundary_threshold = float(tr.get("rgb_boundary_threshold", 0.01) if rgb_boundary_threshold is None
                                            else rgb_boundary_threshold)
        self.dataset_type = ds.get("type", "tum") if dataset_type is None else dataset_type
        self.patch = is_patch_mode(self.dataset_type)
        self.H, self.W, self.device = int(H), int(W), device
        _check_shape(self.H, self.W, self.patch)
        nbytes = int(_cabi.lib().mgs_frame_prepare_scratch_bytes(self.H, self.W))
        if nbytes == 0:
            raise ValueError(f"mgs_frame_prepare_scratch_bytes({H}, {W}) refused the size")
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.num_medians = (self.H // PATCH) * (self.W // PATCH) if self.patch else 1
        self.intensity = torch.empty(self.H, self.W, device=device) if keep_intensity else None
        self.buffers = self._new_outputs()
        self._keep = None

    def _new_outputs(self):
        H, W, dev = self.H, self.W, self.device
        out = {k: torch.empty(1, H, W, device=dev) for k in OUTPUTS}
        out["image"] = torch.empty(3, H, W, device=dev)
        out["gt_depth"] = torch.empty(1, H, W, device=dev)
        out["median"] = torch.empty(self.num_medians, device=dev)
        return out

    def _run(self, image, depth, depth_scale, out):
        H, W, dev = self.H, self.W, self.device
        image, depth = _as_tensor(image), _as_tensor(depth)
        a = _cabi.FramePrepareArgs()
        a.width, a.height = W, H
        a.mode = _cabi.FRAME_MODE_PATCH if self.patch else _cabi.FRAME_MODE_GLOBAL
        a.edge_threshold, a.rgb_boundary_threshold = self.edge_threshold, self.rgb_boundary_threshold
        res = dict(out)
        if image.dtype == torch.uint8:
            if tuple(image.shape) != (H, W, 3):
                raise ValueError(f"uint8 image is {tuple(image.shape)}, the preparer was built for ({H}, {W}, 3)")
            image = image.to(dev, non_blocking=True).contiguous()
            a.image_format, a.image = _cabi.FRAME_IMAGE_U8_HWC, out["image"].data_ptr()
        else:
            if tuple(image.shape) != (3, H, W):
                raise ValueError(f"image is {tuple(image.shape)}, the preparer was built for (3, {H}, {W})")
            image = image.detach().to(dev, torch.float32, non_blocking=True).contiguous()
            a.image_format = _cabi.FRAME_IMAGE_F32_CHW
            res["image"] = image                           # already the float image: nothing is copied
        a.image_in = image.data_ptr()
        a.depth_format = _cabi.FRAME_DEPTH_NONE
        res["gt_depth"] = None
        if depth is not None:
            if depth.numel() != H * W:
                raise ValueError(f"depth has {depth.numel()} elements, the image {H * W}")
            if depth.dtype in (torch.uint16, torch.int16):
                if depth_scale is None or not float(depth_scale) > 0:
                    raise ValueError("a uint16 depth needs a positive depth_scale")
                depth = depth.view(torch.int16).to(dev, non_blocking=True).contiguous()
                a.depth_format, a.depth_scale = _cabi.FRAME_DEPTH_U16, float(depth_scale)
                a.gt_depth = out["gt_depth"].data_ptr()
                res["gt_depth"] = out["gt_depth"]
            else:
                depth = depth.detach().to(dev, torch.float32, non_blocking=True).contiguous()
                a.depth_format = _cabi.FRAME_DEPTH_F32
                res["gt_depth"] = depth.reshape(1, H, W)
            a.depth_in = depth.data_ptr()
        a.grad_mask, a.rgb_pixel_mask = out["grad_mask"].data_ptr(), out["rgb_pixel_mask"].data_ptr()
        a.rgb_pixel_mask_mapping = out["rgb_pixel_mask_mapping"].data_ptr()
        a.median_out = out["median"].data_ptr()
        a.intensity_out = None if self.intensity is None else self.intensity.data_ptr()
        a.scratch = self.scratch.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(_cabi.lib().mgs_frame_prepare(C.byref(a), stream), "mgs_frame_prepare")
        self._keep = (image, depth)
        if self.intensity is not None:
            res["intensity"] = self.intensity
        return res

    def prepare(self, image, depth=None, depth_scale=None):
        """One frame.  image: float [3,H,W] or uint8 [H,W,3]; depth: None, float [H,W] / [1,H,W] or uint16 [H,W] with
        `depth_scale`; torch tensors (host or device) or NumPy arrays.  Returns a dict of device tensors: image
        [3,H,W] (a float input is handed back as it is), gt_depth [1,H,W] or None, grad_mask, rgb_pixel_mask,
        rgb_pixel_mask_mapping float32 0 / 1 [1,H,W], median ([1]; Replica: one per patch) and, with keep_intensity,
        intensity [H,W].  Views of this object's buffers: valid until its next call."""
        return self._run(image, depth, depth_scale, self.buffers)

    def prepare_into(self, viewpoint, image=None, depth=None, depth_scale=None):
        """What compute_grad_mask leaves on a Camera, on a ViewCamera-like `viewpoint`: original_image, grad_mask,
        rgb_pixel_mask, rgb_pixel_mask_mapping and gt_depth (when there is a depth; otherwise the attribute is left
        alone).  image None: the viewpoint's own original_image.  The tensors are the viewpoint's own (allocated here),
        so they outlive the preparer's next call.  Returns the same dict as `prepare`."""
        if image is None:
            image = viewpoint.original_image
        res = self._run(image, depth, depth_scale, self._new_outputs())
        viewpoint.original_image = res["image"]
        for k in OUTPUTS:
            setattr(viewpoint, k, res[k])
        if res["gt_depth"] is not None:
            viewpoint.gt_depth = res["gt_depth"]
        return res
