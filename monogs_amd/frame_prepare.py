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

Undistortion and rectification (DESIGN.md "Undistort and rectify on the device").  The reference's dataset remaps every
frame through cv2.initUndistortRectifyMap's maps when Calibration.distorted is set (utils/dataset.py:226-244,264-265),
before step 1.  Here that is a step 0 fused into the tile load of the same call (`mgs_frame_prepare_remapped`); the
contract - this repository's own, parity with cv2 is unpinned - is the docstring of `remap_build_numpy` (the map) and
of `remap_torch` (the gather), and the header's.

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


# ---- step 0: undistort and rectify ------------------------------------------------------------------------------------
MAP_CLAMP = 1 << 30
DIST_KEYS = ("k1", "k2", "p1", "p2", "k3")


def _intrinsics(K):
    """(fx, fy, cx, cy) of a 3x3 camera matrix, or of a sequence of those four."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (3, 3):
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if K.shape == (4,):
        return tuple(float(v) for v in K)
    raise ValueError(f"K is a 3x3 camera matrix or (fx, fy, cx, cy), not an array of shape {K.shape}")


def _camera_matrix(K):
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (3, 3):
        return K
    fx, fy, cx, cy = _intrinsics(K)
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def remap_inverse(K, R=None, new_K=None):
    """ir [9]: the row-major inverse of new_K @ R in double (new_K None: K; R None: the identity) - the nine numbers
    the mirror and the kernel share; the device inverts nothing."""
    M = _camera_matrix(K if new_K is None else new_K)
    if R is not None:
        M = M @ np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.linalg.inv(M).reshape(9)


def remap_build_numpy(H, W, K, dist, R=None, new_K=None, ir=None):
    """The fp64 NumPy mirror of mgs_remap_build, the map cv2.initUndistortRectifyMap + cv2.remap's fixed point stand
    for.  K: the source (distorted) camera, 3x3 or (fx, fy, cx, cy); dist = (k1, k2, p1, p2, k3), OpenCV's order; R:
    the rectifying rotation; new_K: the destination camera (None: K).  Returns (ir [9] float64, map_q5 int32 [H,W,2]).

    All arithmetic is fp64, every operation rounded on its own, in this order.  ir = inv(new_K @ R), row-major
    (`ir=` takes the nine numbers as they are).  For destination pixel (u, v):
        X = (ir0*u + ir1*v) + ir2;  Y = (ir3*u + ir4*v) + ir5;  Wd = (ir6*u + ir7*v) + ir8
        x = X / Wd;  y = Y / Wd
        x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  txy = (2*x)*y
        kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
        xd = (x*kr + p1*txy) + p2*(r2 + 2*x2)
        yd = (y*kr + p1*(r2 + 2*y2)) + p2*txy
        mx = float32(fx*xd + cx);  my = float32(fy*yd + cy)
        ix = rint_half_even(double(mx) * 32) clamped to [-2^30, 2^30];  iy likewise
    mx or my not finite: ix = iy = -2^30, so that every tap falls outside the image.  map_q5[v, u] = (ix, iy): the
    source position in 1/32-pixel fixed point."""
    fx, fy, cx, cy = _intrinsics(K)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in dist)
    ir = remap_inverse(K, R, new_K) if ir is None else np.asarray(ir, dtype=np.float64).reshape(9)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (ir[0] * u + ir[1] * v) + ir[2]
        Y = (ir[3] * u + ir[4] * v) + ir[5]
        Wd = (ir[6] * u + ir[7] * v) + ir[8]
        x, y = X / Wd, Y / Wd
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        txy = (2.0 * x) * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * txy) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * txy
        mx = (fx * xd + cx).astype(np.float32)
        my = (fy * yd + cy).astype(np.float32)
        ok = np.isfinite(mx) & np.isfinite(my)
        q = lambda m: np.clip(np.rint(np.where(ok, m, 0).astype(np.float64) * 32.0), -MAP_CLAMP, MAP_CLAMP)
        ix = np.where(ok, q(mx), -MAP_CLAMP).astype(np.int32)
        iy = np.where(ok, q(my), -MAP_CLAMP).astype(np.int32)
    return ir, np.ascontiguousarray(np.stack([ix, iy], axis=-1))


def _map_parts(map_q5, device, H, W):
    m = _as_tensor(map_q5)
    if tuple(m.shape) != (H, W, 2) or m.dtype != torch.int32:
        raise ValueError(f"the map is int32 [{H}, {W}, 2] like the image, not {m.dtype} {tuple(m.shape)}")
    m = m.to(device)
    return m[..., 0].to(torch.int64), m[..., 1].to(torch.int64)


def remap_torch(image, map_q5):
    """The gather of mgs_frame_prepare_remapped on its own: uint8 [H,W,3] -> uint8 [H,W,3], float [3,H,W] -> float32
    [3,H,W].  map_q5: int32 [H,W,2] holding (ix, iy).  sx = ix >> 5, sy = iy >> 5 (arithmetic shifts); ax = ix & 31,
    ay = iy & 31; the taps are (sy,sx), (sy,sx+1), (sy+1,sx), (sy+1,sx+1), and a tap outside [0,H) x [0,W) reads 0 in
    every channel, decided per tap (a constant border).  Integer weights w00 = (32-ax)(32-ay), w01 = ax(32-ay),
    w10 = (32-ax)ay, w11 = ax*ay (they sum to 1024).
        uint8   k = (w00*v00 + w01*v01 + w10*v10 + w11*v11 + 512) >> 10
        float   (f00*v00 + f01*v01) + (f10*v10 + f11*v11) with f = float(w) / 1024 (exact), every product and sum
                rounded on its own."""
    image = _as_tensor(image)
    u8 = image.dtype == torch.uint8
    H, W = (image.shape[0], image.shape[1]) if u8 else (image.shape[1], image.shape[2])
    if tuple(image.shape) != ((H, W, 3) if u8 else (3, H, W)):
        raise ValueError(f"image is uint8 [H,W,3] or float [3,H,W], not {tuple(image.shape)}")
    with torch.no_grad():
        ix, iy = _map_parts(map_q5, image.device, H, W)
        sx, sy, ax, ay = ix >> 5, iy >> 5, ix & 31, iy & 31
        flat = image.reshape(H * W, 3) if u8 else image.detach().to(torch.float32).reshape(3, H * W)

        def tap(dy, dx):
            yy, xx = sy + dy, sx + dx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            if u8:
                return flat[idx].to(torch.int64) * inside[..., None]
            v = flat[:, idx]
            return torch.where(inside, v, torch.zeros_like(v))

        w = ((32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay)
        v = (tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1))
        if u8:
            k = (w[0][..., None] * v[0] + w[1][..., None] * v[1] + w[2][..., None] * v[2] + w[3][..., None] * v[3]
                 + 512) >> 10
            return k.to(torch.uint8)
        f = [x.to(torch.float32) / 1024.0 for x in w]
        return ((f[0] * v[0] + f[1] * v[1]) + (f[2] * v[2] + f[3] * v[3])).contiguous()


def remap_depth_torch(depth, map_q5):
    """MGS_FRAME_REMAP_DEPTH_NEAREST: float depth [H,W] (or [1,H,W]) -> the same shape, each pixel the tap
    ((iy+16) >> 5, (ix+16) >> 5) of the source depth and 0 outside.  Not what the reference does (it remaps the image
    only): for callers who want depth and image registered."""
    depth = _as_tensor(depth)
    H, W = depth.shape[-2:]
    with torch.no_grad():
        ix, iy = _map_parts(map_q5, depth.device, H, W)
        xx, yy = (ix + 16) >> 5, (iy + 16) >> 5
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = depth.reshape(H * W)[yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)]
        return torch.where(inside, v, torch.zeros_like(v)).reshape(depth.shape)


def calibration_remap(calibration):
    """(K, dist) of a MonoGS Dataset.Calibration dict whose `distorted` is true, else None.  The reference builds its
    maps with R = I and new_K = K (utils/dataset.py:237-244)."""
    if not calibration or not calibration.get("distorted", False):
        return None
    K = tuple(float(calibration[k]) for k in ("fx", "fy", "cx", "cy"))
    return K, tuple(float(calibration.get(k, 0.0)) for k in DIST_KEYS)


def prepare_frame_torch(image, depth=None, *, dataset_type, edge_threshold, rgb_boundary_threshold=0.01,
                        depth_scale=None, remap=None, remap_depth=False):
    """The torch mirror.  image: float [3,H,W] or uint8 [H,W,3]; depth: None, float [H,W] or uint16 [H,W] (then
    `depth_scale` is needed); tensors on any device, or NumPy arrays.  `remap`: an int32 [H,W,2] map
    (remap_build_numpy's): the image goes through `remap_torch` before anything else, and with `remap_depth` the
    converted depth through `remap_depth_torch`.  Returns a dict: image [3,H,W], gt_depth [1,H,W] (None without depth),
    grad_mask / rgb_pixel_mask / rgb_pixel_mask_mapping float32 [1,H,W], intensity [H,W], median (0-dim; Replica: one
    per patch, row-major)."""
    image, depth = _as_tensor(image), _as_tensor(depth)
    if remap_depth and (remap is None or depth is None):
        raise ValueError("remap_depth needs a map and a depth")
    with torch.no_grad():
        if remap is not None:
            image = remap_torch(image, remap)
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
            if remap_depth:
                gt_depth = remap_depth_torch(gt_depth, remap)
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
    enqueued on the current stream; nothing is read back.  The inputs of a call are kept referenced until the next.

    Undistortion.  `calibration`: a MonoGS Dataset.Calibration dict (fx, fy, cx, cy, k1, k2, p1, p2, k3, distorted),
    read from config["Dataset"]["Calibration"] when not given.  With `distorted` true the preparer builds its map on
    the device once, here (mgs_remap_build, R = I and new_K = K as the reference's dataset), and every frame goes
    through mgs_frame_prepare_remapped: the frames handed in must then be RAW.  `remap`: a caller-made int32 [H,W,2]
    device tensor instead, e.g. a stereo rectification map; `build_remap` rebuilds the map.  `remap_depth`: the depth
    follows the image (MGS_FRAME_REMAP_DEPTH_NEAREST; the reference leaves the depth as it is).  A preparer with a map
    always returns its own `image` buffer - a float input is not handed back.  Without a map (no calibration, or
    `distorted` false) the preparer is the un-remapped one.  Stream order: the map is built (build_remap) or copied
    (set_remap) on the stream that is current at that moment; a `prepare` on ANOTHER stream is ordered after it only if
    the caller makes it so (torch.cuda.Stream.wait_stream, or a synchronise after construction)."""

    def __init__(self, H: int, W: int, device, config: Optional[dict] = None, *, dataset_type=None,
                 edge_threshold=None, rgb_boundary_threshold=None, keep_intensity: bool = False, calibration=None,
                 remap=None, remap_depth: bool = False):
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
        self.remap_depth = bool(remap_depth)
        self.map_q5 = self.remap_ir = None
        if remap is not None:
            self.set_remap(remap)
        else:
            cal = calibration_remap(ds.get("Calibration") if calibration is None else calibration)
            if cal is not None:
                self.build_remap(*cal)
        if self.remap_depth and self.map_q5 is None:
            raise ValueError("remap_depth needs a map: a distorted calibration or remap=")

    def set_remap(self, remap):
        """Take a caller-made map: int32 [H,W,2] holding (ix, iy) in 1/32 pixel; None: no remap (refused on a preparer
        with remap_depth, as the constructor refuses it).  A host tensor is copied on the current stream."""
        if remap is None and self.remap_depth:
            raise ValueError("remap_depth needs a map: a distorted calibration or remap=")
        if remap is not None:
            remap = _as_tensor(remap)
            if tuple(remap.shape) != (self.H, self.W, 2) or remap.dtype != torch.int32:
                raise ValueError(f"remap is int32 [{self.H}, {self.W}, 2], not {remap.dtype} {tuple(remap.shape)}")
            remap = remap.to(self.device).contiguous()
        self.map_q5, self.remap_ir = remap, None
        return remap

    def build_remap(self, K, dist, R=None, new_K=None, ir=None):
        """(Re)build the map on the device: one mgs_remap_build launch on the current stream.  Arguments as
        remap_build_numpy's; the inverse of new_K @ R is taken here, on the host, in double."""
        fx, fy, cx, cy = _intrinsics(K)
        ir = remap_inverse(K, R, new_K) if ir is None else np.asarray(ir, dtype=np.float64).reshape(9)
        m = torch.empty(self.H, self.W, 2, dtype=torch.int32, device=self.device)
        b = _cabi.RemapBuildArgs()
        b.width, b.height = self.W, self.H
        b.ir[:] = [float(v) for v in ir]
        b.fx, b.fy, b.cx, b.cy = fx, fy, cx, cy
        b.dist[:] = [float(v) for v in dist]
        b.map_q5 = m.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(_cabi.lib().mgs_remap_build(C.byref(b), stream), "mgs_remap_build")
        self.map_q5, self.remap_ir = m, ir
        return m

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
            if self.map_q5 is None:
                res["image"] = image                       # already the float image: nothing is copied
            else:
                a.image = out["image"].data_ptr()
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
                if self.remap_depth:
                    a.gt_depth = out["gt_depth"].data_ptr()
                    res["gt_depth"] = out["gt_depth"]
            a.depth_in = depth.data_ptr()
        a.grad_mask, a.rgb_pixel_mask = out["grad_mask"].data_ptr(), out["rgb_pixel_mask"].data_ptr()
        a.rgb_pixel_mask_mapping = out["rgb_pixel_mask_mapping"].data_ptr()
        a.median_out = out["median"].data_ptr()
        a.intensity_out = None if self.intensity is None else self.intensity.data_ptr()
        a.scratch = self.scratch.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if self.map_q5 is None:
            _cabi.check(_cabi.lib().mgs_frame_prepare(C.byref(a), stream), "mgs_frame_prepare")
        else:
            r = _cabi.FrameRemapArgs()
            r.map_q5 = self.map_q5.data_ptr()
            r.depth_mode = _cabi.FRAME_REMAP_DEPTH_NEAREST if self.remap_depth and depth is not None \
                else _cabi.FRAME_REMAP_DEPTH_NONE
            _cabi.check(_cabi.lib().mgs_frame_prepare_remapped(C.byref(a), C.byref(r), stream),
                        "mgs_frame_prepare_remapped")
        self._keep = (image, depth, self.map_q5)
        if self.intensity is not None:
            res["intensity"] = self.intensity
        return res

    def prepare(self, image, depth=None, depth_scale=None):
        """One frame.  image: float [3,H,W] or uint8 [H,W,3]; depth: None, float [H,W] / [1,H,W] or uint16 [H,W] with
        `depth_scale`; torch tensors (host or device) or NumPy arrays.  Returns a dict of device tensors: image
        [3,H,W] (a float input is handed back as it is, unless the preparer remaps), gt_depth [1,H,W] or None,
        grad_mask, rgb_pixel_mask, rgb_pixel_mask_mapping float32 0 / 1 [1,H,W], median ([1]; Replica: one per patch)
        and, with keep_intensity, intensity [H,W].  Views of this object's buffers: valid until its next call."""
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
