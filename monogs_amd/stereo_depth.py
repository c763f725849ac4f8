"""Stereo depth: from a stereo pair to the depth map the frontend treats as sensor depth (DESIGN.md "Stereo depth on
the device").

The reference's StereoDataset.__getitem__ (utils/dataset.py:367-395) does this to EVERY frame of a `sensor_type:
'stereo'` run (configs/stereo/euroc/*) on the host: cv2.remap of both images, cv2.StereoSGBM_create(minDisparity=0,
numDisparities=64, blockSize=20) with setUniquenessRatio(40), depth = 47.90639384423901 / disparity; that depth then
plays the RGB-D sensor depth's role (keyframe seeding, the RGB-D mapping loss).

Two implementations of one contract (include/monogs_raster.h "stereo depth"; the docstring of `stereo_sgbm_numpy`):
  * `stereo_sgbm_numpy`: the NumPy mirror, for any number of disparities - the statement of the contract.
  * `StereoMatcher`: one `mgs_stereo_depth` call (stereo_depth.hip, D = 64) with no host read and no synchronisation.
Every step is integer arithmetic and one correctly rounded double division: the two agree bit for bit.

The algorithm restates OpenCV's single-pass MODE_SGBM, with the parameters the reference passes and OpenCV's defaults
for the rest, from knowledge of that algorithm.  Parity with cv2.StereoSGBM itself is UNPINNED: there is no cv2 to make
a fixture with.  The accuracy of the depth on real EuRoC imagery is unchecked as well (no dataset).

Grey.  The matcher works on rectified grey uint8 images.  `to_grey_numpy` states how an input becomes one, an
approximation of what cv2.imread(path, 0) hands the reference:
  uint8 [H,W]      the byte itself (EuRoC's PNGs are grey: this is the exact case);
  uint8 [H,W,3]    RGB order, (4899*r + 9617*g + 1868*b + 8192) >> 14 - OpenCV's fixed-point grey (equal channels give
                   the channel itself);
  float [3,H,W]    each channel to clamp(rint_half_even(float32(v) * 255 in fp32), 0, 255), NaN to 0, then as above.
With a rectification map every channel is first gathered as frame_prepare.remap_torch states (uint8: the rounded integer
blend (.. + 512) >> 10, a byte again; float: the fp32 blend; constant 0 border), then reduced to grey.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _cabi
from .frame_prepare import DIST_KEYS, _as_tensor, _intrinsics, remap_inverse

BF_REFERENCE = 47.90639384423901       # utils/dataset.py:382, "following ORB-SLAM2 config, baseline*fx"
NUM_DISPARITIES = 64
BLOCK_SIZE = 20
UNIQUENESS_RATIO = 40
P1, P2 = 2, 5                          # OpenCV's substitutes for StereoSGBM_create's defaults P1 = P2 = 0
FTZERO = 15                            # preFilterCap
_BIG = 1 << 28


# ---- the NumPy mirror ---------------------------------------------------------------------------------------------------
def to_grey_numpy(image) -> np.ndarray:
    """uint8 [H,W], uint8 [H,W,3] (RGB) or float [3,H,W] -> uint8 [H,W] by the module docstring's rule."""
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu().numpy()
    image = np.asarray(image)
    if image.dtype == np.uint8 and image.ndim == 2:
        return np.ascontiguousarray(image)
    if image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3:
        k = image.astype(np.int64)
    elif image.ndim == 3 and image.shape[0] == 3 and image.dtype.kind == "f":
        v = image.astype(np.float32) * np.float32(255.0)
        with np.errstate(invalid="ignore"):
            k = np.clip(np.where(np.isnan(v), np.float32(0), np.rint(v)), 0, 255).astype(np.int64).transpose(1, 2, 0)
    else:
        raise ValueError(f"an image is uint8 [H,W], uint8 [H,W,3] or float [3,H,W], not {image.dtype} {image.shape}")
    return ((4899 * k[..., 0] + 9617 * k[..., 1] + 1868 * k[..., 2] + 8192) >> 14).astype(np.uint8)


def prefilter_numpy(I) -> np.ndarray:
    """The clipped horizontal Sobel response g, int32 [H,W] in 0..30 (rows clamped; 15 in the first and last column)."""
    I = np.asarray(I).astype(np.int32)
    H, W = I.shape
    up, dn = I[np.maximum(np.arange(H) - 1, 0)], I[np.minimum(np.arange(H) + 1, H - 1)]

    def dx(A):
        o = np.zeros_like(A)
        o[:, 1:-1] = A[:, 2:] - A[:, :-2]
        return o

    g = np.clip(2 * dx(I) + dx(up) + dx(dn), -FTZERO, FTZERO) + FTZERO
    g[:, 0] = FTZERO
    g[:, -1] = FTZERO
    return g


def _bt_bounds(A):
    W = A.shape[1]
    lf, rt = A[:, np.maximum(np.arange(W) - 1, 0)], A[:, np.minimum(np.arange(W) + 1, W - 1)]
    al, ar = (A + lf) // 2, (A + rt) // 2
    return np.minimum(np.minimum(al, ar), A), np.maximum(np.maximum(al, ar), A)


def pixel_cost_numpy(L, R, D=NUM_DISPARITIES) -> np.ndarray:
    """Birchfield-Tomasi on the two channels g and I: int32 [H,W,D], zero in the columns x < D."""
    L, R = np.asarray(L), np.asarray(R)
    H, W = L.shape
    out = np.zeros((H, W, D), np.int32)
    xs = np.arange(D, W)
    for a, b in ((prefilter_numpy(L), prefilter_numpy(R)), (L.astype(np.int32), R.astype(np.int32))):
        u0, u1 = _bt_bounds(a)
        v0, v1 = _bt_bounds(b)
        for d in range(D):
            u, v = a[:, xs], b[:, xs - d]
            c0 = np.maximum(0, np.maximum(u - v1[:, xs - d], v0[:, xs - d] - u))
            c1 = np.maximum(0, np.maximum(v - u1[:, xs], u0[:, xs] - v))
            out[:, D:, d] += np.minimum(c0, c1) >> 2
    return out


def block_cost_numpy(pc, r=BLOCK_SIZE // 2) -> np.ndarray:
    """C: the pixel cost summed over |dx| <= r, |dy| <= r, y clamped to [0,H-1] and x to [D,W-1]; int32 [H,W,D]."""
    H, W, D = pc.shape
    ys = np.clip(np.arange(-r, H + r), 0, H - 1)
    xs = np.clip(np.arange(D - r, W + r), D, W - 1)
    p = pc[ys][:, xs].astype(np.int64)
    cs = np.cumsum(np.concatenate([np.zeros((1,) + p.shape[1:], np.int64), p]), 0)
    v = cs[2 * r + 1:] - cs[:-(2 * r + 1)]
    cs = np.cumsum(np.concatenate([np.zeros((v.shape[0], 1, D), np.int64), v], 1), 1)
    C_ = np.zeros((H, W, D), np.int32)
    C_[:, D:] = cs[:, 2 * r + 1:] - cs[:, :-(2 * r + 1)]
    return C_


def path_step_numpy(Lq, Cp) -> np.ndarray:
    """L(p,.) from the predecessor's L(q,.) [...,D] and C(p,.)."""
    m = Lq.min(-1, keepdims=True)
    lo = np.concatenate([np.full_like(m, _BIG), Lq[..., :-1]], -1) + P1
    hi = np.concatenate([Lq[..., 1:], np.full_like(m, _BIG)], -1) + P1
    return Cp + np.minimum(np.minimum(Lq, lo), np.minimum(hi, m + P2)) - m


def aggregate_numpy(C_) -> np.ndarray:
    """S: the sum of the five paths' L; int32 [H,W,D], zero in the columns x < D."""
    H, W, D = C_.shape
    S = np.zeros_like(C_)
    for rev in (False, True):                                   # predecessors (x-1, y) and (x+1, y)
        L = np.zeros_like(C_)
        prev = None
        for x in (range(W - 1, D - 1, -1) if rev else range(D, W)):
            L[:, x] = C_[:, x] if prev is None else path_step_numpy(L[:, prev], C_[:, x])
            prev = x
        S += L
    xs = np.arange(D, W)
    for dx in (-1, 0, 1):                                       # predecessors (x+dx, y-1)
        L = np.zeros_like(C_)
        L[0] = C_[0]
        for y in range(1, H):
            q = xs + dx
            ok = (q >= D) & (q < W)
            new = path_step_numpy(L[y - 1][np.clip(q, D, W - 1)], C_[y, xs])
            new[~ok] = C_[y, xs][~ok]
            L[y, xs] = new
        S += L
    return S


def select_numpy(S, uniqueness_ratio=UNIQUENESS_RATIO, return_flags=False):
    """disp16 int16 [H,W] from S: argmin, uniqueness, sub-pixel and the left-right check.  `return_flags`: also the bool
    maps (not_unique, failed_left_right) over [H,W]."""
    H, W, D = S.shape
    Sv = S[:, D:].astype(np.int64)
    d = np.arange(D)
    b = Sv.argmin(-1)                                            # the first minimum: the smallest d on ties
    sb = np.take_along_axis(Sv, b[..., None], -1)[..., 0]
    far = np.abs(d - b[..., None]) > 1
    not_unique = (far & (Sv * (100 - int(uniqueness_ratio)) < sb[..., None] * 100)).any(-1)
    sm = np.take_along_axis(Sv, np.maximum(b - 1, 0)[..., None], -1)[..., 0]
    sp = np.take_along_axis(Sv, np.minimum(b + 1, D - 1)[..., None], -1)[..., 0]
    den = np.maximum(sm + sp - 2 * sb, 1)
    num = (sm - sp) * 16 + den
    q = np.sign(num) * (np.abs(num) // (2 * den))                # C division: toward zero
    dv = np.where((b > 0) & (b < D - 1), 16 * b + q, 16 * b)
    dv = np.where(not_unique, -16, dv)
    # votes: (S[b], b) into x2 = x - b; the smallest S wins, on ties the smallest b
    no_vote = np.iinfo(np.int64).max
    vote = np.full(H * W, no_vote, np.int64)
    yy, xx = np.nonzero(~not_unique)
    bb = b[yy, xx]
    np.minimum.at(vote, yy * W + (xx + D - bb), sb[yy, xx] * D + bb)
    vote = vote.reshape(H, W)
    x = np.arange(D, W)[None, :]
    rows = np.arange(H)[:, None]

    def disagrees(cand):
        xc = x - cand
        inside = (xc >= 0) & (xc < W)
        v = vote[rows, np.clip(xc, 0, W - 1)]
        return inside & (v != no_vote) & (v % D != cand)

    failed = (dv >= 0) & disagrees(dv >> 4) & disagrees((dv + 15) >> 4)
    dv = np.where(failed, -16, dv)
    disp = np.full((H, W), -16, np.int16)
    disp[:, D:] = dv
    if not return_flags:
        return disp
    flags = [np.zeros((H, W), bool) for _ in range(2)]
    flags[0][:, D:], flags[1][:, D:] = not_unique, failed
    return disp, flags[0], flags[1]


def depth_numpy(disp16, bf=BF_REFERENCE) -> np.ndarray:
    """The reference's lines 380-385: disparity 0 -> 1e10, depth = float32(bf / disparity), negative depth -> 0."""
    disp = np.asarray(disp16).astype(np.float64) / 16.0
    disp[disp == 0] = 1e10
    depth = (np.float64(bf) / disp).astype(np.float32)
    depth[depth < 0] = 0
    return depth


def stereo_sgbm_numpy(left_u8, right_u8, *, numDisparities=NUM_DISPARITIES, blockSize=BLOCK_SIZE,
                      uniquenessRatio=UNIQUENESS_RATIO, bf=BF_REFERENCE, return_flags=False):
    """The mirror: rectified grey uint8 L, R [H,W] with W > D -> (disp16 int16 [H,W], depth float32 [H,W]).

    D = numDisparities disparities d = 0..D-1, minDisparity 0; half block r = blockSize // 2 (a 21x21 window at 20);
    P1 = 2, P2 = 5 (OpenCV's substitutes for 0, 0); ftzero = 15; disp12MaxDiff = 0; valid columns x in [D, W).
      prefilter   g = clip(2(I[y,x+1]-I[y,x-1]) + (I[y-1,x+1]-I[y-1,x-1]) + (I[y+1,x+1]-I[y+1,x-1]), -15, 15) + 15; rows
                  clamped at the border; g = 15 in the first and the last column.
      pixel cost  Birchfield-Tomasi on g and on the raw intensity.  For u at x (neighbours clamped): ul = (u+u[x-1])//2,
                  ur = (u+u[x+1])//2, u0 = min(u,ul,ur), u1 = max(u,ul,ur); likewise for v = R[x-d];
                  c = min(max(0, u-v1, v0-u), max(0, v-u1, u0-v)) >> 2; the cost is the sum over the two channels (<= 70).
      block cost  C(x,y,d): the pixel cost over |dx| <= r, |dy| <= r, y clamped to [0,H-1], x to [D,W-1]
                  (<= (2r+1)^2 * 70: 30 870 at blockSize 20, 58 870 at 29, the largest the device takes).
      paths       five: the predecessor q of p = (x,y) is (x-1,y), (x+1,y), (x-1,y-1), (x,y-1) or (x+1,y-1);
                  L(p,d) = C(p,d) + min(L(q,d), L(q,d-1)+P1, L(q,d+1)+P1, m_q+P2) - m_q with m_q = min_d L(q,d) and
                  d-1 / d+1 outside 0..D-1 left out; q outside the valid region: L(p,.) = C(p,.).  S = their sum.
      selection   b = argmin_d S, the smallest d on ties; not unique (invalid) if some d with |d-b| > 1 has
                  S[d]*(100-uniquenessRatio) < S[b]*100; 0 < b < D-1: den = max(S[b-1]+S[b+1]-2S[b], 1),
                  disp16 = 16b + ((S[b-1]-S[b+1])*16 + den) / (2 den), C division; b at either end: 16b.  Invalid
                  pixels and all of x < D hold -16.
      left-right  every unique pixel votes (S[b], b) into x2 = x-b; a column keeps the smallest S, on ties the smallest
                  b (OpenCV's first-come rule: at a fixed x2 a smaller x means a smaller b).  A valid pixel with
                  d1 = disp16 is invalidated if both candidates d1 >> 4 and (d1+15) >> 4 disagree; a candidate c
                  disagrees when x-c is inside the row, holds a vote, and the vote's b differs from c.
      depth       `depth_numpy`: the reference's lines to the letter - invalid pixels and the left D columns get 0, a
                  disparity of exactly 0 gets bf / 1e10.
    `return_flags`: also the bool maps (not_unique, failed_left_right)."""
    L, R = np.asarray(left_u8), np.asarray(right_u8)
    D, r = int(numDisparities), int(blockSize) // 2
    if L.dtype != np.uint8 or R.dtype != np.uint8 or L.ndim != 2 or L.shape != R.shape:
        raise ValueError("left and right are uint8 [H,W] images of one shape")
    if D < 1 or L.shape[1] <= D:
        raise ValueError(f"a {L.shape[1]}-column image has no valid column at {D} disparities")
    S = aggregate_numpy(block_cost_numpy(pixel_cost_numpy(L, R, D), r))
    out = select_numpy(S, uniquenessRatio, return_flags)
    disp = out[0] if return_flags else out
    depth = depth_numpy(disp, bf)
    return (disp, depth) + tuple(out[1:]) if return_flags else (disp, depth)


# ---- the native path --------------------------------------------------------------------------------------------------
def stereo_calibration_remaps(calibration):
    """((K, dist, R, new_K) of cam0, the same of cam1) of a MonoGS stereo Dataset.Calibration dict (cam0 / cam1 with
    raw, opt, R; `distorted`) - per camera K = raw, dist = raw k1..k3, R = cam.R, new_K = opt, what the reference hands
    cv2.initUndistortRectifyMap (utils/dataset.py:346-365) - or None when `distorted` is false."""
    if not calibration or not calibration.get("distorted", False):
        return None
    out = []
    for name in ("cam0", "cam1"):
        cam = calibration[name]
        raw, opt, R = cam["raw"], cam["opt"], cam["R"]
        R = np.asarray(R["data"] if isinstance(R, dict) else R, dtype=np.float64).reshape(3, 3)
        out.append((tuple(float(raw[k]) for k in ("fx", "fy", "cx", "cy")),
                    tuple(float(raw.get(k, 0.0)) for k in DIST_KEYS), R,
                    tuple(float(opt[k]) for k in ("fx", "fy", "cx", "cy"))))
    return tuple(out)


class StereoMatcher:
    """Owns the scratch, the outputs and up to two rectification maps of mgs_stereo_depth for one image size.
    `config`: a MonoGS config dict; its Dataset.Calibration is read when `calibration` is not given.  With a stereo
    calibration whose `distorted` is true both maps are built on the device once, here (mgs_remap_build), and the pairs
    handed in must be RAW; `remap_left` / `remap_right` take caller-made int32 [H,W,2] maps instead.  `bf`: baseline *
    fx (None: the reference's constant).  numDisparities must be 64 on the device.  Everything is enqueued on the
    current stream, nothing is read back; a map is built or copied on the stream current at construction."""

    def __init__(self, H: int, W: int, device, config: Optional[dict] = None, *, calibration=None, bf=None,
                 remap_left=None, remap_right=None, numDisparities=NUM_DISPARITIES, blockSize=BLOCK_SIZE,
                 uniquenessRatio=UNIQUENESS_RATIO):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mgs_stereo_depth runs on the GPU only (HIP kernels, gfx950)")
        self.H, self.W, self.device = int(H), int(W), device
        self.bf = BF_REFERENCE if bf is None else float(bf)
        self.num_disparities, self.block_size = int(numDisparities), int(blockSize)
        self.uniqueness_ratio = int(uniquenessRatio)
        if self.num_disparities != _cabi.STEREO_DISPARITIES:
            raise ValueError(f"the kernels hold one pixel's disparities in one wave: numDisparities is "
                             f"{_cabi.STEREO_DISPARITIES}, not {numDisparities} (the NumPy mirror takes any)")
        nbytes = int(_cabi.lib().mgs_stereo_scratch_bytes(self.H, self.W))
        if nbytes == 0:
            raise ValueError(f"mgs_stereo_scratch_bytes({H}, {W}) refused the size (W must exceed 64)")
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.buffers = self._new_outputs()
        self._keep = None
        self.map_left = self._take_map(remap_left)
        self.map_right = self._take_map(remap_right)
        if remap_left is None and remap_right is None:
            ds = (config or {}).get("Dataset") or {}
            cal = stereo_calibration_remaps(ds.get("Calibration") if calibration is None else calibration)
            if cal is not None:
                self.map_left, self.map_right = (self.build_remap(*c) for c in cal)

    def _take_map(self, remap):
        if remap is None:
            return None
        remap = _as_tensor(remap)
        if tuple(remap.shape) != (self.H, self.W, 2) or remap.dtype != torch.int32:
            raise ValueError(f"a map is int32 [{self.H}, {self.W}, 2], not {remap.dtype} {tuple(remap.shape)}")
        return remap.to(self.device).contiguous()

    def build_remap(self, K, dist, R=None, new_K=None):
        """One mgs_remap_build launch on the current stream (arguments as frame_prepare.remap_build_numpy's); returns
        the int32 [H,W,2] device map."""
        fx, fy, cx, cy = _intrinsics(K)
        m = torch.empty(self.H, self.W, 2, dtype=torch.int32, device=self.device)
        b = _cabi.RemapBuildArgs()
        b.width, b.height = self.W, self.H
        b.ir[:] = [float(v) for v in remap_inverse(K, R, new_K)]
        b.fx, b.fy, b.cx, b.cy = fx, fy, cx, cy
        b.dist[:] = [float(v) for v in dist]
        b.map_q5 = m.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(_cabi.lib().mgs_remap_build(C.byref(b), stream), "mgs_remap_build")
        return m

    def _new_outputs(self):
        H, W, dev = self.H, self.W, self.device
        return {"depth": torch.empty(1, H, W, device=dev), "disp16": torch.empty(H, W, dtype=torch.int16, device=dev),
                "image": torch.empty(3, H, W, device=dev)}

    def _ingest(self, image, name):
        H, W = self.H, self.W
        image = _as_tensor(image)
        if image.dtype == torch.uint8 and tuple(image.shape) == (H, W):
            fmt = _cabi.STEREO_IMAGE_U8_GREY
        elif image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3):
            fmt = _cabi.STEREO_IMAGE_U8_HWC
        elif image.is_floating_point() and tuple(image.shape) == (3, H, W):
            fmt = _cabi.STEREO_IMAGE_F32_CHW
            image = image.detach().to(torch.float32)
        else:
            raise ValueError(f"the {name} image is uint8 [{H},{W}], uint8 [{H},{W},3] or float [3,{H},{W}], not "
                             f"{image.dtype} {tuple(image.shape)}")
        return image.to(self.device, non_blocking=True).contiguous(), fmt

    def _run(self, left, right, out):
        left, fl = self._ingest(left, "left")
        right, fr = self._ingest(right, "right")
        if fl != fr:
            raise ValueError("the left and the right image must have one format")
        a = _cabi.StereoDepthArgs()
        a.width, a.height, a.image_format = self.W, self.H, fl
        a.num_disparities, a.block_size = self.num_disparities, self.block_size
        a.uniqueness_ratio, a.bf = self.uniqueness_ratio, self.bf
        a.left_in, a.right_in = left.data_ptr(), right.data_ptr()
        a.map_left = None if self.map_left is None else self.map_left.data_ptr()
        a.map_right = None if self.map_right is None else self.map_right.data_ptr()
        a.depth, a.disp16, a.image = out["depth"].data_ptr(), out["disp16"].data_ptr(), out["image"].data_ptr()
        a.scratch = self.scratch.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _cabi.check(_cabi.lib().mgs_stereo_depth(C.byref(a), stream), "mgs_stereo_depth")
        self._keep = (left, right)
        return dict(out)

    def compute(self, left, right):
        """One pair: uint8 [H,W], uint8 [H,W,3] or float [3,H,W], both of one format; torch tensors (host or device) or
        NumPy arrays.  Returns dict(depth [1,H,W] float32, disp16 [H,W] int16, image [3,H,W] float32 - the rectified left
        grey in three channels, / 255, as the reference's cvtColor and / 255.0).  Views of this object's buffers: valid
        until its next call."""
        return self._run(left, right, self.buffers)

    def compute_into(self, viewpoint, left, right):
        """Sets `viewpoint.original_image` to the rectified left image and returns the depth [1,H,W], both tensors of
        the viewpoint's own (allocated here): the image and depth for FramePreparer.prepare_into(viewpoint, image,
        depth), which makes the edge mask, the pixel masks and gt_depth - none of that is done here."""
        res = self._run(left, right, self._new_outputs())
        viewpoint.original_image = res["image"]
        return res["depth"]
