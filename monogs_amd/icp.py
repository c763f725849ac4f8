"""Frame-to-model ICP: point-to-plane alignment of a sensor depth frame against a model view - the ray cast of a TSDF
volume, or the viewer's surface planes (csrc/icp.hip; the contract is in include/monogs_raster.h and DESIGN.md
"Frame-to-model ICP").  With integrate and ray cast this closes KinectFusion's loop: integrate, ray cast, align.

    res = vol.track(depth, T_prev, camera, z_far=4.0)       # ray cast at T_prev, then align: all on the device
    camera.T.copy_(res["T_w2c"])                             # fp32 [4,4]; res["status"] says whether to trust it
    res = align(planes, depth, view, T_model, T_init=T_guess, levels=((2, 5), (1, 10)))

    res = vol.track(depth, T_prev, camera, image=camera.original_image, photo_weight=1.0)   # RGB-D: also the colour

RGB-D alignment (the header's "RGB-D alignment"): with an image and photo_weight = lambda > 0 every pixel that projects into
the model view also adds the photometric row lambda [J_I, r_I], r_I = I_model(pi(D p)) - I_sensor(u), into the same sums -
on a textured plane the three directions [n ; p x n] cannot see.  `intensity_planes` forms luma and gradient once per call.
Without both arguments every call is the call it was.

The whole schedule of levels and iterations is enqueued at once; a level that has converged lets its remaining launches
return at once, a failure status ends everything, nothing is read by the host in between.

The mirrors `intensity_planes_torch`, `icp_rows_numpy`, `icp_solve_numpy` and `align_numpy` ARE the contract: fp32 NumPy for the rows (every
product, sum and quotient one rounding), Python floats for the fp64 solve and update (one rounding per operation), int64
for the sums.  The device equals them bit for bit.  They need no GPU.  There is no CPU fall-back behind `align`."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _cabi
from ._device import stream_ptr
from .mesh_render import view_tuple

LEVELS = ((4, 4), (2, 5), (1, 10))      # (pixel stride, iterations): KinectFusion's counts, coarse to fine
ITERATING, CONVERGED, MAX_ITERATIONS, TOO_FEW, DEGENERATE, STEP_TOO_LARGE = range(6)
STATUS_NAMES = ("iterating", "converged", "max iterations", "too few", "degenerate", "step too large")
COUNT_NAMES = ("accepted", "invalid", "range", "outside", "no_model", "distance", "normal")
MAX_PIXELS = _cabi.ICP_MAX_PIXELS
ROWS_LANES = _cabi.ICP_ROWS_BLOCKS * 256      # the lanes of the persistent grid: a level with more stride-grid tiles than
ROWS_TILES = ROWS_LANES // 64                 # ROWS_TILES makes more than one trip
INDEX_LIMIT = float(2 ** 23)
RANGE = 16.0
MAX_DIST = 8.0
FIXED = float(2 ** 30)
MAX_STEP2 = 0.25
EXP_TERMS = _cabi.ICP_EXP_TERMS
# 1 / (2k+1)!, 1 / (2k+2)!, 1 / (2k+3)!: ONE division each, of factorials that are exact in fp64
COEF_A = tuple(1.0 / float(math.factorial(2 * k + 1)) for k in range(EXP_TERMS))
COEF_B = tuple(1.0 / float(math.factorial(2 * k + 2)) for k in range(EXP_TERMS))
COEF_C = tuple(1.0 / float(math.factorial(2 * k + 3)) for k in range(EXP_TERMS))
_REC_COUNTS, _REC_X, _REC_PIVOTS, _REC_STATUS, _REC_LEVEL, _REC_ITER, _REC_RUN, _REC_DONE = 28, 35, 41, 47, 48, 49, 50, 51
# RGB-D alignment (the header's "RGB-D alignment"): the record's words 52 .. 55, the marks of the intensity planes
PHOTO_NAMES = ("accepted", "invalid", "bound")
_REC_PHOTO = 52
PHOTO_WEIGHT_MAX = _cabi.ICP_PHOTO_WEIGHT_MAX
PHOTO_BOUND = 16.0
NO_INTENSITY, NO_GRADIENT = -1.0, 2.0
LUMA = (0.299, 0.587, 0.114)


def status_ok(status) -> bool:
    """Whether a final status leaves a pose to use: converged, or out of iterations without a failure."""
    return int(status) in (CONVERGED, MAX_ITERATIONS)


def tri(i: int, j: int) -> int:
    """The index of the product (i, j), i <= j, among the 28 of the upper triangle of [J r]^T [J r], row-major."""
    return i * 7 - i * (i - 1) // 2 + (j - i)


# ---- arguments --------------------------------------------------------------------------------------------------------
def _np(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _intrinsics(view):
    """(fx, fy, cx, cy) of (fx, fy, cx, cy), of a view tuple or of a camera object."""
    if isinstance(view, (tuple, list)) and len(view) == 4:
        return tuple(float(v) for v in view)
    return view_tuple(view)[1:5]


def check_levels(levels):
    """((stride, iterations), ...) as ints, or ValueError."""
    try:
        lv = tuple((int(s), int(n)) for s, n in levels)
        same = all(float(s) == int(s) and float(n) == int(n) for s, n in levels)
    except (TypeError, ValueError):
        raise ValueError(f"icp: levels must be ((stride, iterations), ...), got {levels!r}") from None
    if not same or not 1 <= len(lv) <= _cabi.ICP_MAX_LEVELS or any(s < 1 or n < 1 for s, n in lv):
        raise ValueError(f"icp: levels must be 1 .. {_cabi.ICP_MAX_LEVELS} pairs of a stride >= 1 and an iteration count >= 1, got {levels!r}")
    if sum(n for _, n in lv) > _cabi.ICP_MAX_ITERATIONS_TOTAL:
        raise ValueError(f"icp: more than {_cabi.ICP_MAX_ITERATIONS_TOTAL} iterations in {levels!r}")
    return lv


def check_params(dist, cos_min, depth_max, min_pixels, min_pivot_ratio, damping, converged):
    if not 0.0 <= float(depth_max) <= RANGE:
        raise ValueError(f"icp: depth_max {depth_max} must lie in [0, 16]: the fixed-point sums are bounded for |p| < 16")
    if not 0.0 <= float(dist) <= MAX_DIST:
        raise ValueError(f"icp: dist {dist} must lie in [0, 8]")
    if not -1.0 <= float(cos_min) <= 1.0:
        raise ValueError(f"icp: cos_min {cos_min} must lie in [-1, 1]")
    if int(min_pixels) < 0 or not 0.0 <= float(min_pivot_ratio) <= 1.0 or not float(damping) >= 0.0 or not float(converged) >= 0.0 \
            or math.isinf(float(damping)) or math.isinf(float(converged)):
        raise ValueError("icp: min_pixels, damping and converged must be >= 0 and finite, min_pivot_ratio in [0, 1]")


def _model_layout(model, what="icp"):
    """(Hm, Wm, chw) of dict(depth [Hm,Wm], normal [Hm,Wm,3] or [3,Hm,Wm]), or ValueError."""
    try:
        d, n = model["depth"], model["normal"]
    except (KeyError, TypeError):
        raise ValueError(f"{what}: the model is a ray cast's dict, or dict(depth=, normal=)") from None
    ds = tuple(int(v) for v in d.shape)
    if len(ds) == 3 and ds[0] == 1:
        ds = ds[1:]
    if len(ds) != 2 or ds[0] < 1 or ds[1] < 1:
        raise ValueError(f"{what}: the model depth must be a plane [H,W], got {tuple(d.shape)}")
    ns = tuple(int(v) for v in n.shape)
    if ns == ds + (3,):
        return ds[0], ds[1], False
    if ns == (3,) + ds:
        return ds[0], ds[1], True
    raise ValueError(f"{what}: the model normal must be [H,W,3] or [3,H,W] for the depth plane {ds}, got {ns}")


def _sensor_shape(depth, what="icp"):
    s = tuple(int(v) for v in depth.shape)
    if len(s) == 3 and s[0] == 1:
        s = s[1:]
    if len(s) != 2 or s[0] < 1 or s[1] < 1:
        raise ValueError(f"{what}: the sensor depth must be a plane [H,W], got {tuple(depth.shape)}")
    if s[0] * s[1] > MAX_PIXELS:
        raise ValueError(f"{what}: {s[0]} x {s[1]} pixels exceed 2^22, the bound that keeps the int64 sums below 2^62")
    return s


def check_photo_weight(photo_weight) -> float:
    w = float(photo_weight)
    if not 0.0 <= w <= PHOTO_WEIGHT_MAX:          # false for a NaN
        raise ValueError(f"icp: photo_weight {photo_weight} must lie in [0, {PHOTO_WEIGHT_MAX:g}]")
    return w


def _rgb_layout(image, hw=None, what="icp"):
    """(H, W, chw) of an RGB plane [H,W,3] (the ray cast's colour) or [3,H,W] (a camera's image) - against the plane size
    `hw` where one is given; (3, W, 3) without one counts as [3,H,W]."""
    s = tuple(int(v) for v in image.shape)
    if len(s) == 3 and (hw is None or s == (3,) + tuple(hw)) and s[0] == 3 and s[1] >= 1 and s[2] >= 1:
        return s[1], s[2], True
    if len(s) == 3 and (hw is None or s == tuple(hw) + (3,)) and s[2] == 3 and s[0] >= 1 and s[1] >= 1:
        return s[0], s[1], False
    raise ValueError(f"{what}: an RGB plane must be [H,W,3] or [3,H,W]" + (f" for the plane {tuple(hw)}" if hw else "") + f", got {s}")


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def intensity_planes_torch(image, valid=None) -> torch.Tensor:
    """k_icp_intensity in fp32 on the CPU: [3,H,W] = (I, gx, gy) of an RGB plane [H,W,3] or [3,H,W].  A pixel is valid iff
    every channel lies in [0, 1] (false for NaN and inf) and `valid` [H,W] (None: all on; bool, or fp32 that is on where
    > 0) is on; I = (0.299 R + 0.587 G) + 0.114 B; gx = 0.5 (I[y,x+1] - I[y,x-1]) iff both of those pixels are valid, gy
    alike, so the border has no gradient.  An invalid I is NO_INTENSITY = -1, an invalid gradient NO_GRADIENT = 2."""
    f = np.float32
    H, W, chw = _rgb_layout(image, None, "intensity_planes_torch")
    rgb = _np(image, f)
    r, g, b = (rgb[c] if chw else rgb[..., c] for c in range(3))
    with np.errstate(all="ignore"):
        ok = (r >= 0) & (r <= 1) & (g >= 0) & (g <= 1) & (b >= 0) & (b <= 1)
        if valid is not None:
            v = _np(valid, f).reshape(-1)
            if v.size != H * W:
                raise ValueError(f"intensity_planes_torch: valid must be [{H},{W}]")
            ok &= v.reshape(H, W) > 0
        I = np.where(ok, (f(LUMA[0]) * r + f(LUMA[1]) * g) + f(LUMA[2]) * b, f(NO_INTENSITY)).astype(f)
        out = np.full((3, H, W), f(NO_GRADIENT), f)
        out[0] = I
        if W > 2:
            out[1][:, 1:-1] = np.where(ok[:, 2:] & ok[:, :-2], f(0.5) * (I[:, 2:] - I[:, :-2]), f(NO_GRADIENT))
        if H > 2:
            out[2][1:-1, :] = np.where(ok[2:, :] & ok[:-2, :], f(0.5) * (I[2:, :] - I[:-2, :]), f(NO_GRADIENT))
    return torch.from_numpy(out)


def icp_rows_numpy(model, depth, sensor_normal, D, view, model_view=None, stride=1, dist=0.1, cos_min=0.8, depth_max=10.0,
                   photo=None):
    """With photo = dict(sensor= [3,H,W], model= [3,Hm,Wm] (intensity planes), weight= lambda) this is k_icp_rows_rgbd and
    returns (sums, counts, extra): `sums` then holds both rows' products and `extra` int64 [4] is the record's words 52 ..
    55 - PHOTO_NAMES' counts and the fixed-point sum of r_I^2.  Without it, k_icp_rows in fp32 NumPy: (sums int64 [28], counts int64 [7]) over the pixels of the stride grid.  `sums` is the
    upper triangle of sum [J r]^T [J r] in fixed point (trunc(v 2^30) of each fp32 product), `counts` is COUNT_NAMES.
    `sensor_normal` [3,H,W] is surface.depth_normal_torch(depth, ..., pixel_center=0); D [3,4] fp64 takes sensor-camera to
    model-camera coordinates; `view` / `model_view` give the intrinsics ((fx, fy, cx, cy), a view tuple or a camera)."""
    f = np.float32
    H, W = _sensor_shape(depth, "icp_rows_numpy")
    Hm, Wm, chw = _model_layout(model, "icp_rows_numpy")
    check_params(dist, cos_min, depth_max, 0, 0.0, 0.0, 0.0)
    stride = int(stride)
    if stride < 1:
        raise ValueError("icp_rows_numpy: stride must be >= 1")
    fx, fy, cx, cy = (f(v) for v in _intrinsics(view))
    mfx, mfy, mcx, mcy = (f(v) for v in _intrinsics(view if model_view is None else model_view))
    dp = _np(depth, f).reshape(H, W)
    sn = _np(sensor_normal, f)
    if sn.shape != (3, H, W):
        raise ValueError(f"icp_rows_numpy: sensor_normal must be [3,{H},{W}], got {sn.shape}")
    md = _np(model["depth"], f).reshape(Hm, Wm)
    mn = _np(model["normal"], f)
    mn = mn.reshape(3, Hm * Wm) if chw else mn.reshape(Hm * Wm, 3).T
    if photo is not None:
        lam = f(check_photo_weight(photo["weight"]))
        si, mi = _np(photo["sensor"], f), _np(photo["model"], f)
        if si.shape != (3, H, W) or mi.shape != (3, Hm, Wm):
            raise ValueError(f"icp_rows_numpy: the intensity planes must be [3,{H},{W}] and [3,{Hm},{Wm}], got {si.shape}, {mi.shape}")
    Df = np.asarray(D, np.float64).reshape(3, 4).astype(f)
    R, t = Df[:, :3], Df[:, 3]
    vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    vv, uu = vv.reshape(-1), uu.reshape(-1)
    counts = np.zeros(7, np.int64)
    with np.errstate(all="ignore"):
        d = dp[vv, uu]
        ns = [sn[a][vv, uu] for a in range(3)]
        alive = np.ones(d.shape, bool)

        def gate(ok, which):
            nonlocal alive
            counts[which] = int((alive & ~ok).sum())
            alive = alive & ok

        gate((d > 0) & np.isfinite(d) & (d <= f(depth_max)) & ((ns[0] != 0) | (ns[1] != 0) | (ns[2] != 0)), 1)
        rx, ry = (uu.astype(f) - cx) / fx, (vv.astype(f) - cy) / fy
        X = [rx * d, ry * d, d]
        p = [((R[a, 0] * X[0] + R[a, 1] * X[1]) + R[a, 2] * X[2]) + t[a] for a in range(3)]
        nr = [(R[a, 0] * ns[0] + R[a, 1] * ns[1]) + R[a, 2] * ns[2] for a in range(3)]
        gate((p[2] > 0) & (np.abs(p[0]) < f(RANGE)) & (np.abs(p[1]) < f(RANGE)) & (np.abs(p[2]) < f(RANGE)), 2)
        xf, yf = mfx * (p[0] / p[2]) + mcx, mfy * (p[1] / p[2]) + mcy
        uf, vf = np.rint(xf), np.rint(yf)
        index = (np.abs(uf) < f(INDEX_LIMIT)) & (np.abs(vf) < f(INDEX_LIMIT))           # in float: false for a NaN
        um, vm = np.where(index, uf, f(-1)).astype(np.int64), np.where(index, vf, f(-1)).astype(np.int64)
        inside = index & (um >= 0) & (um < Wm) & (vm >= 0) & (vm < Hm)
        gate(inside, 3)
        sums = np.zeros(28, np.int64)
        extra = np.zeros(4, np.int64)
        if photo is not None:                       # P1 - P5, for every pixel that passed steps 1 - 4
            Is = si[0][vv, uu]
            x0f, y0f = np.floor(xf), np.floor(yf)
            index0 = (np.abs(x0f) < f(INDEX_LIMIT)) & (np.abs(y0f) < f(INDEX_LIMIT))
            x0, y0 = np.where(index0, x0f, f(-1)).astype(np.int64), np.where(index0, y0f, f(-1)).astype(np.int64)
            ph = alive & (Is >= 0) & index0 & (x0 >= 0) & (x0 < Wm - 1) & (y0 >= 0) & (y0 < Hm - 1)
            m00 = np.where(ph, y0 * Wm + x0, 0)
            taps = [np.minimum(m00 + o, Hm * Wm - 1) for o in (0, 1, Wm, Wm + 1)]      # the clamp only meets pixels that are off
            fm = [[mi[c].reshape(-1)[tp] for tp in taps] for c in range(3)]
            for k in range(4):
                ph = ph & (fm[0][k] >= 0) & (np.abs(fm[1][k]) <= 1) & (np.abs(fm[2][k]) <= 1)
            ax, ay = xf - x0f, yf - y0f

            def bilinear(q):
                top, bot = q[0] + ax * (q[1] - q[0]), q[2] + ax * (q[3] - q[2])
                return top + ay * (bot - top)

            Im, gxm, gym = bilinear(fm[0]), bilinear(fm[1]), bilinear(fm[2])
            rI = Im - Is
            a, b = gxm * mfx, gym * mfy
            J = [a / p[2], b / p[2], -(((a * p[0] + b * p[1]) / p[2]) / p[2])]
            J += [p[1] * J[2] - p[2] * J[1], p[2] * J[0] - p[0] * J[2], p[0] * J[1] - p[1] * J[0]]
            wp = [lam * J[i] for i in range(6)] + [lam * rI]
            bounded = np.ones(d.shape, bool)
            for i in range(7):
                bounded &= np.abs(wp[i]) < f(PHOTO_BOUND)          # false for a NaN
            on = ph & bounded
            extra[0], extra[1], extra[2] = int(on.sum()), int((alive & ~ph).sum()), int((ph & ~bounded).sum())
            for i in range(7):
                for j in range(i, 7):
                    fixed = np.trunc((wp[i] * wp[j]).astype(np.float64) * FIXED)
                    sums[tri(i, j)] = np.where(on, fixed, 0.0).astype(np.int64).sum()
            extra[3] = np.where(on, np.trunc((rI * rI).astype(np.float64) * FIXED), 0.0).astype(np.int64).sum()
        mp = np.where(inside, vm * Wm + um, 0)
        dm = md.reshape(-1)[mp]
        n = [mn[a][mp] for a in range(3)]
        gate((dm > 0) & ((n[0] != 0) | (n[1] != 0) | (n[2] != 0)) & (np.abs(n[0]) <= 1) & (np.abs(n[1]) <= 1) & (np.abs(n[2]) <= 1), 4)
        q = [((uf - mcx) / mfx) * dm, ((vf - mcy) / mfy) * dm, dm]
        e = [p[a] - q[a] for a in range(3)]
        gate(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= f(dist) * f(dist), 5)
        gate(((n[0] * nr[0] + n[1] * nr[1]) + n[2] * nr[2]) >= f(cos_min), 6)
        counts[0] = int(alive.sum())
        w = [n[0], n[1], n[2], p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0],
             (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]]
        for i in range(7):
            for j in range(i, 7):
                fixed = np.trunc((w[i] * w[j]).astype(np.float64) * FIXED)          # fp32 product, exact in fp64
                sums[tri(i, j)] += np.where(alive, fixed, 0.0).astype(np.int64).sum()
    return (sums, counts) if photo is None else (sums, counts, extra)


def _rigid_inverse(R, t):
    Ri = [[R[b][a] for b in range(3)] for a in range(3)]
    return Ri, [-((Ri[a][0] * t[0] + Ri[a][1] * t[1]) + Ri[a][2] * t[2]) for a in range(3)]


def _rigid_product(RA, tA, RB, tB):
    R = [[(RA[a][0] * RB[0][b] + RA[a][1] * RB[1][b]) + RA[a][2] * RB[2][b] for b in range(3)] for a in range(3)]
    return R, [((RA[a][0] * tB[0] + RA[a][1] * tB[1]) + RA[a][2] * tB[2]) + tA[a] for a in range(3)]


def _split(M):
    """(R, t) as Python floats of a [3,4] or [4,4] matrix (an fp32 one converts exactly)."""
    M = np.asarray(_np(M, np.float64))
    return [[float(M[a, b]) for b in range(3)] for a in range(3)], [float(M[a, 3]) for a in range(3)]


def _join(R, t):
    return np.array([[R[a][0], R[a][1], R[a][2], t[a]] for a in range(3)], np.float64)


def initial_transform(T_model, T_init=None):
    """D_0 [3,4] fp64 = T_model T_init^-1 (the header's rigid inverse and product), the identity for T_init = None."""
    if T_init is None:
        return np.eye(4)[:3].copy()
    Ri, ti = _rigid_inverse(*_split(T_init))
    return _join(*_rigid_product(*_split(T_model), Ri, ti))


def pose_of(D, T_model):
    """T_w2c [4,4] fp32 = D^-1 T_model, in fp64 and rounded once."""
    Ri, ti = _rigid_inverse(*_split(D))
    T = np.eye(4, dtype=np.float32)
    T[:3] = _join(*_rigid_product(Ri, ti, *_split(T_model))).astype(np.float32)
    return T


def _horner(c, u):
    v = c[-1]
    for k in range(len(c) - 2, -1, -1):
        v = c[k] + u * v
    return v


def se3_exp_poly(x):
    """Exp([rho; theta]) [3,4] fp64 by the closed form of pose.SE3_exp with the three coefficients as EXP_TERMS-term Taylor
    polynomials in s = |theta|^2 (Horner), for s <= 0.25: neither sin, cos nor sqrt, one rounding per operation."""
    x = [float(v) for v in x]
    th = x[3:]
    s = (th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]
    a, b, c = _horner(COEF_A, -s), _horner(COEF_B, -s), _horner(COEF_C, -s)
    Wm = [[0.0, -th[2], th[1]], [th[2], 0.0, -th[0]], [-th[1], th[0], 0.0]]
    R = [[0.0] * 3 for _ in range(3)]
    V = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            w2 = th[i] * th[j] - s if i == j else th[i] * th[j]
            eye = 1.0 if i == j else 0.0
            R[i][j] = (eye + a * Wm[i][j]) + b * w2
            V[i][j] = (eye + b * Wm[i][j]) + c * w2
    t = [(V[i][0] * x[0] + V[i][1] * x[1]) + V[i][2] * x[2] for i in range(3)]
    return _join(R, t)


def icp_solve_numpy(sums, accepted, D, min_pixels=32, min_pivot_ratio=1e-6, damping=0.0, converged=1e-4, last=False):
    """k_icp_solve's thread 0 in Python floats (fp64, one rounding per operation): dict(x [6], pivots [6], status, xx, D
    [3,4]).  `sums` are the 28 fixed-point sums, `accepted` the count.  A failure status returns D unchanged."""
    sums = [int(v) for v in np.asarray(sums).reshape(-1)[:28]]
    D0 = np.asarray(D, np.float64).reshape(3, 4).copy()
    out = {"x": np.zeros(6), "pivots": np.zeros(6), "status": ITERATING, "xx": 0.0, "D": D0}
    if int(accepted) < int(min_pixels):
        out["status"] = TOO_FEW
        return out
    inv = 1.0 / FIXED
    H = [[float(sums[tri(min(i, j), max(i, j))]) * inv for j in range(6)] for i in range(6)]
    g = [float(sums[tri(i, 6)]) * inv for i in range(6)]
    damping = float(damping)
    m = 0.0
    for i in range(6):
        H[i][i] = H[i][i] + damping
        m = H[i][i] if i == 0 or H[i][i] > m else m
    floor_ = float(min_pivot_ratio) * m
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    status = ITERATING
    for j in range(6):
        tk = [L[j][k] * d[k] for k in range(j)]
        v = H[j][j]
        for k in range(j):
            v = v - L[j][k] * tk[k]
        out["pivots"][j] = v
        good = v > floor_
        if not good:
            status = DEGENERATE
        d[j] = v if good else 0.0
        for i in range(j + 1, 6):
            s = H[i][j]
            for k in range(j):
                s = s - L[i][k] * tk[k]
            L[i][j] = s / v if good else 0.0
    if status == DEGENERATE:
        out["status"] = status
        return out
    y = [0.0] * 6
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i] / d[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    s = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
    xx = x[0] * x[0]
    for i in range(1, 6):
        xx = xx + x[i] * x[i]
    out["x"], out["xx"] = np.array(x), xx
    if not s <= MAX_STEP2 or not xx < math.inf:
        out["status"] = STEP_TOO_LARGE
        return out
    E = se3_exp_poly(x)
    out["D"] = _join(*_rigid_product(*_split(E), *_split(D0)))
    conv = float(converged)
    out["status"] = CONVERGED if xx < conv * conv else (MAX_ITERATIONS if last else ITERATING)
    return out


def _f64_bits(v) -> int:
    return int(np.array([v], np.float64).view(np.int64)[0])


def read_record(words, rgbd=False) -> dict:
    """The record's MGS_ICP_RECORD_WORDS 8-byte words (int64) as a dict; with `rgbd` (a record of mgs_icp_align_rgbd) also
    "photo", PHOTO_NAMES' counts, and "sum_ri2", the sum of r_I^2 over the accepted photometric rows."""
    w = _np(words, np.int64).reshape(-1)
    st = int(w[_REC_STATUS])
    extra = {} if not rgbd else {"photo": dict(zip(PHOTO_NAMES, (int(v) for v in w[_REC_PHOTO:_REC_PHOTO + 3]))),
                                 "sum_ri2": float(w[_REC_PHOTO + 3]) / FIXED}
    return {**extra, "sums": w[:28].copy(), "counts": dict(zip(COUNT_NAMES, (int(v) for v in w[_REC_COUNTS:_REC_COUNTS + 7]))),
            "x": w[_REC_X:_REC_X + 6].view(np.float64).copy(), "pivots": w[_REC_PIVOTS:_REC_PIVOTS + 6].view(np.float64).copy(),
            "status": st, "status_name": STATUS_NAMES[st] if 0 <= st < len(STATUS_NAMES) else "undefined", "ok": status_ok(st),
            "level": int(w[_REC_LEVEL]), "iteration": int(w[_REC_ITER]), "iterations_run": int(w[_REC_RUN]),
            "converged_level": int(w[_REC_DONE])}


def read_history(rows, rgbd=False) -> dict:
    """The history table [n, MGS_ICP_HISTORY_WORDS] (int64) as a dict of columns; with `rgbd` also "sum_ri2" (then sum_r2
    is the combined sum, the photometric part weighted by lambda^2)."""
    h = _np(rows, np.int64).reshape(-1, _cabi.ICP_HISTORY_WORDS)
    extra = {"sum_ri2": h[:, 7].astype(np.float64) / FIXED} if rgbd else {}
    return {**extra, "accepted": h[:, 0].copy(), "sum_r2": h[:, 1].astype(np.float64) / FIXED, "xx": h[:, 2].copy().view(np.float64),
            "status": h[:, 3].copy(), "ran": h[:, 4].copy(), "level": h[:, 5].copy(), "iteration": h[:, 6].copy()}


def align_numpy(model, depth, view, T_model, T_init=None, model_view=None, levels=LEVELS, dist=0.1, cos_min=0.8, depth_max=10.0,
                min_pixels=32, min_pivot_ratio=1e-6, damping=0.0, converged=1e-4, max_jump=0.05, sensor_normal=None,
                image=None, photo_weight=0.0):
    """With `image` (the sensor's RGB, [3,H,W] or [H,W,3]) and photo_weight > 0: mgs_icp_align_rgbd on the CPU - `model`
    carries "color", the intensity planes are formed once (returned under "intensity" and "model_intensity"), too few tests
    accepted + photo accepted, and the record and history carry the photometric words.  Otherwise mgs_icp_align on the CPU: the whole schedule with the device's early-exit rules.  dict(T_w2c fp32 [4,4], D fp64
    [3,4], record int64 [MGS_ICP_RECORD_WORDS], history int64 [n,8], status, info = read_record(record)): `record` and
    `history` are the device's words.  `sensor_normal` defaults to surface.depth_normal_torch(depth, pixel_center=0,
    max_jump)."""
    levels = check_levels(levels)
    check_params(dist, cos_min, depth_max, min_pixels, min_pivot_ratio, damping, converged)
    H, W = _sensor_shape(depth, "align_numpy")
    Hm, Wm, _ = _model_layout(model, "align_numpy")
    intr = _intrinsics(view)
    photo = None
    if check_photo_weight(photo_weight) > 0.0 and image is not None:
        _rgb_layout(image, (H, W), "align_numpy")
        if not isinstance(model, dict) or model.get("color") is None:
            raise ValueError("align_numpy: photometric rows need the model's colour plane, model[\"color\"]")
        _rgb_layout(model["color"], (Hm, Wm), "align_numpy")
        photo = {"sensor": intensity_planes_torch(image), "model": intensity_planes_torch(model["color"], valid=model["depth"]),
                 "weight": photo_weight}
    if sensor_normal is None:
        from .surface import depth_normal_torch
        sensor_normal = depth_normal_torch(torch.from_numpy(_np(depth, np.float32).reshape(H, W)), *intr, pixel_center=0.0, max_jump=max_jump)
    Tm = _np(T_model, np.float32).reshape(4, 4)
    D = initial_transform(Tm, None if T_init is None else _np(T_init, np.float32).reshape(4, 4))
    total = sum(n for _, n in levels)
    rec = np.zeros(_cabi.ICP_RECORD_WORDS, np.int64)
    rec[_REC_DONE] = -1
    hist = np.zeros((total, _cabi.ICP_HISTORY_WORDS), np.int64)
    index = 0
    for level, (stride, iters) in enumerate(levels):
        for it in range(iters):
            row = hist[index]
            row[5], row[6] = level, it
            if rec[_REC_STATUS] >= TOO_FEW or rec[_REC_DONE] == level:
                row[3] = rec[_REC_STATUS]
            else:
                sums, counts, *extra = icp_rows_numpy(model, depth, sensor_normal, D, intr, model_view, stride, dist, cos_min, depth_max,
                                                      photo=photo)
                rows = int(counts[0]) + (int(extra[0][0]) if photo else 0)
                s = icp_solve_numpy(sums, rows, D, min_pixels, min_pivot_ratio, damping, converged, last=index == total - 1)
                D = s["D"]
                rec[:28], rec[_REC_COUNTS:_REC_COUNTS + 7] = sums, counts
                rec[_REC_X:_REC_X + 6] = s["x"].view(np.int64)
                rec[_REC_PIVOTS:_REC_PIVOTS + 6] = s["pivots"].view(np.int64)
                rec[_REC_STATUS], rec[_REC_LEVEL], rec[_REC_ITER] = s["status"], level, it
                rec[_REC_RUN] += 1
                if s["status"] == CONVERGED:
                    rec[_REC_DONE] = level
                row[0], row[1], row[2], row[3], row[4] = counts[0], sums[tri(6, 6)], _f64_bits(s["xx"]), s["status"], 1
                if photo:
                    rec[_REC_PHOTO:_REC_PHOTO + 4], row[7] = extra[0], extra[0][3]
            index += 1
    out = {"T_w2c": pose_of(D, Tm), "D": D, "record": rec, "history": hist, "status": int(rec[_REC_STATUS]),
           "info": read_record(rec, rgbd=photo is not None)}
    if photo:
        out["intensity"], out["model_intensity"] = photo["sensor"], photo["model"]
    return out


# ---- the device ------------------------------------------------------------------------------------------------------
def depth_normal(depth: torch.Tensor, fx, fy, cx, cy, pixel_center: float = 0.0, max_jump: float = 0.05) -> torch.Tensor:
    """mgs_depth_normal of a contiguous fp32 plane [H,W] on the device: [3,H,W], one launch."""
    H, W = (int(v) for v in depth.shape[-2:])
    out = torch.empty(3, H, W, device=depth.device)
    a = _cabi.DepthNormalArgs()
    a.width, a.height = W, H
    a.fx, a.fy, a.cx, a.cy = float(fx), float(fy), float(cx), float(cy)
    a.pixel_center, a.max_jump = float(pixel_center), float(max_jump)
    a.depth, a.normal = depth.data_ptr(), out.data_ptr()
    _cabi.check(_cabi.lib().mgs_depth_normal(C.byref(a), stream_ptr(depth.device)), "mgs_depth_normal")
    return out


def intensity_planes(image: torch.Tensor, valid=None) -> torch.Tensor:
    """mgs_icp_intensity on the device: [3,H,W] = (I, gx, gy) of an RGB plane [H,W,3] or [3,H,W], as intensity_planes_torch;
    `valid` is None, a bool plane or an fp32 plane [H,W] that is on where > 0 (a ray cast's depth).  One launch, no host
    read."""
    H, W, chw = _rgb_layout(image, None, "icp.intensity_planes")
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise RuntimeError("icp.intensity_planes runs on the GPU only (HIP kernels, gfx950); the mirror intensity_planes_torch runs anywhere")
    rgb = image.detach().to(torch.float32).contiguous()
    a = _cabi.IcpIntensityArgs()
    a.width, a.height, a.chw = W, H, 1 if chw else 0
    if valid is not None:
        valid = torch.as_tensor(valid).detach().to(rgb.device, torch.float32).contiguous()
        if valid.numel() != H * W:
            raise ValueError(f"icp.intensity_planes: valid must be [{H},{W}]")
        a.valid = valid.data_ptr()
    out = torch.empty(3, H, W, device=rgb.device)
    a.rgb, a.out = rgb.data_ptr(), out.data_ptr()
    _cabi.check(_cabi.lib().mgs_icp_intensity(C.byref(a), stream_ptr(rgb.device)), "mgs_icp_intensity")
    del rgb, valid
    return out


def align(model, depth, view, T_model, T_init=None, model_view=None, levels=LEVELS, dist=0.1, cos_min=0.8, depth_max=10.0,
          min_pixels=32, min_pivot_ratio=1e-6, damping=0.0, converged=1e-4, max_jump=0.05, read=True, sensor_normal=None,
          image=None, photo_weight=0.0):
    """Align the sensor plane `depth` [H,W] (pixel centre 0, intrinsics of `view`) to the model view `model` rendered at
    T_model: a ray cast's dict, or dict(depth [Hm,Wm], normal [Hm,Wm,3] or [3,Hm,Wm]) with camera-frame unit normals, with
    the intrinsics of `model_view` (default: those of `view`).  T_init is the sensor camera's start pose (default T_model).
    Returns device tensors: T_w2c fp32 [4,4] (copy_ it into a camera's T), D fp64 [3,4], record int64 [56], history int64
    [n,8], status (a 0-d view of the record's status word); with `read` also info = read_record after ONE host read, with
    the history's columns under info["history"].  1 + 2 n launches (and mgs_depth_normal's), enqueued at once.
    `min_pixels` is an absolute count of accepted pixels and the same at every level: 32 is a sixteenth of the stride-4
    grid of a 160 x 120 image but a thousandth of a 640 x 480 image at stride 1 - scale it with the image where a
    fraction is meant.
    RGB-D: with `image` (the sensor's RGB, [3,H,W] or [H,W,3]) and photo_weight = lambda > 0 the call goes through
    mgs_icp_align_rgbd: `model` carries "color" ([Hm,Wm,3] or [3,Hm,Wm]), every pixel that projects into the model view
    also adds the photometric row lambda [J_I, r_I], too few tests accepted + photo accepted, the result also holds
    "intensity" [3,H,W] and "model_intensity" [3,Hm,Wm], and info gains "photo" and "sum_ri2" (history: "sum_ri2").  Two
    more launches, once per call.  Without either it is the call above, launch for launch."""
    levels = check_levels(levels)
    check_params(dist, cos_min, depth_max, min_pixels, min_pivot_ratio, damping, converged)
    rgbd = check_photo_weight(photo_weight) > 0.0 and image is not None
    H, W = _sensor_shape(depth)
    Hm, Wm, chw = _model_layout(model)
    if rgbd:
        image_chw = _rgb_layout(image, (H, W))[2]
        if not isinstance(model, dict) or model.get("color") is None:
            raise ValueError("icp: photometric rows need the model's colour plane, model[\"color\"]")
        color_chw = _rgb_layout(model["color"], (Hm, Wm))[2]
    if 3 * Hm * Wm > 2 ** 31 - 1:
        raise ValueError(f"icp: the model planes {Hm} x {Wm} exceed 32-bit indices")
    fx, fy, cx, cy = _intrinsics(view)
    mfx, mfy, mcx, mcy = _intrinsics(view if model_view is None else model_view)
    md = model["depth"]
    devices = {t.device for t in (md, model["normal"], depth) + ((image, model["color"]) if rgbd else ()) if torch.is_tensor(t)}
    if not any(d.type == "cuda" for d in devices):
        raise RuntimeError("icp.align runs on the GPU only (HIP kernels, gfx950); the mirror align_numpy runs anywhere")
    if len(devices) != 1:
        raise ValueError(f"icp: the model planes and the depth must lie on one device, got {sorted(str(d) for d in devices)}")
    dev = devices.pop()
    f32 = lambda t: torch.as_tensor(t).detach().to(dev, torch.float32).contiguous()
    dp, md, mn = f32(depth).reshape(H, W), f32(md).reshape(Hm, Wm), f32(model["normal"])
    sn = depth_normal(dp, fx, fy, cx, cy, 0.0, max_jump) if sensor_normal is None else f32(sensor_normal)
    if tuple(sn.shape) != (3, H, W):
        raise ValueError(f"icp: sensor_normal must be [3,{H},{W}]")
    Tm = f32(T_model)
    Ti = None if T_init is None else f32(T_init)
    if tuple(Tm.shape) != (4, 4) or (Ti is not None and tuple(Ti.shape) != (4, 4)):
        raise ValueError("icp: T_model and T_init must be [4,4]")
    total = sum(n for _, n in levels)
    L = _cabi.lib()
    scratch_bytes = L.mgs_icp_rgbd_scratch_bytes if rgbd else L.mgs_icp_scratch_bytes
    scratch_words, hist_at = int(scratch_bytes(total)) // 8, int(scratch_bytes(0)) // 8
    if scratch_words == 0:
        raise ValueError("icp: unsupported iteration count")
    # one allocation: [partial sums | history | record | D | T_w2c], so that ONE read brings everything after the partials
    R, HWORDS = _cabi.ICP_RECORD_WORDS, _cabi.ICP_HISTORY_WORDS
    buf = torch.zeros(scratch_words + R + 12 + 8, dtype=torch.int64, device=dev)
    history = buf[hist_at:scratch_words].view(total, HWORDS)
    record = buf[scratch_words:scratch_words + R]
    D = buf[scratch_words + R:scratch_words + R + 12].view(torch.float64).view(3, 4)
    T = buf[scratch_words + R + 12:].view(torch.float32).view(4, 4)
    r = _cabi.IcpRgbdArgs() if rgbd else None
    a = r.icp if rgbd else _cabi.IcpArgs()          # r.icp is a view of r's own bytes
    a.width, a.height, a.model_width, a.model_height = W, H, Wm, Hm
    a.model_normal_chw, a.num_levels, a.min_pixels = 1 if chw else 0, len(levels), int(min_pixels)
    for l, (s, n) in enumerate(levels):
        a.stride[l], a.iterations[l] = s, n
    a.fx, a.fy, a.cx, a.cy, a.mfx, a.mfy, a.mcx, a.mcy = fx, fy, cx, cy, mfx, mfy, mcx, mcy
    a.dist, a.cos_min, a.depth_max = float(dist), float(cos_min), float(depth_max)
    a.min_pivot_ratio, a.damping, a.converged = float(min_pivot_ratio), float(damping), float(converged)
    a.depth, a.normal, a.model_depth, a.model_normal = dp.data_ptr(), sn.data_ptr(), md.data_ptr(), mn.data_ptr()
    a.T_model, a.T_init = Tm.data_ptr(), None if Ti is None else Ti.data_ptr()
    a.scratch, a.T_w2c, a.D, a.record = buf.data_ptr(), T.data_ptr(), D.data_ptr(), record.data_ptr()
    out = {"T_w2c": T, "D": D, "record": record, "history": history, "status": record[_REC_STATUS]}
    if rgbd:
        im, mc = f32(image), f32(model["color"])
        out["intensity"], out["model_intensity"] = torch.empty(3, H, W, device=dev), torch.empty(3, Hm, Wm, device=dev)
        r.photo_weight, r.image_chw, r.model_color_chw = float(photo_weight), 1 if image_chw else 0, 1 if color_chw else 0
        r.image, r.model_color = im.data_ptr(), mc.data_ptr()
        r.intensity, r.model_intensity = out["intensity"].data_ptr(), out["model_intensity"].data_ptr()
        _cabi.check(L.mgs_icp_align_rgbd(C.byref(r), stream_ptr(dev)), "mgs_icp_align_rgbd")
        del im, mc
    else:
        _cabi.check(L.mgs_icp_align(C.byref(a), stream_ptr(dev)), "mgs_icp_align")
    del dp, md, mn, sn, Tm, Ti      # held until the launches were enqueued; the allocator orders their reuse on this stream
    if read:
        host = buf[hist_at:].cpu().numpy()
        nh = total * HWORDS
        out["info"] = read_record(host[nh:nh + R], rgbd=rgbd)
        out["info"]["history"] = read_history(host[:nh], rgbd=rgbd)
        out["info"]["D"] = host[nh + R:nh + R + 12].view(np.float64).reshape(3, 4).copy()
        out["info"]["T_w2c"] = host[nh + R + 12:].view(np.float32).reshape(4, 4).copy()
    return out


def select_pose(result, T_fallback):
    """result["T_w2c"] where the alignment's status is ok (converged, or out of iterations), else T_fallback: fp32 [4,4],
    chosen on the device by the record's status word - no host read."""
    st = result["status"]
    return torch.where((st == CONVERGED) | (st == MAX_ITERATIONS), result["T_w2c"], T_fallback)


def track_against_volume(vol, depth, T_prev, view, image=None, photo_weight=0.0, z_far=4.0, z_near=0.2, step=0.5, min_weight=1.0,
                         **kw):
    """Ray cast `vol` (a TSDFVolume or a SparseTSDFVolume) at T_prev with the intrinsics and size of `view`, then `align`
    the sensor plane `depth` to it, starting at T_prev: the frame-to-model step of KinectFusion's loop.  No host read
    with read=False.  The result of `align`, with the ray cast's planes under "model".  With `image` and photo_weight > 0
    the ray cast's colour enters too (align's RGB-D path); a volume no view was integrated into with an image then raises
    ValueError."""
    if check_photo_weight(photo_weight) > 0.0 and image is not None and not getattr(vol, "has_color", False):
        raise ValueError("icp: photometric rows need a volume fused with colour (integrate(..., image=))")
    _, fx, fy, cx, cy, H, W = view_tuple(view)
    planes = vol.raycast(T_prev, fx, fy, cx, cy, H, W, z_near=z_near, z_far=z_far, step=step, min_weight=min_weight)
    depth = torch.as_tensor(depth).detach().to(vol.dev, torch.float32)      # a host frame goes to the volume's device
    if image is not None:
        image = torch.as_tensor(image).detach().to(vol.dev, torch.float32)
    out = align(planes, depth, (fx, fy, cx, cy), T_prev, image=image, photo_weight=photo_weight, **kw)
    out["model"] = planes
    return out
