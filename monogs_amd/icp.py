"""Frame-to-model ICP: point-to-plane alignment of a sensor depth frame against a model view - the ray cast of a TSDF
volume, or the viewer's surface planes (csrc/icp.hip; the contract is in include/monogs_raster.h and DESIGN.md
"Frame-to-model ICP").  With integrate and ray cast this closes KinectFusion's loop: integrate, ray cast, align.

    res = vol.track(depth, T_prev, camera, z_far=4.0)       # ray cast at T_prev, then align: all on the device
    camera.T.copy_(res["T_w2c"])                             # fp32 [4,4]; res["status"] says whether to trust it
    res = align(planes, depth, view, T_model, T_init=T_guess, levels=((2, 5), (1, 10)))

The whole schedule of levels and iterations is enqueued at once; a level that has converged lets its remaining launches
return at once, a failure status ends everything, nothing is read by the host in between.

The mirrors `icp_rows_numpy`, `icp_solve_numpy` and `align_numpy` ARE the contract: fp32 NumPy for the rows (every
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


# ---- mirrors ---------------------------------------------------------------------------------------------------------
def icp_rows_numpy(model, depth, sensor_normal, D, view, model_view=None, stride=1, dist=0.1, cos_min=0.8, depth_max=10.0):
    """k_icp_rows in fp32 NumPy: (sums int64 [28], counts int64 [7]) over the pixels of the stride grid.  `sums` is the
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
        uf, vf = np.rint(mfx * (p[0] / p[2]) + mcx), np.rint(mfy * (p[1] / p[2]) + mcy)
        index = (np.abs(uf) < f(INDEX_LIMIT)) & (np.abs(vf) < f(INDEX_LIMIT))           # in float: false for a NaN
        um, vm = np.where(index, uf, f(-1)).astype(np.int64), np.where(index, vf, f(-1)).astype(np.int64)
        inside = index & (um >= 0) & (um < Wm) & (vm >= 0) & (vm < Hm)
        gate(inside, 3)
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
        sums = np.zeros(28, np.int64)
        for i in range(7):
            for j in range(i, 7):
                fixed = np.trunc((w[i] * w[j]).astype(np.float64) * FIXED)          # fp32 product, exact in fp64
                sums[tri(i, j)] = np.where(alive, fixed, 0.0).astype(np.int64).sum()
    return sums, counts


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


def read_record(words) -> dict:
    """The record's MGS_ICP_RECORD_WORDS 8-byte words (int64) as a dict."""
    w = _np(words, np.int64).reshape(-1)
    st = int(w[_REC_STATUS])
    return {"sums": w[:28].copy(), "counts": dict(zip(COUNT_NAMES, (int(v) for v in w[_REC_COUNTS:_REC_COUNTS + 7]))),
            "x": w[_REC_X:_REC_X + 6].view(np.float64).copy(), "pivots": w[_REC_PIVOTS:_REC_PIVOTS + 6].view(np.float64).copy(),
            "status": st, "status_name": STATUS_NAMES[st] if 0 <= st < len(STATUS_NAMES) else "undefined", "ok": status_ok(st),
            "level": int(w[_REC_LEVEL]), "iteration": int(w[_REC_ITER]), "iterations_run": int(w[_REC_RUN]),
            "converged_level": int(w[_REC_DONE])}


def read_history(rows) -> dict:
    """The history table [n, MGS_ICP_HISTORY_WORDS] (int64) as a dict of columns."""
    h = _np(rows, np.int64).reshape(-1, _cabi.ICP_HISTORY_WORDS)
    return {"accepted": h[:, 0].copy(), "sum_r2": h[:, 1].astype(np.float64) / FIXED, "xx": h[:, 2].copy().view(np.float64),
            "status": h[:, 3].copy(), "ran": h[:, 4].copy(), "level": h[:, 5].copy(), "iteration": h[:, 6].copy()}


def align_numpy(model, depth, view, T_model, T_init=None, model_view=None, levels=LEVELS, dist=0.1, cos_min=0.8, depth_max=10.0,
                min_pixels=32, min_pivot_ratio=1e-6, damping=0.0, converged=1e-4, max_jump=0.05, sensor_normal=None):
    """mgs_icp_align on the CPU: the whole schedule with the device's early-exit rules.  dict(T_w2c fp32 [4,4], D fp64
    [3,4], record int64 [MGS_ICP_RECORD_WORDS], history int64 [n,8], status, info = read_record(record)): `record` and
    `history` are the device's words.  `sensor_normal` defaults to surface.depth_normal_torch(depth, pixel_center=0,
    max_jump)."""
    levels = check_levels(levels)
    check_params(dist, cos_min, depth_max, min_pixels, min_pivot_ratio, damping, converged)
    H, W = _sensor_shape(depth, "align_numpy")
    _model_layout(model, "align_numpy")
    intr = _intrinsics(view)
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
                sums, counts = icp_rows_numpy(model, depth, sensor_normal, D, intr, model_view, stride, dist, cos_min, depth_max)
                s = icp_solve_numpy(sums, counts[0], D, min_pixels, min_pivot_ratio, damping, converged, last=index == total - 1)
                D = s["D"]
                rec[:28], rec[_REC_COUNTS:_REC_COUNTS + 7] = sums, counts
                rec[_REC_X:_REC_X + 6] = s["x"].view(np.int64)
                rec[_REC_PIVOTS:_REC_PIVOTS + 6] = s["pivots"].view(np.int64)
                rec[_REC_STATUS], rec[_REC_LEVEL], rec[_REC_ITER] = s["status"], level, it
                rec[_REC_RUN] += 1
                if s["status"] == CONVERGED:
                    rec[_REC_DONE] = level
                row[0], row[1], row[2], row[3], row[4] = counts[0], sums[tri(6, 6)], _f64_bits(s["xx"]), s["status"], 1
            index += 1
    return {"T_w2c": pose_of(D, Tm), "D": D, "record": rec, "history": hist, "status": int(rec[_REC_STATUS]), "info": read_record(rec)}


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


def align(model, depth, view, T_model, T_init=None, model_view=None, levels=LEVELS, dist=0.1, cos_min=0.8, depth_max=10.0,
          min_pixels=32, min_pivot_ratio=1e-6, damping=0.0, converged=1e-4, max_jump=0.05, read=True, sensor_normal=None):
    """Align the sensor plane `depth` [H,W] (pixel centre 0, intrinsics of `view`) to the model view `model` rendered at
    T_model: a ray cast's dict, or dict(depth [Hm,Wm], normal [Hm,Wm,3] or [3,Hm,Wm]) with camera-frame unit normals, with
    the intrinsics of `model_view` (default: those of `view`).  T_init is the sensor camera's start pose (default T_model).
    Returns device tensors: T_w2c fp32 [4,4] (copy_ it into a camera's T), D fp64 [3,4], record int64 [56], history int64
    [n,8], status (a 0-d view of the record's status word); with `read` also info = read_record after ONE host read, with
    the history's columns under info["history"].  1 + 2 n launches (and mgs_depth_normal's), enqueued at once.
    `min_pixels` is an absolute count of accepted pixels and the same at every level: 32 is a sixteenth of the stride-4
    grid of a 160 x 120 image but a thousandth of a 640 x 480 image at stride 1 - scale it with the image where a
    fraction is meant."""
    levels = check_levels(levels)
    check_params(dist, cos_min, depth_max, min_pixels, min_pivot_ratio, damping, converged)
    H, W = _sensor_shape(depth)
    Hm, Wm, chw = _model_layout(model)
    if 3 * Hm * Wm > 2 ** 31 - 1:
        raise ValueError(f"icp: the model planes {Hm} x {Wm} exceed 32-bit indices")
    fx, fy, cx, cy = _intrinsics(view)
    mfx, mfy, mcx, mcy = _intrinsics(view if model_view is None else model_view)
    md = model["depth"]
    devices = {t.device for t in (md, model["normal"], depth) if torch.is_tensor(t)}
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
    scratch_words, hist_at = int(L.mgs_icp_scratch_bytes(total)) // 8, int(L.mgs_icp_scratch_bytes(0)) // 8
    if scratch_words == 0:
        raise ValueError("icp: unsupported iteration count")
    # one allocation: [partial sums | history | record | D | T_w2c], so that ONE read brings everything after the partials
    R, HWORDS = _cabi.ICP_RECORD_WORDS, _cabi.ICP_HISTORY_WORDS
    buf = torch.zeros(scratch_words + R + 12 + 8, dtype=torch.int64, device=dev)
    history = buf[hist_at:scratch_words].view(total, HWORDS)
    record = buf[scratch_words:scratch_words + R]
    D = buf[scratch_words + R:scratch_words + R + 12].view(torch.float64).view(3, 4)
    T = buf[scratch_words + R + 12:].view(torch.float32).view(4, 4)
    a = _cabi.IcpArgs()
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
    _cabi.check(L.mgs_icp_align(C.byref(a), stream_ptr(dev)), "mgs_icp_align")
    del dp, md, mn, sn, Tm, Ti      # held until the launches were enqueued; the allocator orders their reuse on this stream
    out = {"T_w2c": T, "D": D, "record": record, "history": history, "status": record[_REC_STATUS]}
    if read:
        host = buf[hist_at:].cpu().numpy()
        nh = total * HWORDS
        out["info"] = read_record(host[nh:nh + R])
        out["info"]["history"] = read_history(host[:nh])
        out["info"]["D"] = host[nh + R:nh + R + 12].view(np.float64).reshape(3, 4).copy()
        out["info"]["T_w2c"] = host[nh + R + 12:].view(np.float32).reshape(4, 4).copy()
    return out


def select_pose(result, T_fallback):
    """result["T_w2c"] where the alignment's status is ok (converged, or out of iterations), else T_fallback: fp32 [4,4],
    chosen on the device by the record's status word - no host read."""
    st = result["status"]
    return torch.where((st == CONVERGED) | (st == MAX_ITERATIONS), result["T_w2c"], T_fallback)


def track_against_volume(vol, depth, T_prev, view, z_far=4.0, z_near=0.2, step=0.5, min_weight=1.0, **kw):
    """Ray cast `vol` (a TSDFVolume or a SparseTSDFVolume) at T_prev with the intrinsics and size of `view`, then `align`
    the sensor plane `depth` to it, starting at T_prev: the frame-to-model step of KinectFusion's loop.  No host read
    with read=False.  The result of `align`, with the ray cast's planes under "model"."""
    _, fx, fy, cx, cy, H, W = view_tuple(view)
    planes = vol.raycast(T_prev, fx, fy, cx, cy, H, W, z_near=z_near, z_far=z_far, step=step, min_weight=min_weight)
    depth = torch.as_tensor(depth).detach().to(vol.dev, torch.float32)      # a host frame goes to the volume's device
    out = align(planes, depth, (fx, fy, cx, cy), T_prev, **kw)
    out["model"] = planes
    return out
