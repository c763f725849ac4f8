"""Headless viewer: the views of the reference's GUI (gui/slam_gui.py:544-653, gui/gui_utils.py:24-66,
gui/gl_render/shaders/gau_frag.glsl:20-35) as finished uint8 [H,W,3] frames, made on the device.

  NativeViewer.frame(camera, mode)   rgb | depth | opacity | time | flat_ball | gaussian_ball, with the keyframe frusta,
                                     the current camera and the trajectory drawn over it; enqueues HIP kernels
                                     (csrc/viewer.hip through the C ABI) and reads nothing back; also the two
                                     SURFACE_MODES median_depth | normal
  NativeViewer.surface(camera)       the forward's planes plus median depth / index and normals (csrc/surface.hip)
  follow_camera(T, ...)              the GUI's view_dir / view_dir_behind camera of a tracked pose
  view_frame_torch(...)              the mirror in plain torch: the same arithmetic for the colour maps, the time tint
                                     and the line stepping; brute-force searches for the ellipsoid shader and the blend
  save_frame(path, frame)            PNG through PIL when importable, else binary PPM

Contracts that are this repository's own: the colour map is matplotlib's 256-entry `jet` table indexed by
min(255, int(clamp(t, 0, 1) * 256)) - imgviz.depth2rgb, which the GUI calls, is not installed anywhere this project is
built; of the OpenGL path only the fragment rule is followed, on this rasteriser's own projection."""
from __future__ import annotations

import ctypes as C
import functools
import math
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _cabi
from .synthetic import SH_C0, projection_matrix2

MODES = ("rgb", "depth", "opacity", "time", "flat_ball", "gaussian_ball")
SURFACE_MODES = ("median_depth", "normal")      # views of the surface planes (surface.py); frame() takes them too
DEPTH_LO = 0.1                        # slam_gui.py:582-584 (min_value of the depth colour map)
BALL_THRESHOLD = {"flat_ball": 0.22, "gaussian_ball": 0.4}      # gau_frag.glsl:30,33
NEAR_Z = 0.01                         # near plane of the line overlay (the cameras' znear)
COLOR_KEYFRAME, COLOR_CURRENT, COLOR_TRAJECTORY = (0, 0, 255), (0, 255, 0), (255, 0, 0)
# gui_utils.py:52-66
FRUSTUM_POINTS = ((0.0, 0.0, 0.0), (1.0, -0.5, 2.0), (-1.0, -0.5, 2.0), (1.0, 0.5, 2.0), (-1.0, 0.5, 2.0))
FRUSTUM_LINES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (2, 4), (3, 4))

# matplotlib's `jet`, 256 x 3 uint8 (tests/golden/make_jet_lut.py generates the fixture this is checked against)
JET_LUT = np.frombuffer(bytes.fromhex(
    "00007f00008400008800008d00009100009600009a00009f0000a30000a80000ac0000b10000b60000ba0000bf0000c3"
    "0000c80000cc0000d10000d50000da0000de0000e30000e80000ec0000f10000f50000fa0000fe0000ff0000ff0000ff"
    "0000ff0004ff0008ff000cff0010ff0014ff0018ff001cff0020ff0024ff0028ff002cff0030ff0034ff0038ff003cff"
    "0040ff0044ff0048ff004cff0050ff0054ff0058ff005cff0060ff0064ff0068ff006cff0070ff0074ff0078ff007cff"
    "0080ff0084ff0088ff008cff0090ff0094ff0098ff009cff00a0ff00a4ff00a8ff00acff00b0ff00b4ff00b8ff00bcff"
    "00c0ff00c4ff00c8ff00ccff00d0ff00d4ff00d8ff00dcfe00e0fa00e4f702e8f405ecf108f0ed0cf4ea0ff8e712fce4"
    "15ffe118ffdd1cffda1fffd722ffd425ffd029ffcd2cffca2fffc732ffc336ffc039ffbd3cffba3fffb742ffb346ffb0"
    "49ffad4cffaa4fffa653ffa356ffa059ff9d5cff9a5fff9663ff9366ff9069ff8d6cff8970ff8673ff8376ff8079ff7d"
    "7cff7980ff7683ff7386ff7089ff6c8dff6990ff6693ff6396ff5f9aff5c9dff59a0ff56a3ff53a6ff4faaff4cadff49"
    "b0ff46b3ff42b7ff3fbaff3cbdff39c0ff36c3ff32c7ff2fcaff2ccdff29d0ff25d4ff22d7ff1fdaff1cddff18e0ff15"
    "e4ff12e7ff0feaff0cedff08f1fc05f4f802f7f400faf000feed00ffe900ffe500ffe200ffde00ffda00ffd700ffd300"
    "ffcf00ffcb00ffc800ffc400ffc000ffbd00ffb900ffb500ffb100ffae00ffaa00ffa600ffa300ff9f00ff9b00ff9800"
    "ff9400ff9000ff8c00ff8900ff8500ff8100ff7e00ff7a00ff7600ff7300ff6f00ff6b00ff6700ff6400ff6000ff5c00"
    "ff5900ff5500ff5100ff4d00ff4a00ff4600ff4200ff3f00ff3b00ff3700ff3400ff3000ff2c00ff2800ff2500ff2100"
    "ff1d00ff1a00ff1600fe1200fa0f00f50b00f10700ec0300e80000e30000de0000da0000d50000d10000cc0000c80000"
    "c30000bf0000ba0000b60000b10000ac0000a80000a300009f00009a00009600009100008d00008800008400007f0000"),
    dtype=np.uint8).reshape(256, 3)


# ---- cameras ---------------------------------------------------------------------------------------------------------
def make_view_camera(T_w2c, H: int, W: int, fx: float, fy: float, cx: float, cy: float, device="cpu"):
    """What the viewer reads of a camera: T (world -> camera), projection_matrix (as the rasteriser takes it), FoVx /
    FoVy, image_height / image_width and the intrinsics."""
    T = torch.as_tensor(T_w2c).detach().to(device, torch.float32).contiguous()
    P = projection_matrix2(0.01, 100.0, cx, cy, fx, fy, W, H).t().contiguous().to(device)
    return SimpleNamespace(T=T, projection_matrix=P, FoVx=2 * math.atan(W / (2 * fx)), FoVy=2 * math.atan(H / (2 * fy)),
                           image_height=int(H), image_width=int(W), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy))


def frustum_points(pose_c2w: torch.Tensor, size: float) -> torch.Tensor:
    """The five points of create_frustum (gui_utils.py:52-66) in the world: [5,3]."""
    pose = pose_c2w.detach().to(torch.float64).cpu()
    pts = torch.tensor(FRUSTUM_POINTS, dtype=torch.float64) * size
    return pts @ pose[:3, :3].t() + pose[:3, 3]


def follow_camera(T, H: int, W: int, fov_y: float, size: float = 0.02, behind: bool = True, device=None):
    """The camera of Frustum.view_dir_behind / view_dir (gui_utils.py:24-45) for the tracked world -> camera pose T:
    eye = pose (0, -2.5, -30) size (or the camera centre), looking at the mean of the frustum's four far points with
    up = p2 - p4.  Square pixels from fov_y, principal point at the image centre."""
    T = torch.as_tensor(T).detach()
    dev = T.device if device is None else device
    pose = torch.linalg.inv(T.to(torch.float64).cpu())
    pts = frustum_points(pose, size)
    base = torch.tensor([0.0, -2.5, -30.0] if behind else [0.0, 0.0, 0.0], dtype=torch.float64) * size
    eye = pose[:3, :3] @ base + pose[:3, 3]
    center = pts[1:].mean(dim=0)
    up = pts[2] - pts[4]
    fwd = (center - eye) / (center - eye).norm()
    right = torch.linalg.cross(fwd, up)
    right = right / right.norm()
    down = -torch.linalg.cross(right, fwd)
    R = torch.stack([right, down, fwd])              # rows: the camera's axes in the world = world -> camera rotation
    Tv = torch.eye(4, dtype=torch.float64)
    Tv[:3, :3] = R
    Tv[:3, 3] = -R @ eye
    f = H / (2.0 * math.tan(0.5 * fov_y))
    return make_view_camera(Tv, H, W, f, f, 0.5 * W, 0.5 * H, dev)


# ---- mirrors: colour map, time tint ----------------------------------------------------------------------------------
def _lut(device) -> torch.Tensor:
    return torch.from_numpy(JET_LUT.copy()).to(device)


def lut_index(t: torch.Tensor) -> torch.Tensor:
    """min(255, int(clamp(t, 0, 1) * 256)); NaN -> 0 (the callers blacken those pixels)."""
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t).clamp(0.0, 1.0)
    return (t * 256.0).to(torch.int64).clamp_max(255)


def compose_torch(src: torch.Tensor, mode: str) -> torch.Tensor:
    """Mirror of mgs_view_compose: [3,H,W] (rgb) or [1,H,W] / [H,W] (depth, opacity) fp32 -> uint8 [H,W,3]."""
    src = src.detach().to(torch.float32)
    if mode == "rgb":
        x = torch.where(torch.isnan(src), torch.zeros_like(src), src).clamp(0.0, 1.0)
        return (x * 255.0).to(torch.uint8).permute(1, 2, 0).contiguous()
    if mode not in ("depth", "opacity"):
        raise ValueError(f"compose_torch: mode {mode!r}")
    v = src.reshape(src.shape[-2], src.shape[-1])
    lo = DEPTH_LO if mode == "depth" else 0.0
    mx = torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp_min(0.0).max()
    lo_t = torch.tensor(lo, dtype=torch.float32, device=v.device)
    flat = torch.where(torch.isnan(v), v, torch.zeros_like(v))
    t = torch.where(mx > lo_t, (v - lo_t) / (mx - lo_t), flat)
    out = _lut(v.device)[lut_index(t)]
    out[torch.isnan(t)] = 0
    return out.contiguous()


def time_colors_torch(features: torch.Tensor, kf_ids: torch.Tensor) -> torch.Tensor:
    """Mirror of mgs_view_time_colors (slam_gui.py:550-558): 0.1 features + 0.9 jet(t) / 255 on every coefficient row."""
    f = features.detach().to(torch.float32)
    ids = kf_ids.detach().to(torch.int64).reshape(-1)
    lo, hi = ids.min(), ids.max()
    span = (hi - lo).to(torch.float32)
    t = torch.where(hi > lo, (ids - lo).to(torch.float32) / span, torch.zeros_like(ids, dtype=torch.float32))
    jet = _lut(f.device)[lut_index(t)].to(torch.float32) / torch.tensor(255.0, device=f.device)
    return 0.1 * f + (0.9 * jet)[:, None, :]


# ---- mirrors: line overlay -------------------------------------------------------------------------------------------
def overlay_segments(keyframes=None, current=None, trajectory=None, frustum_size: float = 0.02, device="cpu"):
    """(poses [K,4,4], pose colours [K,3], free segments [M,2,3], free colours [M,3]) in the overlay's index order:
    the keyframe frusta (blue), the current camera (green), then the trajectory's pieces (red) - later ones on top."""
    pal = _palette(str(device))              # rows: keyframe, current, trajectory (made once per device: no copy here)
    poses, pcol = [], []
    if keyframes is not None and len(keyframes) > 0:
        kf = torch.as_tensor(keyframes).detach().to(device, torch.float32).reshape(-1, 4, 4)
        poses.append(kf)
        pcol.append(pal[0:1].expand(kf.shape[0], 3))
    if current is not None:
        poses.append(torch.as_tensor(current).detach().to(device, torch.float32).reshape(1, 4, 4))
        pcol.append(pal[1:2])
    poses = torch.cat(poses).contiguous() if poses else torch.zeros(0, 4, 4, device=device)
    pcol = torch.cat(pcol).contiguous() if pcol else pal[:0]
    free = torch.zeros(0, 2, 3, device=device)
    if trajectory is not None and len(trajectory) > 1:
        tr = torch.as_tensor(trajectory).detach().to(device, torch.float32).reshape(-1, 3)
        free = torch.stack([tr[:-1], tr[1:]], dim=1).contiguous()
    return poses, pcol, free, pal[2:3].expand(free.shape[0], 3).contiguous()


@functools.lru_cache(maxsize=None)
def _palette(device: str) -> torch.Tensor:
    return torch.tensor([COLOR_KEYFRAME, COLOR_CURRENT, COLOR_TRAJECTORY], dtype=torch.uint8, device=device)


def world_segments(poses: torch.Tensor, free: torch.Tensor, frustum_size: float) -> torch.Tensor:
    """[8 K + M, 2, 3]: eight lines per camera -> world pose, then the free segments (same dtype as `poses`)."""
    pts = torch.tensor(FRUSTUM_POINTS, dtype=poses.dtype, device=poses.device) * frustum_size
    world = pts[None] @ poses[:, :3, :3].transpose(1, 2) + poses[:, None, :3, 3]          # [K,5,3]
    idx = torch.tensor(FRUSTUM_LINES, device=poses.device)
    segs = world[:, idx]                                                                   # [K,8,2,3]
    return torch.cat([segs.reshape(-1, 2, 3), free.to(poses.dtype).reshape(-1, 2, 3)])


def overlay_project_torch(segments: torch.Tensor, T_view: torch.Tensor, fx, fy, cx, cy, W: int, H: int,
                          near_z: float = NEAR_Z) -> torch.Tensor:
    """The project step of mgs_view_overlay in the dtype of `segments`: [S,2,3] world -> [S,5] int32 (x0, y0, x1, y1 in
    1/16 px, valid).  The same algorithm as the kernel (near clip, projection, Liang-Barsky against the guard rectangle),
    not the same roundings: the device's end points are the contract, this gives them to within a unit."""
    dt = segments.dtype
    T = T_view.detach().to(dt).cpu()
    out = torch.zeros(segments.shape[0], 5, dtype=torch.int32)
    for s, seg in enumerate(segments.detach().cpu()):
        v = seg @ T[:3, :3].t() + T[:3, 3]
        if not bool(torch.isfinite(v).all()) or (v[0, 2] < near_z and v[1, 2] < near_z):
            continue
        v = v.clone()
        for q in range(2):
            if v[q, 2] < near_z:
                t = (near_z - v[q, 2]) / (v[1 - q, 2] - v[q, 2])
                v[q] = v[q] + t * (v[1 - q] - v[q])
                v[q, 2] = near_z
        x = [float(fx * v[q, 0] / v[q, 2] + cx) for q in range(2)]
        y = [float(fy * v[q, 1] / v[q, 2] + cy) for q in range(2)]
        dx, dy = x[1] - x[0], y[1] - y[0]
        t0, t1, ok = 0.0, 1.0, True
        for p, q in ((-dx, x[0] + 0.5 * W), (dx, 1.5 * W - x[0]), (-dy, y[0] + 0.5 * H), (dy, 1.5 * H - y[0])):
            if p == 0.0:
                ok = ok and q >= 0.0
            else:
                r = q / p
                if p < 0.0:
                    ok = ok and r <= t1
                    t0 = max(t0, r)
                else:
                    ok = ok and r >= t0
                    t1 = min(t1, r)
            if not ok:
                break
        if not ok:
            continue
        x1, y1 = (x[0] + t1 * dx, y[0] + t1 * dy) if t1 < 1.0 else (x[1], y[1])
        x0, y0 = (x[0] + t0 * dx, y[0] + t0 * dy) if t0 > 0.0 else (x[0], y[0])
        out[s] = torch.tensor([round(16.0 * x0), round(16.0 * y0), round(16.0 * x1), round(16.0 * y1), 1], dtype=torch.int32)
    return out


def overlay_draw_torch(frame: torch.Tensor, endpoints: torch.Tensor, colors: torch.Tensor) -> torch.Tensor:
    """The draw step of mgs_view_overlay, integers only: returns a copy of uint8 [H,W,3] `frame` with every valid
    segment of `endpoints` [S,5] drawn in index order (so the highest index owns a shared pixel).  colors: [S,3]."""
    out = frame.clone()
    H, W = out.shape[0], out.shape[1]
    ep = endpoints.detach().to(torch.int64).cpu()
    for s in range(ep.shape[0]):
        X0, Y0, X1, Y1, valid = (int(v) for v in ep[s])
        if not valid:
            continue
        dx, dy = X1 - X0, Y1 - Y0
        n = (max(abs(dx), abs(dy)) + 15) >> 4
        if n > 2 * (W + H):
            continue
        k = torch.arange(n + 1, dtype=torch.int64)
        if n > 0:
            ox = torch.div(2 * dx * k + n, 2 * n, rounding_mode="floor")
            oy = torch.div(2 * dy * k + n, 2 * n, rounding_mode="floor")
        else:
            ox = oy = torch.zeros(1, dtype=torch.int64)
        px, py = (X0 + ox + 8) >> 4, (Y0 + oy + 8) >> 4
        keep = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        out[py[keep].to(out.device), px[keep].to(out.device)] = colors[s].to(out.device)
    return out


def segment_colors(pose_colors: torch.Tensor, free_colors: torch.Tensor) -> torch.Tensor:
    """[8 K + M, 3]: the colour of every segment in index order."""
    return torch.cat([pose_colors.repeat_interleave(8, dim=0), free_colors]).reshape(-1, 3)


# ---- mirrors: projection, brute-force first hit and blend (CPU route of view_frame_torch) ------------------------------
def project_torch(gaussians, camera, scale_modifier: float = 1.0, features: Optional[torch.Tensor] = None):
    """Per-Gaussian EWA projection as csrc/raster_math.h project_gaussian states it (degree-0 colour only): a dict of
    xy [N,2], conic [N,3], depth, opacity [N], rgb [N,3], visible [N] (near plane, determinant, tile rectangle)."""
    if int(getattr(gaussians, "active_sh_degree", 0)) != 0:
        raise NotImplementedError("project_torch evaluates degree-0 colour only")
    dt = torch.float32
    p = gaussians._xyz.detach().to(dt)
    dev = p.device
    s = torch.exp(gaussians._scaling.detach().to(dt)).expand(-1, 3) * scale_modifier
    q = torch.nn.functional.normalize(gaussians._rotation.detach().to(dt))
    o = torch.sigmoid(gaussians._opacity.detach().to(dt)).reshape(-1)
    f = (gaussians._features_dc if features is None else features).detach().to(dt)[:, 0, :]
    H, W = camera.image_height, camera.image_width
    T = camera.T.detach().to(dev, dt)
    V, PM = T.t(), T.t() @ camera.projection_matrix.detach().to(dev, dt)
    pv = p @ V[:3, :3] + V[3, :3]
    hom = torch.cat([p, torch.ones_like(p[:, :1])], dim=1) @ PM
    pw = 1.0 / (hom[:, 3] + 1e-7)
    xy = torch.stack([((hom[:, 0] * pw + 1.0) * W - 1.0) * 0.5, ((hom[:, 1] * pw + 1.0) * H - 1.0) * 0.5], dim=1)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    Sigma = L @ L.transpose(1, 2)
    tanx, tany = math.tan(0.5 * camera.FoVx), math.tan(0.5 * camera.FoVy)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    front = pv[:, 2] > 0.2
    tz = torch.where(front, pv[:, 2], torch.ones_like(pv[:, 2]))
    tx = (pv[:, 0] / tz).clamp(-1.3 * tanx, 1.3 * tanx) * tz
    ty = (pv[:, 1] / tz).clamp(-1.3 * tany, 1.3 * tany) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], dim=1).reshape(-1, 2, 3)
    M = J @ V[:3, :3].t()
    cov = M @ Sigma @ M.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    det_s = torch.where(det != 0, det, torch.ones_like(det))
    conic = torch.stack([c / det_s, -b / det_s, a / det_s], dim=1)
    mid = 0.5 * (a + c)
    lam = mid + torch.sqrt((mid * mid - det).clamp_min(0.1))
    rad = torch.ceil(3.0 * torch.sqrt(lam)).clamp(0, 1e7)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tile = lambda v, hi: torch.trunc(v / 16.0).clamp(0, hi)
    cxy = xy.clamp(-1e8, 1e8)
    rect = torch.stack([tile(cxy[:, 0] - rad, gx), tile(cxy[:, 1] - rad, gy),
                        tile(cxy[:, 0] + rad + 15, gx), tile(cxy[:, 1] + rad + 15, gy)], dim=1)       # tiles [min, max)
    area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    return {"xy": xy, "conic": conic, "depth": pv[:, 2], "opacity": o, "rgb": (SH_C0 * f + 0.5).clamp_min(0.0),
            "rect": rect, "visible": front & (det != 0) & (area > 0)}


def _sorted_alpha(proj, H: int, W: int, rows: slice, in_rect: bool = False):
    """The visible splats in stable depth order and their raw alpha o exp(power) at the pixels of `rows`: [n, P]."""
    vis = torch.nonzero(proj["visible"]).reshape(-1)
    order = torch.sort(proj["depth"][vis], stable=True).indices
    ids = vis[order]
    ys = torch.arange(rows.start, rows.stop, dtype=torch.float32, device=ids.device)
    xs = torch.arange(W, dtype=torch.float32, device=ids.device)
    PY, PX = (t.reshape(-1) for t in torch.meshgrid(ys, xs, indexing="ij"))
    dx = proj["xy"][ids, 0:1] - PX[None]
    dy = proj["xy"][ids, 1:2] - PY[None]
    con = proj["conic"][ids]
    power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
    raw = proj["opacity"][ids][:, None] * torch.exp(power)
    if in_rect:         # the rasteriser's binning: a splat only reaches the tiles of its 3-sigma rectangle
        rect, tx, ty = proj["rect"][ids], torch.floor(PX / 16.0)[None], torch.floor(PY / 16.0)[None]
        inside = (tx >= rect[:, 0:1]) & (tx < rect[:, 2:3]) & (ty >= rect[:, 1:2]) & (ty < rect[:, 3:4])
        raw = torch.where(inside, raw, torch.zeros_like(raw))
    return ids, power, raw


def first_hit_torch(proj, H: int, W: int, mode: str, bg: torch.Tensor, rows_per_chunk: int = 8):
    """Brute-force ellipsoid shader over ALL visible splats (no tiles): (colour [3,H,W], depth [1,H,W], id [H,W] or -1)."""
    thr = BALL_THRESHOLD[mode]
    dev = proj["xy"].device
    color = bg.to(dev, torch.float32).reshape(3, 1, 1).repeat(1, H, W)
    depth = torch.zeros(1, H, W, device=dev)
    hit_id = torch.full((H, W), -1, dtype=torch.int64, device=dev)
    for r0 in range(0, H, rows_per_chunk):
        rows = slice(r0, min(H, r0 + rows_per_chunk))
        ids, power, raw = _sorted_alpha(proj, H, W, rows)
        if ids.numel() == 0:
            continue
        a = raw.clamp_max(0.99)
        hit = (power <= 0) & (a >= 1.0 / 255.0) & (a > thr)
        any_hit = hit.any(dim=0)
        first = torch.argmax(hit.to(torch.int8), dim=0)                 # first True along the depth order
        cols = torch.arange(hit.shape[1], device=dev)
        g = ids[first]
        rgb = proj["rgb"][g]
        if mode == "gaussian_ball":
            rgb = rgb * torch.exp(power[first, cols])[:, None]
        n = rows.stop - rows.start
        sel = any_hit.reshape(n, W)
        color[:, rows][:, sel] = rgb.reshape(n, W, 3)[sel].t()
        depth[0, rows][sel] = proj["depth"][g].reshape(n, W)[sel]
        hit_id[rows][sel] = g.reshape(n, W)[sel]
    return color, depth, hit_id


def blend_torch(proj, H: int, W: int, bg: torch.Tensor, rows_per_chunk: int = 8):
    """Brute-force front-to-back blend over all visible splats with the rasteriser's rules (a splat reaches the tiles
    of its 3-sigma rectangle, alpha cap 0.99, skip below 1/255, stop before T (1 - alpha) < 1e-4): (colour [3,H,W], depth [1,H,W], opacity [1,H,W])."""
    dev = proj["xy"].device
    bg = bg.to(dev, torch.float32).reshape(3)
    color, depth, opac = torch.zeros(3, H, W, device=dev), torch.zeros(1, H, W, device=dev), torch.zeros(1, H, W, device=dev)
    for r0 in range(0, H, rows_per_chunk):
        rows = slice(r0, min(H, r0 + rows_per_chunk))
        ids, power, raw = _sorted_alpha(proj, H, W, rows, in_rect=True)
        n = rows.stop - rows.start
        if ids.numel() == 0:
            color[:, rows] = bg[:, None, None]
            continue
        a = raw.clamp_max(0.99)
        a = torch.where((power <= 0) & (a >= 1.0 / 255.0), a, torch.zeros_like(a))
        T_incl = torch.cumprod(1.0 - a, dim=0)
        alive = torch.cumprod((T_incl >= 1e-4).to(torch.float32), dim=0)       # nothing is blended behind the stop
        T_excl = torch.cat([torch.ones_like(T_incl[:1]), T_incl[:-1]])
        w = a * T_excl * alive
        T_fin = torch.prod(torch.where(alive > 0, 1.0 - a, torch.ones_like(a)), dim=0)
        color[:, rows] = (proj["rgb"][ids].t() @ w + T_fin[None] * bg[:, None]).reshape(3, n, W)
        depth[0, rows] = (proj["depth"][ids] @ w).reshape(n, W)
        opac[0, rows] = (1.0 - T_fin).reshape(n, W)
    return color, depth, opac


def view_frame_torch(mode: str = "rgb", *, color=None, depth=None, opacity=None, hit_color=None, gaussians=None,
                     camera=None, background=None, scale_modifier: float = 1.0, keyframes=None, current=None,
                     trajectory=None, frustum_size: float = 0.02, endpoints=None, median_depth=None, normal=None,
                     max_jump: float = 0.05) -> torch.Tensor:
    """The mirror of NativeViewer.frame.  Given the float planes of a forward (`color`, `depth`, `opacity`; `hit_color`
    for the two ball modes) it repeats the device's arithmetic byte for byte: compose_torch, then overlay_draw_torch on
    `endpoints` (the device's own [S,5] end points; without them they are projected here in fp64, which agrees with the
    device to within a unit).  Without planes it makes them from `gaussians` and `camera` by brute force (project_torch,
    blend_torch / first_hit_torch, the time tint through time_colors_torch) - the CPU route.  The two SURFACE_MODES take
    `median_depth` (the jet composition of the depth mode) and `normal` (0.5 n + 0.5 as rgb; without it the normals of
    `median_depth` through surface.depth_normal_torch, for which `camera` gives the intrinsics)."""
    if mode not in MODES + SURFACE_MODES:
        raise ValueError(f"mode must be one of {MODES + SURFACE_MODES}, got {mode!r}")
    ball = mode in BALL_THRESHOLD
    plane = {"rgb": color, "time": color, "depth": depth, "opacity": opacity}.get(mode, hit_color)
    if mode in SURFACE_MODES:
        from . import surface
        if median_depth is None and (mode == "median_depth" or normal is None):
            if gaussians is None or camera is None:
                raise ValueError("view_frame_torch needs the surface planes or (gaussians, camera)")
            proj = project_torch(gaussians, camera, scale_modifier)
            median_depth = surface.median_depth_torch(proj, camera.image_height, camera.image_width)[0]
        if mode == "normal":
            if normal is None:
                if camera is None:
                    raise ValueError("view_frame_torch: the normals of a median plane need `camera`")
                normal = surface.depth_normal_torch(median_depth, camera.fx, camera.fy, camera.cx, camera.cy, 0.5, max_jump)
            plane = surface.normal_rgb_torch(normal)
        else:
            plane = median_depth
    if plane is None:
        if gaussians is None or camera is None:
            raise ValueError("view_frame_torch needs the forward's planes or (gaussians, camera)")
        H, W = camera.image_height, camera.image_width
        bg = torch.zeros(3) if background is None else background
        feats = None
        if mode == "time":
            feats = time_colors_torch(torch.cat((gaussians._features_dc, gaussians._features_rest), dim=1),
                                      gaussians.unique_kfIDs)
        proj = project_torch(gaussians, camera, scale_modifier, feats)
        if ball:
            plane = first_hit_torch(proj, H, W, mode, bg)[0]
        else:
            c, d, o = blend_torch(proj, H, W, bg)
            plane = {"rgb": c, "time": c, "depth": d, "opacity": o}[mode]
    frame = compose_torch(plane, {"depth": "depth", "median_depth": "depth", "opacity": "opacity"}.get(mode, "rgb"))
    if keyframes is None and current is None and trajectory is None:
        return frame
    poses, pcol, free, fcol = overlay_segments(keyframes, current, trajectory, frustum_size, device="cpu")
    if endpoints is None:
        if camera is None:
            raise ValueError("view_frame_torch: the overlay needs `camera` or the device's `endpoints`")
        segs = world_segments(poses.double(), free.double(), frustum_size)
        endpoints = overlay_project_torch(segs, camera.T.double(), camera.fx, camera.fy, camera.cx - 0.5, camera.cy - 0.5,
                                          frame.shape[1], frame.shape[0])
    return overlay_draw_torch(frame, endpoints, segment_colors(pcol, fcol))


def save_frame(path: str, frame) -> str:
    """Writes a uint8 [H,W,3] frame: PNG through PIL when it is importable (and the path does not end in .ppm), else a
    binary PPM (P6) next to the requested name.  Returns the path written."""
    a = frame.detach().cpu().numpy() if isinstance(frame, torch.Tensor) else np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"save_frame: expected uint8 [H,W,3], got {a.dtype} {a.shape}")
    a = np.ascontiguousarray(a)
    if not path.lower().endswith(".ppm"):
        try:
            from PIL import Image
        except ImportError:
            path = path.rsplit(".", 1)[0] + ".ppm" if "." in path.rsplit("/", 1)[-1] else path + ".ppm"
        else:
            Image.fromarray(a).save(path)
            return path
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        fh.write(a.tobytes())
    return path


# ---- the device path -------------------------------------------------------------------------------------------------
class NativeViewer:
    """Frames of one map on the device.  frame() activates the map as it is now (mgs_map_activate), runs the forward
    (or mgs_view_ellipsoid) at a fixed pair capacity, composes the chosen plane into a new uint8 [H,W,3] tensor and
    draws the overlay - all enqueued on the current stream, nothing read back.  The planes of the last call stay in
    `color`, `depth`, `opacity`, `hit_color`, `hit_depth` (and, after surface(), `median_depth`, `median_index`,
    `normal`), the overlay's end points in `endpoints` (tests compare the mirror on them).  check_capacity() is the one
    synchronising call: True when no frame so far exceeded the pair capacity; otherwise the capacity is grown for the
    frames to come and the affected frames have to be taken again."""

    def __init__(self, gaussians, background, H: int, W: int, device, capacity: Optional[int] = None,
                 capacity_margin: float = 1.5):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("NativeViewer runs on the GPU only (HIP kernels, gfx950); view_frame_torch is the CPU route")
        self.gaussians, self.H, self.W = gaussians, int(H), int(W)
        L = _cabi.lib()
        if L.mgs_view_overlay_scratch_bytes(self.W, self.H) == 0:
            raise ValueError(f"NativeViewer: unsupported size {self.H} x {self.W}")
        dev = self.dev
        self.bg = background.detach().to(dev, torch.float32).reshape(-1).contiguous()
        self.lut = _lut(dev).contiguous()
        self.view_m, self.full_m = torch.empty(4, 4, device=dev), torch.empty(4, 4, device=dev)
        self.color, self.hit_color = torch.empty(3, H, W, device=dev), torch.empty(3, H, W, device=dev)
        self.depth, self.opacity = torch.empty(1, H, W, device=dev), torch.empty(1, H, W, device=dev)
        self.hit_depth = torch.empty(1, H, W, device=dev)
        self.median_depth = self.median_index = self.normal = None      # made by the first surface()
        self.compose_scratch = torch.empty(int(L.mgs_view_compose_scratch_bytes()), dtype=torch.uint8, device=dev)
        self.time_scratch = torch.empty(int(L.mgs_view_time_colors_scratch_bytes()), dtype=torch.uint8, device=dev)
        self.owner = torch.empty(int(L.mgs_view_overlay_scratch_bytes(self.W, self.H)), dtype=torch.uint8, device=dev)
        self.pair_max = torch.zeros(1, dtype=torch.int32, device=dev)
        self.capacity = 0 if capacity is None else max(1024, int(capacity))
        self.capacity_margin = capacity_margin
        self.endpoints = None
        self._N, self.K, self._cap_alloc, self._geom_key = -1, -1, 0, None
        self._keep = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _activate(self):
        g, dev = self.gaussians, self.dev
        N = int(g._xyz.shape[0])
        if N < 1:
            raise RuntimeError("NativeViewer: the map is empty")
        K = int(g._features_dc.shape[1] + g._features_rest.shape[1])
        if (N, K) != (self._N, self.K):
            self.scales, self.rots = torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev)
            self.opac = torch.empty(N, device=dev)
            self.shs = torch.empty(N, K, 3, device=dev)
            self.tinted = torch.empty(N, K, 3, device=dev)
            self.radii = torch.empty(N, dtype=torch.int32, device=dev)
            self.n_touched = torch.empty(N, dtype=torch.int32, device=dev)
        self._N, self.K = N, K
        if self.capacity == 0:
            self.capacity = max(65536, (16 * N + 1023) // 1024 * 1024)
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        p = self._params = {k: f32(getattr(g, k)) for k in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc",
                                                            "_features_rest")}
        a = _cabi.MapActivateArgs()
        a.num_gaussians, a.scale_dims, a.sh_coeffs = N, int(g._scaling.shape[1]), K
        a.log_scales, a.raw_rotations = p["_scaling"].data_ptr(), p["_rotation"].data_ptr()
        a.opacity_logits, a.features_dc = p["_opacity"].data_ptr(), p["_features_dc"].data_ptr()
        a.features_rest = p["_features_rest"].data_ptr() if K > 1 else None
        a.scales, a.rotations, a.opacities = self.scales.data_ptr(), self.rots.data_ptr(), self.opac.data_ptr()
        a.shs = self.shs.data_ptr() if K > 1 else None
        _cabi.check(_cabi.lib().mgs_map_activate(C.byref(a), self._stream()), "mgs_map_activate")
        return p["_features_dc"] if K == 1 else self.shs

    def _ensure_workspaces(self, deg):
        key = (self._N, self.K, deg)
        if key != self._geom_key:
            sizes = _cabi.workspace_sizes(_cabi.RasterShape(self._N, self.W, self.H, deg, self.K, 1024, 1.0, 1.0, 1.0))
            self.geom = torch.empty(int(sizes.geom_bytes), dtype=torch.uint8, device=self.dev)
            self._geom_key = key
        if self._cap_alloc != self.capacity:
            sizes = _cabi.workspace_sizes(_cabi.RasterShape(self._N, self.W, self.H, deg, self.K, self.capacity, 1.0, 1.0,
                                                            1.0))
            self.bins = torch.empty(int(sizes.bins_bytes), dtype=torch.uint8, device=self.dev)
            self._cap_alloc = self.capacity

    def _forward_args(self, f, camera, shs, scale_modifier, T, proj):
        deg = int(getattr(self.gaussians, "active_sh_degree", 0))
        self._ensure_workspaces(deg)
        p = self._params
        f.shape = _cabi.RasterShape(self._N, self.W, self.H, deg, self.K, self.capacity,
                                    math.tan(0.5 * camera.FoVx), math.tan(0.5 * camera.FoVy), float(scale_modifier))
        f.means3D, f.scales, f.rotations = p["_xyz"].data_ptr(), self.scales.data_ptr(), self.rots.data_ptr()
        f.opacities, f.shs = self.opac.data_ptr(), shs.data_ptr()
        f.viewmatrix, f.projmatrix, f.projmatrix_raw = self.view_m.data_ptr(), self.full_m.data_ptr(), proj.data_ptr()
        f.campos, f.bg = self.view_m.data_ptr(), self.bg.data_ptr()      # camera_center as render() passes it
        f.geom, f.bins = self.geom.data_ptr(), self.bins.data_ptr()
        f.out_color, f.out_depth, f.out_opacity = self.color.data_ptr(), self.depth.data_ptr(), self.opacity.data_ptr()
        f.radii, f.n_touched = self.radii.data_ptr(), self.n_touched.data_ptr()
        f.pair_count_max = self.pair_max.data_ptr()

    def time_colors(self, features: torch.Tensor, kf_ids: torch.Tensor, out: Optional[torch.Tensor] = None):
        """mgs_view_time_colors: [N,K,3] tinted coefficients of `features` into `out` (the viewer's scratch by default)."""
        N, K = int(features.shape[0]), int(features.shape[1])
        out = torch.empty(N, K, 3, device=self.dev) if out is None else out
        ids = kf_ids.detach().to(self.dev, torch.int32).contiguous()
        a = _cabi.ViewTimeColorsArgs()
        a.num_gaussians, a.sh_coeffs = N, K
        a.features, a.kf_ids, a.lut = features.data_ptr(), ids.data_ptr(), self.lut.data_ptr()
        a.out, a.scratch = out.data_ptr(), self.time_scratch.data_ptr()
        _cabi.check(_cabi.lib().mgs_view_time_colors(C.byref(a), self._stream()), "mgs_view_time_colors")
        self._keep_ids = ids
        return out

    def compose(self, src: torch.Tensor, mode: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mgs_view_compose of a float plane of this viewer's size: uint8 [H,W,3]."""
        out = torch.empty(self.H, self.W, 3, dtype=torch.uint8, device=self.dev) if out is None else out
        a = _cabi.ViewComposeArgs()
        a.width, a.height = self.W, self.H
        a.mode = {"rgb": _cabi.VIEW_RGB, "depth": _cabi.VIEW_DEPTH, "opacity": _cabi.VIEW_OPACITY}[mode]
        a.src, a.lut, a.out, a.scratch = src.data_ptr(), self.lut.data_ptr(), out.data_ptr(), self.compose_scratch.data_ptr()
        _cabi.check(_cabi.lib().mgs_view_compose(C.byref(a), self._stream()), "mgs_view_compose")
        return out

    def overlay(self, frame: torch.Tensor, camera, keyframes=None, current=None, trajectory=None,
                frustum_size: float = 0.02) -> torch.Tensor:
        """mgs_view_overlay into `frame` (in place); the end points stay in self.endpoints."""
        poses, pcol, free, fcol = overlay_segments(keyframes, current, trajectory, frustum_size, device=self.dev)
        S = 8 * int(poses.shape[0]) + int(free.shape[0])
        if S == 0:
            self.endpoints = torch.zeros(0, 5, dtype=torch.int32, device=self.dev)
            return frame
        self.endpoints = torch.empty(S, 5, dtype=torch.int32, device=self.dev)
        T = camera.T.detach().to(self.dev, torch.float32).contiguous()
        a = _cabi.ViewOverlayArgs()
        a.width, a.height, a.num_poses, a.num_free = self.W, self.H, int(poses.shape[0]), int(free.shape[0])
        # the rasteriser puts pixel i's centre at i + 0.5 of the intrinsics' frame (synthetic.projection_matrix2)
        a.fx, a.fy, a.cx, a.cy = camera.fx, camera.fy, camera.cx - 0.5, camera.cy - 0.5
        a.frustum_size, a.near_z = float(frustum_size), NEAR_Z
        a.T_view = T.data_ptr()
        a.poses = poses.data_ptr() if poses.shape[0] else None
        a.free_segments = free.data_ptr() if free.shape[0] else None
        a.pose_colors = pcol.data_ptr() if poses.shape[0] else None
        a.free_colors = fcol.data_ptr() if free.shape[0] else None
        a.endpoints, a.frame, a.scratch = self.endpoints.data_ptr(), frame.data_ptr(), self.owner.data_ptr()
        _cabi.check(_cabi.lib().mgs_view_overlay(C.byref(a), self._stream()), "mgs_view_overlay")
        self._keep = (T, poses, pcol, free, fcol)           # alive until the next call: the work is only enqueued
        return frame

    def frame(self, camera, mode: str = "rgb", scale_modifier: float = 1.0, keyframes=None, current=None,
              trajectory=None, frustum_size: float = 0.02) -> torch.Tensor:
        """One finished frame: uint8 [H,W,3] on the device.  `camera`: T (world -> camera), projection_matrix, FoVx,
        FoVy, image_height / image_width (and fx, fy, cx, cy for the overlay) - a ViewCamera, make_view_camera() or
        follow_camera().  keyframes [K,4,4] / current [4,4]: camera -> world poses; trajectory [M,3]: world points."""
        if mode not in MODES + SURFACE_MODES:
            raise ValueError(f"mode must be one of {MODES + SURFACE_MODES}, got {mode!r}")
        L = _cabi.lib()
        if mode in SURFACE_MODES:
            self.surface(camera, normals=mode == "normal", scale_modifier=scale_modifier)
            if mode == "normal":                     # 0.5 n + 0.5: an exact product and one rounding, as the mirror
                out = self.compose(torch.add(torch.mul(self.normal, 0.5), 0.5), "rgb")
            else:
                out = self.compose(self.median_depth, "depth")
            if keyframes is not None or current is not None or trajectory is not None:
                self.overlay(out, camera, keyframes, current, trajectory, frustum_size)
            return out
        shs, T, proj = self._prepare(camera, mode)
        if mode in BALL_THRESHOLD:
            a = _cabi.ViewEllipsoidArgs()
            self._forward_args(a.fwd, camera, shs, scale_modifier, T, proj)
            a.mode = _cabi.VIEW_FLAT_BALL if mode == "flat_ball" else _cabi.VIEW_GAUSSIAN_BALL
            a.hit_color, a.hit_depth = self.hit_color.data_ptr(), self.hit_depth.data_ptr()
            _cabi.check(L.mgs_view_ellipsoid(C.byref(a), self._stream()), "mgs_view_ellipsoid")
            out = self.compose(self.hit_color, "rgb")
        else:
            f = _cabi.ForwardArgs()
            self._forward_args(f, camera, shs, scale_modifier, T, proj)
            _cabi.check(L.mgs_raster_forward_project(C.byref(f), self._stream()), "mgs_raster_forward_project")
            _cabi.check(L.mgs_raster_forward_blend(C.byref(f), self._stream()), "mgs_raster_forward_blend")
            plane = {"depth": self.depth, "opacity": self.opacity}.get(mode, self.color)
            out = self.compose(plane, mode if mode in ("depth", "opacity") else "rgb")
        if keyframes is not None or current is not None or trajectory is not None:
            self.overlay(out, camera, keyframes, current, trajectory, frustum_size)
        return out

    def _prepare(self, camera, mode: str = "rgb"):
        """Activates the map and makes the camera's matrices on the device: (shs, T, projection)."""
        if int(camera.image_height) != self.H or int(camera.image_width) != self.W:
            raise ValueError(f"camera is {camera.image_height} x {camera.image_width}, viewer {self.H} x {self.W}")
        shs = self._activate()
        if mode == "time":
            shs = self.time_colors(shs, self.gaussians.unique_kfIDs, self.tinted)
        f32 = lambda t: t.detach().to(self.dev, torch.float32).contiguous()
        T, proj = f32(camera.T), f32(camera.projection_matrix)
        self._keep_cam = (T, proj)
        _cabi.check(_cabi.lib().mgs_camera_from_pose(T.data_ptr(), proj.data_ptr(), self.view_m.data_ptr(),
                                                     self.full_m.data_ptr(), self._stream()), "mgs_camera_from_pose")
        return shs, T, proj

    def depth_normal(self, depth: torch.Tensor, fx, fy, cx, cy, pixel_center: float = 0.5, max_jump: float = 0.05,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mgs_depth_normal of a contiguous fp32 depth plane of this viewer's size on the device: [3,H,W]."""
        if depth.device != self.dev or depth.dtype != torch.float32 or not depth.is_contiguous() or \
                depth.numel() != self.H * self.W:
            raise ValueError(f"depth_normal: depth must be a contiguous fp32 plane of {self.H} x {self.W} on {self.dev}")
        out = torch.empty(3, self.H, self.W, device=self.dev) if out is None else out
        a = _cabi.DepthNormalArgs()
        a.width, a.height = self.W, self.H
        a.fx, a.fy, a.cx, a.cy = float(fx), float(fy), float(cx), float(cy)
        a.pixel_center, a.max_jump = float(pixel_center), float(max_jump)
        a.depth, a.normal = depth.data_ptr(), out.data_ptr()
        _cabi.check(_cabi.lib().mgs_depth_normal(C.byref(a), self._stream()), "mgs_depth_normal")
        return out

    def surface(self, camera, normals: bool = True, max_jump: float = 0.05, scale_modifier: float = 1.0) -> dict:
        """The surface planes of one view (mgs_surface_forward, then mgs_depth_normal on the median plane with this
        rasteriser's pixel centre 0.5): `color`, `depth`, `opacity` exactly as frame("rgb") leaves them, `median_depth`
        [1,H,W] (0 where the transmittance never falls to one half), `median_index` [H,W] int32 (-1 there) and, with
        `normals`, `normal` [3,H,W] in the camera frame (needs the camera's fx, fy, cx, cy).  Enqueued on the current
        stream, nothing read back; the planes stay on the viewer and are returned as a dict.  check_capacity() tells
        afterwards whether the pair capacity held, as for frame()."""
        shs, T, proj = self._prepare(camera)
        if self.median_depth is None:
            self.median_depth = torch.empty(1, self.H, self.W, device=self.dev)
            self.median_index = torch.empty(self.H, self.W, dtype=torch.int32, device=self.dev)
            self.normal = torch.empty(3, self.H, self.W, device=self.dev)
        a = _cabi.SurfaceArgs()
        self._forward_args(a.fwd, camera, shs, scale_modifier, T, proj)
        a.median_depth, a.median_index = self.median_depth.data_ptr(), self.median_index.data_ptr()
        _cabi.check(_cabi.lib().mgs_surface_forward(C.byref(a), self._stream()), "mgs_surface_forward")
        out = {"color": self.color, "depth": self.depth, "opacity": self.opacity, "median_depth": self.median_depth,
               "median_index": self.median_index}
        if normals:
            self.depth_normal(self.median_depth, camera.fx, camera.fy, camera.cx, camera.cy, 0.5, max_jump, self.normal)
            out["normal"] = self.normal
        return out

    def check_capacity(self) -> bool:
        """Synchronises.  False when a frame since the last check held more (tile, Gaussian) pairs than the capacity:
        the capacity is then grown, and frames taken since the last check are incomplete."""
        seen = int(self.pair_max.item())
        self.pair_max.zero_()
        if seen <= self.capacity:
            return True
        self.capacity = (int(seen * self.capacity_margin) + 1023) // 1024 * 1024
        return False
