"""Surface planes: the median depth of a view and the normals of a depth plane (csrc/surface.hip through the C ABI;
the contracts are in include/monogs_raster.h and DESIGN.md "Surface planes").

  viewer.NativeViewer.surface(camera)    colour / depth / opacity of the forward plus median_depth, median_index and
                                         normal, on the device; tsdf.fuse_map(..., depth_mode="median") fuses them
  median_depth_torch(proj, H, W)         the mirror of the median walk on viewer.project_torch's projection
  depth_normal_torch(depth, ...)         the mirror of mgs_depth_normal: the same single fp32 roundings in the same
                                         order, so the device's normals equal its output bit for bit; runs anywhere

The median depth of a pixel is the view depth of the splat at which the transmittance falls through one half, walking
the tile's list front to back with the blend's rules; 0 (index -1) where it never does.  At a silhouette it is the
depth of ONE of the two surfaces, where the blend's depth / opacity lies between them."""
from __future__ import annotations

import torch

from . import viewer as _viewer


def median_depth_torch(proj, H: int, W: int, rows_per_chunk: int = 8):
    """Brute-force median walk over all visible splats of `proj` (viewer.project_torch) with the rasteriser's rules (a
    splat reaches the tiles of its 3-sigma rectangle, power <= 0, alpha = min(0.99, o exp(power)) >= 1/255):
    (median depth [1,H,W], 0 where T never reaches one half; median index [H,W] int64, -1 there)."""
    dev = proj["xy"].device
    depth = torch.zeros(1, H, W, device=dev)
    index = torch.full((H, W), -1, dtype=torch.int64, device=dev)
    for r0 in range(0, H, rows_per_chunk):
        rows = slice(r0, min(H, r0 + rows_per_chunk))
        ids, power, raw = _viewer._sorted_alpha(proj, H, W, rows, in_rect=True)
        if ids.numel() == 0:
            continue
        a = raw.clamp_max(0.99)
        counts = (power <= 0) & (a >= 1.0 / 255.0)
        T_incl = torch.cumprod(1.0 - torch.where(counts, a, torch.zeros_like(a)), dim=0)
        cross = counts & (T_incl <= 0.5)
        found = cross.any(dim=0)
        g = ids[torch.argmax(cross.to(torch.int8), dim=0)]               # first True along the depth order
        n = rows.stop - rows.start
        sel = found.reshape(n, W)
        depth[0, rows][sel] = proj["depth"][g].reshape(n, W)[sel]
        index[rows][sel] = g.reshape(n, W)[sel]
    return depth, index


def depth_normal_torch(depth, fx, fy, cx, cy, pixel_center: float = 0.5, max_jump: float = 0.05) -> torch.Tensor:
    """mgs_depth_normal in fp32 torch (any device): camera-frame unit normals [3,H,W] of depth [H,W] (or [1,H,W]) by
    central differences of the back-projected neighbours, (0,0,0) on the border, next to an invalid depth (not > 0 or
    not finite) and across a depth step above max_jump * depth.  Every product, sum, difference, quotient and root
    is one torch operation, i.e. one rounding.  pixel_center: 0.5 for this rasteriser's planes, 0 for sensor planes."""
    d = torch.as_tensor(depth).detach().to(torch.float32)
    H, W = (int(v) for v in d.shape[-2:])
    d = d.reshape(H, W)
    dev = d.device
    out = torch.zeros(3, H, W, device=dev)
    if H < 3 or W < 3:
        return out
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)
    rx = ((torch.arange(W, dtype=torch.float32, device=dev) + f(pixel_center)) - f(cx)) / f(fx)
    ry = ((torch.arange(H, dtype=torch.float32, device=dev) + f(pixel_center)) - f(cy)) / f(fy)
    dc, dl, dr, du, dd = d[1:-1, 1:-1], d[1:-1, :-2], d[1:-1, 2:], d[:-2, 1:-1], d[2:, 1:-1]
    valid = lambda t: (t > 0) & torch.isfinite(t)
    jump = f(max_jump) * dc
    ok = valid(dc)
    for t in (dl, dr, du, dd):
        ok = ok & valid(t) & ((t - dc).abs() <= jump)
    x0, xl, xr = rx[None, 1:-1], rx[None, :-2], rx[None, 2:]
    y0, yu, yd = ry[1:-1, None], ry[:-2, None], ry[2:, None]
    ax, ay, az = xr * dr - xl * dl, y0 * dr - y0 * dl, dr - dl
    bx, by, bz = x0 * dd - x0 * du, yd * dd - yu * du, dd - du
    nx, ny, nz = by * az - bz * ay, bz * ax - bx * az, bx * ay - by * ax
    # the correctly rounded fp32 root: torch's vectorised fp32 sqrt on the CPU is an ulp off at ~1 % of its arguments,
    # and the fp64 root rounded to fp32 is the correctly rounded one (53 >= 2 * 24 + 2 bits: no double rounding)
    length = torch.sqrt(((nx * nx + ny * ny) + nz * nz).double()).float()
    ok = ok & (length > 0) & torch.isfinite(length)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    for c, comp in enumerate((nx, ny, nz)):
        out[c, 1:-1, 1:-1] = torch.where(ok, comp / length, zero)
    return out


def normal_rgb_torch(normal: torch.Tensor) -> torch.Tensor:
    """0.5 n + 0.5 as an rgb plane [3,H,W] (the product is exact, the sum one rounding): what the viewer's `normal`
    mode composes.  A pixel without a normal is mid-grey."""
    return 0.5 * normal.detach().to(torch.float32) + 0.5
