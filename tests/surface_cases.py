"""Scenes and the fp64 reference of the surface-plane tests (test_cpu_surface.py, test_gpu_surface.py).

median_oracle(name): a brute-force fp64 median walk over oracle.torch_raster.project - stable depth order, ties by
index, a splat reaches only the tiles of its rectangle - evaluated three times: at nominal, at a "more opaque" extreme
(alpha x (1 + 1e-4), alpha cut 1/255 - 2e-4, crossing at 0.5 + 2e-4) and at the mirror-image "less opaque" extreme.  The
crossing index is monotone in these perturbations, so a pixel at which both extremes name the Gaussian nominal names
has that median for every fp32 evaluation inside the band; the other pixels are left out of a comparison.  1e-4 / 2e-4
are the viewer test's band (the fp32 exponent and exp differ from the fp64 ones by ~1e-5 relative)."""
import functools

import torch

from conftest import oracle_settings

REL, BAND, CAP = 1e-4, 2e-4, 0.02
Z_FRONT, Z_BACK = 1.0, 2.0


def deep_scene(W=70, H=45, seed=21):
    """A sparse scene plus, inside tile (1, 1): 140 near, SMALL Gaussians of moderate opacity (a pixel is under a few of
    them only, so its transmittance stays above one half while the list goes by) in front of 30 large opaque ones that
    cover part of the tile - the tile's list is longer than the 64-splat staging chunk, pixels under an opaque splat
    cross behind position 64, and the pixels no opaque splat covers never cross."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(40, W, H, seed=seed)
    cam = sc.cam
    g = torch.Generator().manual_seed(seed + 1)

    def cluster(n, z0, z1, sig_px, logit0, logit1, u0, u1):
        u = u0 + (u1 - u0) * torch.rand(n, generator=g)
        v = 17.0 + 13.0 * torch.rand(n, generator=g)
        z = z0 + (z1 - z0) * torch.rand(n, generator=g)
        xyz = torch.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], dim=1)
        sig = sig_px * torch.exp(0.2 * torch.randn(n, generator=g))
        ls = torch.log((sig * z / cam.fx)[:, None] * torch.exp(0.2 * torch.randn(n, 3, generator=g)))
        rot = torch.nn.functional.normalize(torch.randn(n, 4, generator=g))
        op = logit0 + (logit1 - logit0) * torch.rand(n, 1, generator=g)
        fdc = ((torch.rand(n, 3, generator=g) - 0.5) / S.SH_C0)[:, None, :]
        return xyz, ls, rot, op, fdc

    parts = [cluster(140, 0.6, 0.9, 0.7, -1.5, -0.5, 17.0, 30.0), cluster(30, 3.0, 4.0, 1.6, 3.0, 3.5, 17.0, 25.0)]
    cat = lambda i, base: torch.cat([base] + [p[i] for p in parts]).contiguous()
    return sc._replace(means3D=cat(0, sc.means3D), log_scales=cat(1, sc.log_scales), rot=cat(2, sc.rot),
                       opacity_logit=cat(3, sc.opacity_logit), features_dc=cat(4, sc.features_dc))


def two_layer_scene(W=70, H=45):
    """Two fronto-parallel layers of near-opaque isotropic Gaussians (sigma 1.5 px on a 2 px lattice) with centres
    exactly at Z_FRONT and Z_BACK; the back layer covers the image, the front layer its left half.  Along the front
    layer's edge the blend mixes the two depths; the median is one or the other."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(1, W, H, seed=5)
    cam = sc.cam
    parts = []
    for z, u_hi in ((Z_FRONT, 0.5 * W), (Z_BACK, W + 4.0)):
        u = torch.arange(-4.0, u_hi, 2.0)
        v = torch.arange(-4.0, H + 4.0, 2.0)
        vv, uu = (t.reshape(-1) for t in torch.meshgrid(v, u, indexing="ij"))
        zz = torch.full_like(uu, z)
        parts.append((torch.stack([(uu - cam.cx) * z / cam.fx, (vv - cam.cy) * z / cam.fy, zz], dim=1),
                      torch.full((uu.numel(), 3), 1.5 * z / cam.fx).log()))
    xyz = torch.cat([p[0] for p in parts]).contiguous()
    n = xyz.shape[0]
    g = torch.Generator().manual_seed(6)
    rot = torch.zeros(n, 4)
    rot[:, 0] = 1.0
    fdc = ((torch.rand(n, 3, generator=g) - 0.5) / S.SH_C0)[:, None, :].contiguous()
    return sc._replace(means3D=xyz, log_scales=torch.cat([p[1] for p in parts]).contiguous(), rot=rot,
                       opacity_logit=torch.full((n, 1), 6.0), features_dc=fdc)


# the volume the two-layer view is fused into: 2 cm lattice around the front layer's edge, truncation 8 cm
LAYER_VOLUME = dict(origin=(-0.2, -0.1, 0.8), voxel_size=0.02, dims=(21, 11, 71))


def scene(name):
    from monogs_amd import synthetic as S
    if name == "syn2000":
        return S.make_scene(2000, 160, 120, seed=3)
    if name == "syn600":
        return S.make_scene(600, 70, 45, seed=4)
    if name == "deep":
        return deep_scene()
    if name == "single_tile":
        return S.make_scene(300, 16, 16, seed=8)
    if name == "two_layer":
        return two_layer_scene()
    raise KeyError(name)


def model(sc, dev="cpu"):
    from monogs_amd.slam_loops import GaussianParams
    return GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev), sc.opacity_logit.to(dev),
                          sc.features_dc.to(dev))


def camera(sc, dev="cpu"):
    from monogs_amd import viewer as V
    c = sc.cam
    return V.make_view_camera(torch.eye(4), c.H, c.W, c.fx, c.fy, c.cx, c.cy, dev)


@functools.lru_cache(maxsize=None)
def median_oracle(name):
    """{"depth" [H,W] f64 (0 = never crosses), "index" [H,W] (-1), "excluded" [H,W] bool, "position" [H,W]: the median's
    place in its tile's rectangle list (-1)}, computed once per scene and left unchanged."""
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    sc = scene(name)
    H, W = sc.cam.H, sc.cam.W
    m, s, r, o, sh = (t.double() for t in S.activated(sc))
    proj = O.project(m, None, sh, None, o, s, r, None, oracle_settings(sc.cam, sc.bg, dtype=torch.float64), None)
    vis = torch.nonzero(proj.radii > 0).reshape(-1)
    ids = vis[torch.sort(proj.depth[vis], stable=True).indices]              # stable: ties keep ascending index
    xy, con, op, dep = proj.xy[ids], proj.conic[ids], proj.opacity[ids], proj.depth[ids]
    rmin, rmax = proj.rect_min[ids], proj.rect_max[ids]
    res = {"depth": torch.zeros(H, W, dtype=torch.float64), "index": torch.full((H, W), -1, dtype=torch.int64),
           "excluded": torch.zeros(H, W, dtype=torch.bool), "position": torch.full((H, W), -1, dtype=torch.int64)}
    xs = torch.arange(W, dtype=torch.float64)
    tx = (torch.arange(W) // 16)[None]
    cols = torch.arange(W)
    none = torch.full((W,), -1, dtype=torch.int64)

    def walk(alpha, counts_from, cross_at):
        counts = ok & (alpha >= counts_from)
        T = torch.cumprod(1.0 - torch.where(counts, alpha, torch.zeros_like(alpha)), dim=0)
        cross = counts & (T <= cross_at)
        first = torch.argmax(cross.to(torch.int8), dim=0)
        found = cross.any(dim=0)
        return torch.where(found, ids[first], none), first, found

    for y in range(H):
        dx, dy = xy[:, 0:1] - xs[None], xy[:, 1:2] - float(y)
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        inside = (rmin[:, 0:1] <= tx) & (tx < rmax[:, 0:1]) & (rmin[:, 1:2] <= y // 16) & (y // 16 < rmax[:, 1:2])
        ok = inside & (power <= 0)
        a = (op[:, None] * torch.exp(power)).clamp_max(0.99)
        g0, first, found = walk(a, 1.0 / 255.0, 0.5)
        g_hi = walk(a * (1.0 + REL), 1.0 / 255.0 - BAND, 0.5 + BAND)[0]
        g_lo = walk(a * (1.0 - REL), 1.0 / 255.0 + BAND, 0.5 - BAND)[0]
        res["index"][y] = g0
        res["depth"][y] = torch.where(found, dep[first], torch.zeros(W, dtype=torch.float64))
        res["excluded"][y] = (g_hi != g0) | (g_lo != g0)
        res["position"][y] = torch.where(found, (torch.cumsum(inside, dim=0) - 1)[first, cols], none)
    return res


def judge(name, got_depth, got_index, what=""):
    """The comparison both test files make: excluded share <= 2 %; elsewhere the index is equal and the depth agrees
    within 1e-5 (1 + d).  Returns (share, wrong) for the caller's report."""
    ref = median_oracle(name)
    keep = ~ref["excluded"]
    share = ref["excluded"].float().mean().item()
    gd, gi = got_depth.reshape(keep.shape).cpu().double(), got_index.reshape(keep.shape).cpu().long()
    wrong = keep & ((gi != ref["index"]) | ((gd - ref["depth"]).abs() > 1e-5 * (1.0 + ref["depth"])))
    outside = (gi != ref["index"]) & keep
    print(f"{what}{name}: excluded {100 * share:.2f} %, crossing pixels {int((ref['index'] >= 0).sum())} of {keep.numel()}, "
          f"positions up to {int(ref['position'].max())}, index differs outside the exclusion at {int(outside.sum())}")
    assert share <= CAP, share
    assert not wrong.any(), (int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())
    return share, int(wrong.sum())
