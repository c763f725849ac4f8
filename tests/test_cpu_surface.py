"""The surface planes off the GPU (monogs_amd/surface.py and the C ABI's argument checks).

The median mirror is held against the fp64 brute force of surface_cases.median_oracle (its docstring states the
exclusion rule): excluded share <= 2 %, the viewer test's cap - 1.15 % (2000 Gaussians, 160x120) and 0.89 % (600,
70x45) - and everywhere else the same Gaussian and a depth within 1e-5 (1 + d).  The crossings lie at list positions up
to 98 and 124, behind the first 64-splat chunk of the device's walk.

The two-layer scene is the reason the median exists: along the front layer's edge depth / opacity lies between the
layers (135 pixels more than 0.1 from both, in the fp64 oracle and in the fp32 mirror alike: three columns of 45), and
a mesh fused from it has vertices in empty space; the median is exactly one layer's depth at every pixel and the mesh
fused from it has none there.

depth_normal_torch is the contract of mgs_depth_normal; here it is checked against analytic planes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import surface_cases as K
from conftest import oracle_settings

BLEED_PIXELS = 135


def _mirror(name):
    from monogs_amd import surface as SF, viewer as V
    sc = K.scene(name)
    proj = V.project_torch(K.model(sc), K.camera(sc))
    return sc, proj, SF.median_depth_torch(proj, sc.cam.H, sc.cam.W)


@pytest.mark.parametrize("name,deepest", [("syn2000", 98), ("syn600", 124)])
def test_median_mirror_against_fp64_brute_force(name, deepest):
    sc, _, (depth, index) = _mirror(name)
    assert depth.shape == (1, sc.cam.H, sc.cam.W) and index.shape == (sc.cam.H, sc.cam.W) and index.dtype == torch.int64
    K.judge(name, depth, index, "mirror ")
    ref = K.median_oracle(name)
    assert int(ref["position"].max()) == deepest            # crossings behind the first 64-splat chunk
    never = index < 0
    assert bool((depth[0][never] == 0).all()) and bool((depth[0][~never] > 0).all())


def test_two_layers_median_is_a_layer_and_the_mean_bleeds():
    from monogs_amd import surface as SF, synthetic as S, tsdf as T, viewer as V
    from oracle import torch_raster as O
    sc, proj, (median, index) = _mirror("two_layer")
    H, W, zf, zb = sc.cam.H, sc.cam.W, K.Z_FRONT, K.Z_BACK
    cam = K.camera(sc)
    color, depth, opacity = V.blend_torch(proj, H, W, sc.bg)
    opaque = opacity[0] >= 0.95
    assert int(opaque.sum()) > H * W // 2
    m = median[0][opaque].double()
    rel = torch.minimum((m - zf).abs() / zf, (m - zb).abs() / zb)
    assert float(rel.max()) <= 1e-6, float(rel.max())
    assert int((m < 0.5 * (zf + zb)).sum()) > 100 and int((m > 0.5 * (zf + zb)).sum()) > 100      # both layers show

    def bleed(d, o):
        mean = d / o
        return (o >= 0.95) & (mean > zf + 0.1) & (mean < zb - 0.1)

    m_, s_, r_, o_, sh_ = (t.double() for t in S.activated(sc))
    _, _, od, oo, _, _ = O.rasterize(m_, None, sh_, None, o_, s_, r_, None,
                                     oracle_settings(sc.cam, sc.bg, dtype=torch.float64), None, None)
    n_oracle, n_mirror = int(bleed(od[0], oo[0]).sum()), int(bleed(depth[0], opacity[0]).sum())
    print(f"depth / opacity more than 0.1 from both layers: {n_oracle} pixels in the oracle, {n_mirror} in the mirror")
    assert n_oracle >= BLEED_PIXELS and n_mirror >= BLEED_PIXELS
    # fuse the one view and extract
    vol = K.LAYER_VOLUME
    nx, ny, nz = vol["dims"]
    trunc = 4.0 * vol["voxel_size"]
    mid = {}
    for mode, plane in (("mean", depth), ("median", median)):
        planes = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
        T.integrate_torch(*planes, vol["origin"], vol["voxel_size"], trunc, plane, cam.T, cam.fx, cam.fy, cam.cx, cam.cy,
                          image=color, opacity=opacity, min_opacity=0.95, normalize=mode == "mean")
        verts, faces, _ = T.extract_mesh_numpy(*(p.numpy() for p in planes), vol["origin"], vol["voxel_size"], 1.0)
        assert verts.shape[0] > 100 and faces.shape[0] > 100
        z = verts[:, 2]
        mid[mode] = int(((z > zf + trunc) & (z < zb - trunc)).sum())
    print(f"vertices between the layers: mean {mid['mean']}, median {mid['median']}")
    assert mid["mean"] > 0
    assert mid["median"] == 0


# ---- normals ---------------------------------------------------------------------------------------------------------
FX, FY, CX, CY = 60.0, 57.0, 34.5, 22.25


def test_normal_of_a_fronto_parallel_plane_is_exact():
    from monogs_amd.surface import depth_normal_torch
    H, W = 45, 70
    for pc in (0.5, 0.0):
        n = depth_normal_torch(torch.full((H, W), 1.7), FX, FY, CX, CY, pixel_center=pc)
        assert n.shape == (3, H, W) and n.dtype == torch.float32
        inner = n[:, 1:-1, 1:-1]
        assert bool((inner[0] == 0).all()) and bool((inner[1] == 0).all()) and bool((inner[2] == -1).all())
        border = torch.ones(H, W, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        assert bool((n[:, border] == 0).all())
    assert depth_normal_torch(torch.ones(1, H, W), FX, FY, CX, CY).shape == (3, H, W)
    assert bool((depth_normal_torch(torch.ones(2, 5), FX, FY, CX, CY) == 0).all())          # nothing but border


@pytest.mark.parametrize("pc", [0.5, 0.0])
def test_normal_of_a_tilted_plane(pc):
    from monogs_amd.surface import depth_normal_torch
    H, W = 45, 70
    nrm = torch.tensor([0.3, -0.2, -0.93], dtype=torch.float64)
    nrm = nrm / nrm.norm()
    # plane n . P = n_z * 2: depth along the ray ((x + pc - cx) / fx, (y + pc - cy) / fy, 1)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    rx, ry = (x + pc - CX) / FX, (y + pc - CY) / FY
    d = (nrm[2] * 2.0) / (nrm[0] * rx + nrm[1] * ry + nrm[2])
    assert float(d.min()) > 1.0
    n = depth_normal_torch(d.float(), FX, FY, CX, CY, pixel_center=pc, max_jump=0.05)
    inner = n[:, 1:-1, 1:-1].double()
    err = (inner - nrm[:, None, None]).abs().max().item()
    print(f"tilted plane, pixel centre {pc}: max component error {err:.2e}")
    assert err <= 1e-5, err
    # with the wrong pixel centre the plane is a (slightly) different one: the argument is live
    other = depth_normal_torch(d.float(), FX, FY, CX, CY, pixel_center=0.5 - pc)[:, 1:-1, 1:-1].double()
    assert (other - nrm[:, None, None]).abs().max().item() > 1e-4


def test_normal_is_zero_at_steps_and_invalid_taps():
    from monogs_amd.surface import depth_normal_torch
    H, W = 12, 13
    base = torch.full((H, W), 2.0)
    taps = ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0))
    # (the steps: 0.12 > 0.05 * 2.12 seen from the middle and > 0.05 * 2 from a neighbour; 0.102 > 0.05 * 1.898)
    for bad in (0.0, float("nan"), float("inf"), -1.0, 2.0 * 1.06, 2.0 * 0.949):
        d = base.clone()
        d[6, 6] = bad
        n = depth_normal_torch(d, FX, FY, CX, CY, max_jump=0.05)
        assert bool(torch.isfinite(n).all())
        lost = (n == 0).all(dim=0)
        want = torch.zeros(H, W, dtype=torch.bool)
        want[0], want[-1], want[:, 0], want[:, -1] = True, True, True, True
        for dy, dx in taps:                     # the pixel itself and the four whose stencil holds it
            want[6 + dy, 6 + dx] = True
        assert torch.equal(lost, want), bad
    d = base.clone()
    d[6, 6] = 2.0 * 1.049                       # a step inside max_jump keeps the normal
    n = depth_normal_torch(d, FX, FY, CX, CY, max_jump=0.05)
    assert not bool((n[:, 6, 5] == 0).all()) and abs(float(n[:, 6, 5].norm()) - 1.0) < 1e-6


# ---- modes and ABI ---------------------------------------------------------------------------------------------------
def test_surface_modes_compose_like_depth_and_rgb():
    from monogs_amd import surface as SF, viewer as V
    assert V.SURFACE_MODES == ("median_depth", "normal")
    assert V.MODES == ("rgb", "depth", "opacity", "time", "flat_ball", "gaussian_ball")
    sc, proj, (median, _) = _mirror("syn600")
    cam = K.camera(sc)
    f = V.view_frame_torch("median_depth", median_depth=median)
    assert f.dtype == torch.uint8 and f.shape == (sc.cam.H, sc.cam.W, 3)
    assert torch.equal(f, V.compose_torch(median, "depth"))
    n = SF.depth_normal_torch(median, cam.fx, cam.fy, cam.cx, cam.cy)
    g = V.view_frame_torch("normal", normal=n)
    assert torch.equal(g, V.compose_torch(0.5 * n + 0.5, "rgb"))
    assert torch.equal(g, V.view_frame_torch("normal", median_depth=median, camera=cam))
    assert torch.equal(g, V.view_frame_torch("normal", gaussians=K.model(sc), camera=cam))           # the CPU route
    none = (n == 0).all(dim=0)
    assert bool(none.any()) and bool((g[none] == 127).all())                                        # mid-grey
    with pytest.raises(ValueError):
        V.view_frame_torch("wireframe", color=torch.zeros(3, 4, 4))


def test_exports_and_struct_sizes(built):
    from monogs_amd import _cabi
    for n in ("mgs_surface_args_size", "mgs_surface_forward", "mgs_depth_normal_args_size", "mgs_depth_normal"):
        assert n in _cabi.EXPORTS, n
    L = _cabi.lib()
    assert L.mgs_surface_args_size() == C.sizeof(_cabi.SurfaceArgs) == C.sizeof(_cabi.ForwardArgs) + 16
    assert L.mgs_depth_normal_args_size() == C.sizeof(_cabi.DepthNormalArgs) == 48


def test_entry_points_reject_bad_arguments(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_surface_forward(None, None) == -1 and L.mgs_depth_normal(None, None) == -1
    a = _cabi.DepthNormalArgs()
    a.width, a.height, a.fx, a.fy, a.max_jump = 64, 48, 60.0, 60.0, 0.05
    assert L.mgs_depth_normal(C.byref(a), None) == -1                       # null planes
    a.depth = a.normal = 4096
    for w, h in ((0, 48), (64, -1)):
        a.width, a.height = w, h
        assert L.mgs_depth_normal(C.byref(a), None) == -1
    a.width, a.height, a.fx = 64, 48, 0.0
    assert L.mgs_depth_normal(C.byref(a), None) == -1
    s = _cabi.SurfaceArgs()
    s.median_depth = 4096
    assert L.mgs_surface_forward(C.byref(s), None) == -1                    # no bins, no shape
    s.fwd.shape = _cabi.RasterShape(100, 64, 48, 0, 1, 4096, 1.0, 1.0, 1.0)
    for n in ("means3D", "scales", "rotations", "opacities", "shs", "viewmatrix", "projmatrix", "projmatrix_raw", "campos",
              "bg", "geom", "out_color", "out_depth", "out_opacity", "radii", "n_touched"):
        setattr(s.fwd, n, 4096)
    assert L.mgs_surface_forward(C.byref(s), None) == -1                    # everything but the bins workspace
    s.fwd.bins, s.median_depth = 4096, None
    assert L.mgs_surface_forward(C.byref(s), None) == -1                    # no median plane
