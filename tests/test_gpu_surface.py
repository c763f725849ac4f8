"""The surface planes on the device (csrc/surface.hip through the C ABI, viewer.NativeViewer.surface, the viewer's two
surface modes and tsdf's depth_mode="median").

The median plane is held against the fp64 brute force of surface_cases.median_oracle under its exclusion rule (at most
2 % of the pixels left out; everywhere else the same Gaussian and a depth within 1e-5 (1 + d)); mgs_depth_normal, the
two composed modes and the fused planes are compared BIT FOR BIT with their torch mirrors evaluated on the CPU on the
device's own planes.

Sizes: 70x45 is five by three tiles with partial tiles and a width that is no multiple of 4; 160x120 is 80 tiles; 16x16
is a single tile.  The `deep` scene's tile (1, 1) holds a list longer than the walk's 64-splat staging chunk with
crossings behind it, and pixels that never cross."""
import math

import numpy as np
import pytest
import torch

import surface_cases as K

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4, 12345.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _surface_on_device(name, **kw):
    from monogs_amd import viewer as V
    dev = _dev()
    sc = K.scene(name)
    vw = V.NativeViewer(K.model(sc, dev), sc.bg, sc.cam.H, sc.cam.W, dev)
    cam = K.camera(sc, dev)
    out = vw.surface(cam, **kw)
    torch.cuda.synchronize()
    assert vw.check_capacity()
    return sc, vw, cam, out


@pytest.mark.parametrize("name", ["syn2000", "syn600", "deep", "single_tile"])
def test_surface_against_fp64_brute_force(built, name):
    sc, vw, cam, out = _surface_on_device(name)
    H, W = sc.cam.H, sc.cam.W
    assert set(out) == {"color", "depth", "opacity", "median_depth", "median_index", "normal"}
    assert out["median_depth"].shape == (1, H, W) and out["median_index"].shape == (H, W)
    assert out["median_index"].dtype == torch.int32 and out["normal"].shape == (3, H, W)
    K.judge(name, out["median_depth"], out["median_index"], "device ")
    md, mi = out["median_depth"][0].cpu(), out["median_index"].cpu()
    assert bool((md[mi < 0] == 0).all()) and bool((md[mi >= 0] > 0).all())
    # the walk does not disturb the forward: the same planes as a plain frame
    planes = [bits(out[k]) for k in ("color", "depth", "opacity")]
    vw.frame(cam, "rgb")
    torch.cuda.synchronize()
    for got, want, k in zip(planes, (vw.color, vw.depth, vw.opacity), ("color", "depth", "opacity")):
        assert torch.equal(got, bits(want)), k


def test_median_behind_the_first_staging_chunk(built):
    from monogs_amd import _cabi
    name = "deep"
    sc, vw, cam, out = _surface_on_device(name, normals=False)
    assert set(out) == {"color", "depth", "opacity", "median_depth", "median_index"}
    ref = K.median_oracle(name)
    # the scene has the properties it was built for, on the device's own tile lists:
    sizes = _cabi.workspace_sizes(_cabi.RasterShape(vw._N, vw.W, vw.H, 0, vw.K, vw.capacity, 1.0, 1.0, 1.0))
    gx = (vw.W + 15) // 16
    T = gx * ((vw.H + 15) // 16)
    off = vw.geom[sizes.off_tile_offset:sizes.off_tile_offset + 4 * (T + 1)].view(torch.int32).cpu()
    tile = 1 * gx + 1
    n_list = int(off[tile + 1] - off[tile])
    keys = vw.bins[sizes.off_keys:sizes.off_keys + 8 * int(off[T])].view(torch.int64).cpu()
    lo = keys[int(off[tile]):int(off[tile + 1])] & 0xffffffff
    order = (lo >> 12 if vw._N <= (1 << 20) and T <= (1 << 12) else lo).tolist()      # packed keys: id << 12 | pair index
    where = {g: i for i, g in enumerate(order)}
    got_i = out["median_index"].cpu()
    keep = ~ref["excluded"]
    pos = torch.tensor([[where.get(int(got_i[y, x]), -1) for x in range(16, 32)] for y in range(16, 32)])
    crossed = got_i[16:32, 16:32] >= 0
    never = (got_i < 0) & (out["median_depth"][0].cpu() == 0) & keep & (ref["index"] < 0)
    print(f"tile (1,1): list of {n_list}; median positions up to {int(pos.max())}; "
          f"{int((pos >= 64).sum())} pixels cross behind the first chunk; {int(never.sum())} pixels never cross, "
          f"{int(never[16:32, 16:32].sum())} of them in the tile")
    assert n_list > 64
    assert bool((pos[crossed] >= 0).all())                 # every median of the tile is in the tile's list
    assert int((pos >= 64).sum()) >= 8
    assert int(never.sum()) >= 8 and int(never[16:32, 16:32].sum()) >= 1
    K.judge(name, out["median_depth"], out["median_index"], "device ")


# ---- normals ---------------------------------------------------------------------------------------------------------
def _normal_in_guards(vw, depth, args):
    HW = vw.H * vw.W
    buf = torch.full((GUARD + 3 * HW + GUARD,), SENTINEL, device=vw.dev)
    got = vw.depth_normal(depth, *args, out=buf[GUARD:GUARD + 3 * HW].view(3, vw.H, vw.W))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + 3 * HW:] == SENTINEL).all())
    return got


@pytest.mark.parametrize("name", ["syn600", "syn2000"])
def test_normals_of_the_median_plane_bit_for_bit(built, name):
    from monogs_amd.surface import depth_normal_torch
    sc, vw, cam, out = _surface_on_device(name, max_jump=0.08)
    want = depth_normal_torch(out["median_depth"].cpu(), cam.fx, cam.fy, cam.cx, cam.cy, 0.5, 0.08)
    assert torch.equal(bits(out["normal"]), bits(want)), int((bits(out["normal"]) != bits(want)).sum())
    has = (want != 0).any(dim=0)
    lens = want[:, has].norm(dim=0)
    print(f"{name}: {int(has.sum())} of {has.numel()} pixels have a normal")
    assert int(has.sum()) > has.numel() // 20 and int((~has).sum()) > has.numel() // 20
    assert float((lens - 1.0).abs().max()) < 1e-6
    again = _normal_in_guards(vw, out["median_depth"], (cam.fx, cam.fy, cam.cx, cam.cy, 0.5, 0.08))
    assert torch.equal(bits(again), bits(want))


@pytest.mark.parametrize("W,H", [(70, 45), (160, 120)])
def test_normals_of_a_sensor_plane_bit_for_bit(built, W, H):
    from monogs_amd import viewer as V
    from monogs_amd.surface import depth_normal_torch
    dev = _dev()
    g = torch.Generator().manual_seed(7 * W + H)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 1.5 + 0.2 * torch.sin(u / 9.0) * torch.cos(v / 7.0) + 0.002 * torch.rand(H, W, generator=g)
    depth[:, W // 2:] += 0.4                                 # a step past max_jump
    r = torch.rand(H, W, generator=g)
    depth[r < 0.05] = 0.0
    depth[(r >= 0.05) & (r < 0.07)] = float("nan")
    depth[(r >= 0.07) & (r < 0.09)] = float("inf")
    depth[(r >= 0.09) & (r < 0.10)] = -1.0
    vw = V.NativeViewer(None, torch.zeros(3), H, W, dev)
    args = (0.9 * W, 0.88 * W, 0.5 * W - 0.3, 0.5 * H + 0.2, 0.0, 0.05)
    got = _normal_in_guards(vw, depth.to(dev).contiguous(), args)
    want = depth_normal_torch(depth, *args)
    assert torch.equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    has = (want != 0).any(dim=0)
    assert int(has.sum()) > H * W // 4 and int((~has).sum()) > H * W // 10
    assert not bool(has[:, W // 2 - 1:W // 2 + 1][1:-1].any())                   # the step's two columns
    assert bool(torch.isfinite(got).all())


# ---- the viewer's modes ----------------------------------------------------------------------------------------------
def test_surface_modes_equal_the_mirror(built):
    from monogs_amd import viewer as V
    dev = _dev()
    sc = K.scene("syn600")
    vw = V.NativeViewer(K.model(sc, dev), sc.bg, sc.cam.H, sc.cam.W, dev)
    cam = K.camera(sc, dev)
    assert V.MODES == ("rgb", "depth", "opacity", "time", "flat_ball", "gaussian_ball")
    assert V.SURFACE_MODES == ("median_depth", "normal")
    with pytest.raises(ValueError):
        vw.frame(cam, "wireframe")
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.1, 0.05, 0.6])                           # a camera in view
    over = dict(current=pose, frustum_size=0.2)
    got = vw.frame(cam, "median_depth", **over)
    torch.cuda.synchronize()
    want = V.view_frame_torch("median_depth", median_depth=vw.median_depth.cpu(), endpoints=vw.endpoints.cpu(), **over)
    assert got.dtype == torch.uint8 and got.shape == (sc.cam.H, sc.cam.W, 3)
    assert torch.equal(got.cpu(), want)
    plain = V.view_frame_torch("median_depth", median_depth=vw.median_depth.cpu())
    assert int((plain != want).any(dim=2).sum()) > 0                       # the overlay drew something
    got = vw.frame(cam, "normal")
    torch.cuda.synchronize()
    want = V.view_frame_torch("normal", normal=vw.normal.cpu())
    assert torch.equal(got.cpu(), want)
    none = (vw.normal.cpu() == 0).all(dim=0)
    assert bool(none.any()) and bool((got.cpu()[none] == 127).all()) and bool((got.cpu()[~none] != 127).any())
    # the normals are those of the median plane this call made
    assert torch.equal(want, V.view_frame_torch("normal", median_depth=vw.median_depth.cpu(), camera=cam))
    assert vw.check_capacity()


# ---- fusion ----------------------------------------------------------------------------------------------------------
def _view_camera(sc, dev):
    from monogs_amd.slam_loops import ViewCamera
    c = sc.cam
    return ViewCamera(0, torch.zeros(3, c.H, c.W), torch.eye(4), c.projmatrix_raw, 2 * math.atan(c.tanfovx),
                      2 * math.atan(c.tanfovy), c.H, c.W, dev, intrinsics=(c.fx, c.fy, c.cx, c.cy))


def test_integrate_view_median_equals_the_mirror_and_mean_is_untouched(built):
    from monogs_amd.tsdf import TSDFVolume, integrate_torch
    dev = _dev()
    sc = K.scene("two_layer")
    gm, cam, bg = K.model(sc, dev), _view_camera(sc, dev), sc.bg.to(dev)
    dims, vs = (72, 19, 10), 0.02
    origin = (-0.71, -0.18, K.Z_FRONT - 0.09)               # around the front layer and its edge
    vol = TSDFVolume(origin, vs, dims, device=dev)
    planes = vol.integrate_view(gm, cam, bg, depth_mode="median", weight=1.5)
    torch.cuda.synchronize()
    nx, ny, nz = dims
    ref = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    integrate_torch(*ref, origin, vs, vol.trunc, planes["median_depth"].cpu(), cam.T.cpu(), cam.fx, cam.fy, cam.cx, cam.cy,
                    image=planes["color"].cpu(), opacity=planes["opacity"].cpu(), min_opacity=0.95, normalize=False,
                    view_weight=1.5, max_weight=vol.max_weight)
    for got, want, name in zip((vol.tsdf, vol.weight, vol.color), ref, ("tsdf", "weight", "color")):
        assert torch.equal(bits(got), bits(want)), name
    assert float(vol.weight.max()) == 1.5 and float(vol.tsdf.min()) < 0.0 and float(vol.color.max()) > 0.0
    # a second view accumulates once (the capacity is confirmed before the integration, not after)
    vol.integrate_view(gm, cam, bg, depth_mode="median", weight=1.5)
    assert float(vol.weight.max()) == 3.0
    # the default is the mean mode, bit for bit
    a, b = TSDFVolume(origin, vs, dims, device=dev), TSDFVolume(origin, vs, dims, device=dev)
    a.integrate_view(gm, cam, bg)
    b.integrate_view(gm, cam, bg, depth_mode="mean")
    torch.cuda.synchronize()
    for x, y in zip((a.tsdf, a.weight, a.color), (b.tsdf, b.weight, b.color)):
        assert torch.equal(bits(x), bits(y))
    assert float(a.weight.max()) == 1.0
    with pytest.raises(ValueError):
        a.integrate_view(gm, cam, bg, depth_mode="mode")


def test_integrate_view_median_renders_again_after_a_capacity_overflow(built):
    from monogs_amd.tsdf import TSDFVolume
    dev = _dev()
    sc = K.scene("two_layer")
    gm, cam, bg = K.model(sc, dev), _view_camera(sc, dev), sc.bg.to(dev)
    dims, vs, origin = (72, 19, 10), 0.02, (-0.71, -0.18, K.Z_FRONT - 0.09)
    vols = {}
    for name, cap in (("small", 1024), ("large", None)):
        vol = vols[name] = TSDFVolume(origin, vs, dims, device=dev)
        vw = vol._surface_viewer(gm, bg, sc.cam.H, sc.cam.W)
        if cap is not None:
            vw.capacity = cap                                  # far below the view's pairs: the first render is truncated
        vol.integrate_view(gm, cam, bg, depth_mode="median")
        assert vol._surface_viewer(gm, bg, sc.cam.H, sc.cam.W) is vw             # kept per (H, W, map)
    torch.cuda.synchronize()
    assert vols["small"]._viewer.capacity > 1024 and float(vols["small"].weight.max()) == 1.0      # integrated once
    for a, b in zip((vols["small"].tsdf, vols["small"].weight, vols["small"].color),
                    (vols["large"].tsdf, vols["large"].weight, vols["large"].color)):
        assert torch.equal(bits(a), bits(b))


def test_two_layer_mesh_on_the_device(built):
    from monogs_amd import tsdf as T
    dev = _dev()
    sc = K.scene("two_layer")
    gm, cam, bg = K.model(sc, dev), _view_camera(sc, dev), sc.bg.to(dev)
    vs = K.LAYER_VOLUME["voxel_size"]
    mid = {}
    for mode in ("mean", "median"):
        vol = T.TSDFVolume(K.LAYER_VOLUME["origin"], vs, K.LAYER_VOLUME["dims"], device=dev)
        assert T.fuse_map(gm, [cam], bg, vs, volume=vol, depth_mode=mode) is vol
        verts, faces, _ = vol.extract_mesh()
        assert verts.shape[0] > 100 and faces.shape[0] > 100
        z = verts[:, 2].cpu()
        mid[mode] = int(((z > K.Z_FRONT + vol.trunc) & (z < K.Z_BACK - vol.trunc)).sum())
    print(f"vertices between the layers: mean {mid['mean']}, median {mid['median']}")
    assert mid["mean"] > 0
    assert mid["median"] == 0
