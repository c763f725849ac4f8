"""The headless viewer on the device (csrc/viewer.hip through the C ABI and monogs_amd.viewer.NativeViewer).

Compose, the time tint and the overlay's draw step are compared BIT FOR BIT with the torch mirror, evaluated on the CPU
on the same float planes / the device's own end points.  The ellipsoid shader is compared with a brute-force fp64 search
over all visible Gaussians of oracle.torch_raster.project (stable depth order, ties by index): a pixel is left out when
any visible splat's alpha lies within 2e-4 of the threshold there (the kernel's fp32 exponent and exp differ from the
fp64 ones by ~1e-5 relative) - at most 2 % of the pixels - and everywhere else the hit Gaussian (through
its depth) is the same and the colour agrees to 1e-4, the project's forward tolerance.  The overlay's fixed-point end
points are within one unit (1/16 px) of an fp64 projection written out here.

Sizes: 70x45 is five by three tiles with partial tiles, a width that is no multiple of 4 and H W 3 = 9450 bytes, no
multiple of 4 (the compose kernel's byte path); 160x120 = 19200 pixels is past one trip (16384) of the maximum's
reduction; 20000 Gaussians are past one trip of the id-range reduction; the crowded tile's list is longer than the
first-hit kernel's 64-splat staging chunk; the overlay's lines are longer than the 64 steps a wave draws per trip."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from conftest import oracle_settings

pytestmark = pytest.mark.gpu

BAND, CAP, COLOR_TOL = 2e-4, 0.02, 1e-4
THR = {"flat_ball": 0.22, "gaussian_ball": 0.4}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _model(sc, dev, kf_groups=7):
    from monogs_amd.slam_loops import GaussianParams
    gm = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev), sc.opacity_logit.to(dev),
                        sc.features_dc.to(dev))
    n = sc.means3D.shape[0]
    gm.unique_kfIDs = (torch.arange(n, dtype=torch.int32, device=dev) * kf_groups // n) * 3 + 2
    return gm


def _camera(sc, dev, T=None):
    from monogs_amd import viewer as V
    c = sc.cam
    return V.make_view_camera(torch.eye(4) if T is None else T, c.H, c.W, c.fx, c.fy, c.cx, c.cy, dev)


# ---- (a) compose -----------------------------------------------------------------------------------------------------
def _planes(H, W, mode, kind, dev):
    g = torch.Generator().manual_seed(100 * H + W + len(mode) + 7 * len(kind))
    if mode == "rgb":
        x = -0.3 + 1.6 * torch.rand(3, H, W, generator=g)                 # the clamp is live at both ends
        x[:, 0, :5] = torch.tensor([0.0, 1.0, 1.0 / 255, 254.999 / 255, 0.5])
    elif mode == "depth":
        x = 6.0 * torch.rand(1, H, W, generator=g)
        x[0, 0, :3] = torch.tensor([0.0, 0.1, 0.05])
    else:
        x = torch.rand(1, H, W, generator=g) ** 2
    if kind == "nan":
        x[torch.rand(x.shape, generator=g) < 0.05] = float("nan")
        x[..., -1, -1] = float("nan")                                      # the very last pixel (the byte path at 70x45)
    elif kind == "constant":
        x = torch.full_like(x, {"rgb": 0.4, "depth": 0.05, "opacity": 0.0}[mode])      # depth, opacity: max <= lo
    return x.to(dev).contiguous()


@pytest.mark.parametrize("kind", ["random", "nan", "constant"])
@pytest.mark.parametrize("mode", ["rgb", "depth", "opacity"])
@pytest.mark.parametrize("W,H", [(70, 45), (160, 120)])
def test_compose_bit_exact(built, W, H, mode, kind):
    from monogs_amd import viewer as V
    dev = _dev()
    vw = V.NativeViewer(None, torch.zeros(3), H, W, dev)
    src = _planes(H, W, mode, kind, dev)
    out = torch.full((H * W * 3 + 8,), 77, dtype=torch.uint8, device=dev)                # guard bytes behind the frame
    got = vw.compose(src, mode, out[:H * W * 3].view(H, W, 3))
    torch.cuda.synchronize()
    want = V.compose_torch(src.cpu(), mode)
    assert got.dtype == torch.uint8 and got.shape == (H, W, 3)
    diff = (got.cpu() != want).any(dim=2)
    assert not diff.any(), (int(diff.sum()), torch.nonzero(diff)[:4].tolist())
    assert (out[H * W * 3:] == 77).all()
    if kind == "nan":
        if mode == "rgb":                                  # channel by channel: the NaN element is 0
            assert (got.permute(2, 0, 1)[torch.isnan(src)] == 0).all()
        else:                                              # a colour-mapped NaN is a black pixel
            assert (got[torch.isnan(src[0])] == 0).all()
    if kind == "constant" and mode != "rgb":
        assert (got.cpu() == torch.from_numpy(V.JET_LUT[0].copy())).all()


# ---- (b) first hit ---------------------------------------------------------------------------------------------------
def hit_cluster_scene(W=70, H=45, seed=11):
    """A sparse scene plus, inside tile (1, 1): 150 near, low-opacity Gaussians (opacity 0.05 .. 0.29: most can never
    reach 0.22, let alone 0.4) in front of 25 small opaque ones - tile list > 64, first hits behind the first staging
    chunk where an opaque splat shows through, and no hit at all where none does."""
    from monogs_amd import synthetic as S
    sc = S.make_scene(40, W, H, seed=seed)
    cam = sc.cam
    g = torch.Generator().manual_seed(seed + 1)

    def cluster(n, z0, z1, sig_px, logit0, logit1):
        u = 17.0 + 13.0 * torch.rand(n, generator=g)
        v = 17.0 + 13.0 * torch.rand(n, generator=g)
        z = z0 + (z1 - z0) * torch.rand(n, generator=g)
        xyz = torch.stack([(u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z], dim=1)
        sig = sig_px * torch.exp(0.2 * torch.randn(n, generator=g))
        ls = torch.log((sig * z / cam.fx)[:, None] * torch.exp(0.2 * torch.randn(n, 3, generator=g)))
        rot = torch.nn.functional.normalize(torch.randn(n, 4, generator=g))
        op = logit0 + (logit1 - logit0) * torch.rand(n, 1, generator=g)
        fdc = ((torch.rand(n, 3, generator=g) - 0.5) / S.SH_C0)[:, None, :]
        return xyz, ls, rot, op, fdc

    parts = [cluster(150, 0.6, 0.9, 3.0, -2.9, -0.9), cluster(25, 3.0, 4.0, 0.9, 3.0, 3.5)]
    cat = lambda i, base: torch.cat([base] + [p[i] for p in parts]).contiguous()
    return sc._replace(means3D=cat(0, sc.means3D), log_scales=cat(1, sc.log_scales), rot=cat(2, sc.rot),
                       opacity_logit=cat(3, sc.opacity_logit), features_dc=cat(4, sc.features_dc))


def _scene(name):
    from monogs_amd import synthetic as S
    if name == "syn2000":
        return S.make_scene(2000, 160, 120, seed=3)
    if name == "syn600":
        return S.make_scene(600, 70, 45, seed=4)
    return hit_cluster_scene()


@functools.lru_cache(maxsize=None)
def brute_force(name):
    """fp64 first hit of both thresholds over ALL visible Gaussians (no tiles), computed once per scene:
    {mode: (depth [H,W] (0 = none), colour [3,H,W], excluded [H,W], hit id [H,W] (-1 = none))} and the projection."""
    from monogs_amd import synthetic as S
    from oracle import torch_raster as O
    sc = _scene(name)
    H, W = sc.cam.H, sc.cam.W
    m, s, r, o, sh = (t.double() for t in S.activated(sc))
    proj = O.project(m, None, sh, None, o, s, r, None, oracle_settings(sc.cam, sc.bg, dtype=torch.float64), None)
    vis = torch.nonzero(proj.radii > 0).reshape(-1)
    ids = vis[torch.sort(proj.depth[vis], stable=True).indices]              # stable: ties keep ascending index
    xy, con, op, rgb, dep = proj.xy[ids], proj.conic[ids], proj.opacity[ids], proj.rgb[ids], proj.depth[ids]
    res = {k: (torch.zeros(H, W, dtype=torch.float64), sc.bg.double().reshape(3, 1, 1).repeat(1, H, W),
               torch.zeros(H, W, dtype=torch.bool), torch.full((H, W), -1, dtype=torch.int64)) for k in THR}
    xs = torch.arange(W, dtype=torch.float64)
    for y in range(H):
        dx, dy = xy[:, 0:1] - xs[None], xy[:, 1:2] - float(y)
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        a = (op[:, None] * torch.exp(power)).clamp_max(0.99)
        ok = (power <= 0) & (a >= 1.0 / 255.0)
        cols = torch.arange(W)
        for k, thr in THR.items():
            hit = ok & (a > thr)
            first = torch.argmax(hit.to(torch.int8), dim=0)
            found = hit.any(dim=0)
            c = rgb[first].t() * (torch.exp(power[first, cols])[None] if k == "gaussian_ball" else 1.0)
            res[k][0][y] = torch.where(found, dep[first], torch.zeros(W, dtype=torch.float64))
            res[k][1][:, y] = torch.where(found[None], c, res[k][1][:, y])
            res[k][2][y] = ((a - thr).abs() <= BAND).any(dim=0)
            res[k][3][y] = torch.where(found, ids[first], torch.full((W,), -1, dtype=torch.int64))
    return res, proj, ids


def _first_hit_on_device(name, mode):
    from monogs_amd import viewer as V
    dev = _dev()
    sc = _scene(name)
    vw = V.NativeViewer(_model(sc, dev), sc.bg, sc.cam.H, sc.cam.W, dev)
    frame = vw.frame(_camera(sc, dev), mode)
    torch.cuda.synchronize()
    assert vw.check_capacity()
    return vw, frame


def _judge(name, mode, vw):
    depth, color, excluded, _ = brute_force(name)[0][mode]
    share = excluded.float().mean().item()
    got_d, got_c = vw.hit_depth[0].cpu().double(), vw.hit_color.cpu().double()
    keep = ~excluded
    wrong = keep & ((got_d - depth).abs() > 1e-5 * (1.0 + depth))
    cerr = ((got_c - color).abs().max(dim=0).values * keep).max().item()
    print(f"{name} {mode}: excluded {100 * share:.2f} %, hit pixels {int((depth > 0).sum())} of {depth.numel()}, "
          f"wrong Gaussian at {int(wrong.sum())}, colour err {cerr:.2e}")
    assert share <= CAP, share
    assert not wrong.any(), (int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())
    assert cerr <= COLOR_TOL, cerr


@pytest.mark.parametrize("mode", ["flat_ball", "gaussian_ball"])
@pytest.mark.parametrize("name", ["syn2000", "syn600"])
def test_first_hit_against_brute_force(built, name, mode):
    vw, _ = _first_hit_on_device(name, mode)
    _judge(name, mode, vw)


@pytest.mark.parametrize("mode", ["flat_ball", "gaussian_ball"])
def test_first_hit_behind_the_first_staging_chunk(built, mode):
    from monogs_amd import _cabi
    name = "cluster"
    vw, frame = _first_hit_on_device(name, mode)
    res, proj, ids = brute_force(name)
    depth, _, excluded, hit_id = res[mode]
    # the scene has the properties it was built for, on the device's own tile lists and in the reference:
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
    pos = torch.tensor([[where.get(int(hit_id[y, x]), -1) for x in range(16, 32)] for y in range(16, 32)])
    print(f"tile (1,1): list of {n_list}; hit positions up to {int(pos.max())}; "
          f"{int((pos >= 64).sum())} pixels hit behind the first chunk; {int((depth == 0).sum())} pixels without a hit, "
          f"{int((depth[16:32, 16:32] == 0).sum())} of them in the tile")
    assert n_list > 64
    assert (pos[hit_id[16:32, 16:32] >= 0] >= 0).all()              # every reference hit of the tile is in its list
    assert (pos >= 64).sum() >= 8                                    # first hits past the first chunk
    assert (depth == 0).sum() >= 8 and (depth[16:32, 16:32] == 0).sum() >= 1      # and pixels with no hit at all
    _judge(name, mode, vw)
    bg = torch.zeros(3, dtype=torch.uint8)
    assert (frame.cpu()[(depth == 0) & ~excluded] == bg).all()       # no hit: the background


# ---- (c) time colours ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_time_colors_bit_exact(built, K):
    from monogs_amd import viewer as V
    dev = _dev()
    vw = V.NativeViewer(None, torch.zeros(3), 8, 8, dev)
    g = torch.Generator().manual_seed(K)
    N = 20000                                                      # past one trip (16384) of the id-range reduction
    feats = torch.randn(N, K, 3, generator=g)
    ids = torch.randint(5, 120, (N,), generator=g, dtype=torch.int32)
    ids[N - 1], ids[17000] = 2, 131                                  # the extremes lie in the second trip
    got = vw.time_colors(feats.to(dev).contiguous(), ids.to(dev))
    same = vw.time_colors(feats.to(dev).contiguous(), torch.full((N,), 9, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), V.time_colors_torch(feats, ids))
    assert torch.equal(same.cpu(), V.time_colors_torch(feats, torch.full((N,), 9, dtype=torch.int32)))


# ---- (d) overlay -----------------------------------------------------------------------------------------------------
def _project_fp64(segs, T, fx, fy, cx, cy, W, H, near):
    """World segments [S,2,3] -> (end points [S,4] in pixels, valid [S]) in double: near clip, pinhole, Liang-Barsky
    against [-W/2, 3W/2] x [-H/2, 3H/2]."""
    out, valid = np.zeros((len(segs), 4)), np.zeros(len(segs), bool)
    for s, seg in enumerate(segs):
        v = seg @ T[:3, :3].T + T[:3, 3]
        if v[0, 2] < near and v[1, 2] < near:
            continue
        for q in range(2):
            if v[q, 2] < near:
                t = (near - v[q, 2]) / (v[1 - q, 2] - v[q, 2])
                v[q] = v[q] + t * (v[1 - q] - v[q])
        p = np.stack([fx * v[:, 0] / v[:, 2] + cx, fy * v[:, 1] / v[:, 2] + cy], axis=1)
        d = p[1] - p[0]
        t0, t1, ok = 0.0, 1.0, True
        for pp, qq in ((-d[0], p[0, 0] + 0.5 * W), (d[0], 1.5 * W - p[0, 0]), (-d[1], p[0, 1] + 0.5 * H),
                       (d[1], 1.5 * H - p[0, 1])):
            if pp == 0:
                ok = ok and qq >= 0
            elif pp < 0:
                ok = ok and qq / pp <= t1
                t0 = max(t0, qq / pp)
            else:
                ok = ok and qq / pp >= t0
                t1 = min(t1, qq / pp)
        if ok:
            out[s], valid[s] = np.concatenate([p[0] + t0 * d, p[0] + t1 * d]), True
    return out, valid


def test_overlay_end_points_and_frame(built):
    from monogs_amd import synthetic as S
    from monogs_amd import viewer as V
    from monogs_amd.pose import SE3_exp
    dev = _dev()
    W, H = 160, 120
    sc = S.make_scene(10, W, H, seed=1)
    T_view = SE3_exp(torch.tensor([0.02, -0.01, 0.03, 0.03, -0.02, 0.01]))
    cam = _camera(sc, dev, T_view)

    def pose(x, y, z, rot):
        P = torch.linalg.inv(SE3_exp(torch.tensor([0.0, 0.0, 0.0] + rot)))
        P[:3, 3] = torch.tensor([x, y, z])
        return P

    in_view = pose(-0.2, 0.1, 1.0, [0.2, -0.3, 0.1])
    half_behind = pose(0.3, 0.1, -0.2, [0.0, 0.1, 0.0])              # apex behind the camera, far points in front
    behind = pose(0.1, 0.0, -3.0, [0.1, 0.0, 0.2])
    keyframes = torch.stack([in_view, half_behind, behind])
    current = pose(0.0, -0.1, 0.8, [-0.1, 0.2, 0.0])
    trajectory = torch.tensor([[-3.0, 0.0, 2.0], [-0.5, 0.2, 1.5], [0.0, 0.1, 0.5], [0.2, 0.0, -1.0], [0.3, 0.0, -2.0],
                               [40.0, 0.0, 1.0]])                      # leaves the image, dives behind, far outside
    size = 0.5
    vw = V.NativeViewer(None, torch.zeros(3), H, W, dev)
    g = torch.Generator().manual_seed(3)
    base = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    frame = vw.overlay(base.to(dev).clone(), cam, keyframes, current, trajectory, size)
    torch.cuda.synchronize()
    ep = vw.endpoints.cpu()
    # 1. the fixed-point end points against an fp64 projection
    poses, pcol, free, fcol = V.overlay_segments(keyframes, current, trajectory, size)
    segs = V.world_segments(poses.double(), free.double(), size).numpy()
    assert ep.shape == (8 * 4 + 5, 5)
    want, valid = _project_fp64(segs, T_view.double().numpy(), cam.fx, cam.fy, cam.cx - 0.5, cam.cy - 0.5, W, H, V.NEAR_Z)
    assert ep[:, 4].bool().tolist() == valid.tolist()
    err = (ep[:, :4].double().numpy() - 16.0 * want)[valid]
    print("end points: max error", np.abs(err).max(), "units; valid", int(valid.sum()), "of", len(valid))
    assert np.abs(err).max() <= 1.0
    assert valid[:8].all() and valid[8:16].any() and not valid[16:24].any()          # in view / half behind / behind
    assert (ep[16:24] == 0).all()
    length = np.abs(want[:, 2:] - want[:, :2]).max(axis=1)[valid]
    assert length.max() > 64                                                          # a second trip of the draw loop
    # 2. the frame against the mirror's draw step on the device's own end points
    mirror = V.overlay_draw_torch(base, ep, V.segment_colors(pcol, fcol))
    assert torch.equal(frame.cpu(), mirror)
    drawn = (mirror != base).any(dim=2)
    assert drawn.sum() > 200
    for c in (V.COLOR_KEYFRAME, V.COLOR_CURRENT, V.COLOR_TRAJECTORY):
        assert (mirror == torch.tensor(c, dtype=torch.uint8)).all(dim=2).sum() > 10
    # a second call on the same inputs gives the same bytes (the owner map is reset by every call)
    again = vw.overlay(base.to(dev).clone(), cam, keyframes, current, trajectory, size)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), mirror)


# ---- NativeViewer.frame and run_sequence -----------------------------------------------------------------------------
def test_frame_every_mode_equals_the_mirror(built):
    from monogs_amd import synthetic as S
    from monogs_amd import viewer as V
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe, ViewCamera
    dev = _dev()
    sc = S.make_scene(2000, 160, 120, seed=3)
    H, W = sc.cam.H, sc.cam.W
    gm = _model(sc, dev)
    cam = _camera(sc, dev)
    vw = V.NativeViewer(gm, sc.bg, H, W, dev)
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.1, 0.05, 0.6])
    over = dict(keyframes=pose[None], current=torch.eye(4), trajectory=torch.tensor([[0.0, 0.0, 0.3], [0.1, 0.05, 0.6]]),
                frustum_size=0.2)
    frames = {}
    for mode in V.MODES:
        got = vw.frame(cam, mode, **over)
        torch.cuda.synchronize()
        want = V.view_frame_torch(mode, color=vw.color.cpu(), depth=vw.depth.cpu(), opacity=vw.opacity.cpu(),
                                  hit_color=vw.hit_color.cpu(), endpoints=vw.endpoints.cpu(), **over)
        assert got.dtype == torch.uint8 and got.shape == (H, W, 3) and got.device.type == "cuda"
        assert torch.equal(got.cpu(), want), mode
        frames[mode] = got.cpu()
        if mode == "rgb":          # the planes are the package's own render
            v = ViewCamera(0, torch.zeros(3, H, W), torch.eye(4), sc.cam.projmatrix_raw, 2 * math.atan(sc.cam.tanfovx),
                           2 * math.atan(sc.cam.tanfovy), H, W, dev)
            with torch.no_grad():
                pkg = render(v, gm, Pipe, sc.bg.to(dev))
            assert (pkg["render"] - vw.color).abs().max() < 1e-6 and (pkg["depth"] - vw.depth).abs().max() < 1e-5
    assert vw.check_capacity()
    for a, b in (("rgb", "time"), ("rgb", "flat_ball"), ("flat_ball", "gaussian_ball"), ("depth", "opacity")):
        assert not torch.equal(frames[a], frames[b]), (a, b)
    half = vw.frame(cam, "rgb", scale_modifier=0.5)
    assert not torch.equal(half.cpu(), vw.frame(cam, "rgb").cpu())              # the scaling slider reaches the forward
    # the time tint did not touch the model
    assert torch.equal(gm._features_dc.detach().cpu(), sc.features_dc)
    with pytest.raises(ValueError):
        vw.frame(cam, "wireframe")


def _smoke_sequence(dev):
    """The sequence of tests/test_gpu_slam_smoke.py: six 160x120 frames of a 6000-Gaussian world along one twist."""
    from monogs_amd import slam_surrogate as SS
    from monogs_amd import synthetic as S
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, Pipe, ViewCamera
    W, H = 160, 120
    sc = S.make_scene(6000, W, H, seed=33)
    cam = sc.cam
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    bg = torch.zeros(3, device=dev)
    world = GaussianParams(sc.means3D.to(dev), sc.log_scales.to(dev), sc.rot.to(dev), sc.opacity_logit.to(dev),
                           sc.features_dc.to(dev))
    step = torch.tensor([0.04, -0.02, 0.025, 0.012, -0.009, 0.006])
    frames = []
    with torch.no_grad():
        for k in range(6):
            T = SE3_exp(k * step)
            pkg = render(ViewCamera(k, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, dev), world, Pipe, bg)
            frames.append(SS.Frame(k, pkg["render"].clamp(0, 1).clone(), pkg["depth"][0].clone(), T))
    return frames, cam


def test_run_sequence_takes_frames_and_changes_nothing(built):
    from monogs_amd import slam_surrogate as SS
    dev = _dev()
    frames, cam = _smoke_sequence(dev)
    H, W = cam.H, cam.W
    cfg = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01},
           "Dataset": {"type": "tum", "pcd_downsample": 4, "pcd_downsample_init": 2}}
    kw = dict(sensor_depth=True, init_iters=20, mapping_iters=5, kf_interval=3, first_order_iters=4, second_order_iters=0,
              config=cfg)
    plain = SS.run_sequence(frames, cam, dev, **kw)
    seen = SS.run_sequence(frames, cam, dev, viewer_every=2, viewer_modes=("rgb", "depth", "flat_ball"), **kw)
    torch.cuda.synchronize()
    assert "view_frames" not in plain and sorted(seen["view_frames"]) == [2, 4]
    for k, shots in seen["view_frames"].items():
        assert sorted(shots) == ["depth", "flat_ball", "rgb"]
        for m, f in shots.items():
            assert f.dtype == torch.uint8 and tuple(f.shape) == (H, W, 3) and f.device.type == "cuda", (k, m)
        assert shots["rgb"].float().std() > 1.0                         # the follow-camera sees the map
    assert plain["kf_ids"] == seen["kf_ids"] and sorted(plain["cameras"]) == sorted(seen["cameras"])
    for k in plain["cameras"]:
        assert torch.equal(plain["cameras"][k].T, seen["cameras"][k].T), k
    ga, gb = plain["gaussians"], seen["gaussians"]
    for name in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc"):
        assert torch.equal(getattr(ga, name), getattr(gb, name)), name
    own = SS.run_sequence(frames, cam, dev, viewer_every=4, viewer_follow=False, **kw)["view_frames"]
    assert sorted(own) == [4] and tuple(own[4]["rgb"].shape) == (H, W, 3)
