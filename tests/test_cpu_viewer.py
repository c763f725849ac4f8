"""The headless viewer off the GPU: the colour map and its index rule, the torch mirrors of the time tint and of the
line overlay's integer draw step against pixels written out by hand, the follow-camera and the frustum against the
arithmetic of gui/gui_utils.py:24-66, the CPU route of view_frame_torch, save_frame, and the C ABI's export list."""
import math
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def V():
    from monogs_amd import viewer
    return viewer


# ---- colour map ------------------------------------------------------------------------------------------------------
def test_jet_lut_is_the_committed_table():
    gold = np.load(os.path.join(HERE, "golden", "jet_lut.npz"))["lut"]
    lut = V().JET_LUT
    assert lut.dtype == np.uint8 and lut.shape == (256, 3) and lut.nbytes == 768
    assert lut.tobytes() == gold.tobytes()
    assert lut[0].tolist() == [0, 0, 127] and lut[255].tolist() == [127, 0, 0]      # jet: dark blue ... dark red


def test_index_rule_on_hand_written_cases():
    t = torch.tensor([-0.5, 0.0, 1.0 / 256, 0.5, 255.0 / 256, 1.0 - 2.0 ** -24, 1.0, 7.0, float("nan"), float("inf")])
    assert V().lut_index(t).tolist() == [0, 0, 1, 128, 255, 255, 255, 255, 0, 255]


def test_compose_mirror_on_hand_written_planes():
    v = V()
    lut = torch.from_numpy(v.JET_LUT.copy())
    rgb = torch.tensor([-1.0, 0.0, 0.5, 0.999, 1.0, 3.0, float("nan"), 1.0 / 255]).reshape(1, 1, 8).repeat(3, 1, 1)
    assert v.compose_torch(rgb, "rgb")[0, :, 0].tolist() == [0, 0, 127, 254, 255, 255, 0, 1]      # truncated, NaN black
    d = torch.tensor([[0.1, 2.1, 4.1, float("nan"), 0.0, 1.1]])
    out = v.compose_torch(d[None], "depth")                     # max 4.1: t = (d - 0.1) / 4 up to rounding
    assert out[0, 0].tolist() == lut[0].tolist() and out[0, 2].tolist() == lut[255].tolist()
    assert out[0, 1].tolist() in (lut[127].tolist(), lut[128].tolist())
    assert out[0, 3].tolist() == [0, 0, 0] and out[0, 4].tolist() == lut[0].tolist()
    assert out[0, 5].tolist() == lut[64].tolist()
    o = torch.tensor([[0.0, 0.25, 0.5]])
    assert v.compose_torch(o, "opacity")[0].tolist() == [lut[0].tolist(), lut[128].tolist(), lut[255].tolist()]
    flat = torch.full((1, 2, 3), 0.05)                           # max <= lo: t = 0 everywhere, a NaN is still black
    flat[0, 1, 1] = float("nan")
    out = v.compose_torch(flat, "depth")
    assert out[0, 0].tolist() == lut[0].tolist() and out[1, 1].tolist() == [0, 0, 0]
    assert (v.compose_torch(torch.zeros(1, 2, 2), "opacity") == lut[0]).all()


# ---- overlay: the integer draw step ----------------------------------------------------------------------------------
RED, GREEN = (255, 0, 0), (0, 255, 0)


def _draw(segments, colors, H=8, W=8):
    ep = torch.tensor([[16 * a for a in s] + [1] if len(s) == 4 else s for s in segments], dtype=torch.int32)
    out = V().overlay_draw_torch(torch.zeros(H, W, 3, dtype=torch.uint8), ep, torch.tensor(colors, dtype=torch.uint8))
    lit = {(int(x), int(y)): tuple(out[y, x].tolist()) for y, x in torch.nonzero(out.sum(dim=2) > 0).tolist()}
    return lit


def test_draw_step_against_hand_written_pixels():
    assert _draw([(2, 3, 6, 3)], [RED]) == {(x, 3): RED for x in range(2, 7)}                    # horizontal
    assert _draw([(5, 1, 5, 6)], [RED]) == {(5, y): RED for y in range(1, 7)}                    # vertical
    assert _draw([(0, 0, 4, 4)], [RED]) == {(k, k): RED for k in range(5)}                       # 45 degrees
    assert _draw([(4, 4, 0, 0)], [RED]) == {(k, k): RED for k in range(5)}                       # ... backwards
    # shallow: six steps in x, two in y; y_k = floor((64 k + 6) / 12) sixteenths, rounded to the pixel
    shallow = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (6, 2)]
    assert _draw([(0, 0, 6, 2)], [RED]) == {p: RED for p in shallow}
    assert _draw([(-3, 1, 2, 1)], [RED]) == {(x, 1): RED for x in range(3)}                      # leaves the image
    assert _draw([(6, 6, 11, 9)], [RED]) == {(6, 6): RED, (7, 7): RED}                            # ... on the far side
    assert _draw([(3, 3, 3, 3)], [RED]) == {(3, 3): RED}                                          # a point
    # sub-pixel end points: (2.5, 1.25) -> (4.5, 1.25) in sixteenths; pixel = round half up
    assert _draw([[40, 20, 72, 20, 1]], [RED]) == {(3, 1): RED, (4, 1): RED, (5, 1): RED}
    assert _draw([[0, 0, 64, 64, 0]], [RED]) == {}                                                # not valid


def test_crossing_segments_the_higher_index_wins():
    h, v = (0, 3, 6, 3), (3, 0, 3, 6)
    a = _draw([h, v], [RED, GREEN])
    assert a[(3, 3)] == GREEN and a[(2, 3)] == RED and a[(3, 2)] == GREEN and len(a) == 13
    b = _draw([v, h], [GREEN, RED])
    assert b[(3, 3)] == RED and len(b) == 13


def test_projection_mirror_near_plane_and_guard():
    v = V()
    T = torch.eye(4, dtype=torch.float64)
    seg = torch.tensor([[[0.0, 0.0, 1.0], [0.5, 0.0, 1.0]],           # in view: (4, 4) -> (9, 4) at f = 10, c = 4
                        [[0.0, 0.0, -1.0], [0.5, 0.0, -0.2]],         # wholly behind the near plane
                        [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]],          # half behind: ends on the near plane, same pixel
                        [[50.0, 0.0, 1.0], [60.0, 0.0, 1.0]]],        # far outside the guard rectangle
                       dtype=torch.float64)
    ep = v.overlay_project_torch(seg, T, 10.0, 10.0, 4.0, 4.0, 8, 8, near_z=0.01)
    assert ep[0].tolist() == [64, 64, 144, 64, 1]
    assert ep[1].tolist() == [0, 0, 0, 0, 0] and ep[3].tolist() == [0, 0, 0, 0, 0]
    assert ep[2].tolist() == [64, 64, 64, 64, 1]
    frame = v.overlay_draw_torch(torch.zeros(8, 8, 3, dtype=torch.uint8), ep, torch.tensor([RED] * 4, dtype=torch.uint8))
    assert sorted(map(tuple, torch.nonzero(frame[:, :, 0]).tolist())) == [(4, x) for x in range(4, 8)]
    # a segment that crosses the whole guard rectangle is cut to it: at most 2 W steps
    wide = torch.tensor([[[-1000.0, 0.0, 1.0], [1000.0, 0.0, 1.0]]], dtype=torch.float64)
    e = v.overlay_project_torch(wide, T, 10.0, 10.0, 4.0, 4.0, 8, 8)[0].tolist()
    assert e == [-64, 64, 192, 64, 1]


# ---- follow-camera and frustum ---------------------------------------------------------------------------------------
def _pose():
    from monogs_amd.pose import SE3_exp
    return SE3_exp(torch.tensor([0.3, -0.2, 0.5, 0.2, -0.1, 0.15])).double()        # world -> camera


def test_frustum_geometry():
    v = V()
    size = 0.02
    pose = torch.linalg.inv(_pose())
    pts = v.frustum_points(pose, size)
    hand = [(0, 0, 0), (1, -0.5, 2), (-1, -0.5, 2), (1, 0.5, 2), (-1, 0.5, 2)]
    for p, h in zip(pts, hand):
        want = pose[:3, :3] @ (torch.tensor(h, dtype=torch.float64) * size) + pose[:3, 3]
        assert torch.allclose(p, want, atol=1e-12)
    assert v.FRUSTUM_LINES == ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (2, 4), (3, 4))
    segs = v.world_segments(pose[None], torch.zeros(0, 2, 3, dtype=torch.float64), size)
    assert segs.shape == (8, 2, 3)
    for s, (i, j) in zip(segs, v.FRUSTUM_LINES):
        assert torch.allclose(s[0], pts[i], atol=1e-12) and torch.allclose(s[1], pts[j], atol=1e-12)
    free = torch.arange(12, dtype=torch.float64).reshape(2, 2, 3)
    assert torch.equal(v.world_segments(pose[None], free, size)[8:], free)


@pytest.mark.parametrize("behind", [True, False])
def test_follow_camera(behind):
    v = V()
    T, size, H, W, fov = _pose(), 0.05, 48, 64, 1.0
    cam = v.follow_camera(T.float(), H, W, fov, size, behind=behind)
    pose = torch.linalg.inv(T)
    base = torch.tensor([0.0, -2.5, -30.0, 1.0] if behind else [0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
    base[:3] *= size
    eye = (pose @ base)[:3]
    far = torch.stack([(pose @ torch.tensor([sx * size, sy * size, 2 * size, 1.0], dtype=torch.float64))[:3]
                       for sx, sy in ((1, -0.5), (-1, -0.5), (1, 0.5), (-1, 0.5))])
    center, up = far.mean(dim=0), far[1] - far[3]
    Tv = cam.T.double()
    R, t = Tv[:3, :3], Tv[:3, 3]
    assert torch.allclose(R @ R.t(), torch.eye(3, dtype=torch.float64), atol=1e-5) and torch.det(R) > 0.999
    assert torch.allclose(-R.t() @ t, eye, atol=1e-5)                           # the camera sits at the eye
    c = R @ center + t
    assert abs(c[0]) < 1e-5 and abs(c[1]) < 1e-5 and c[2] > 0                   # and looks at the centre
    u = R @ up
    assert abs(u[0]) < 1e-5 * up.norm() and u[1] < 0                            # `up` points up the image (-y)
    assert cam.image_height == H and cam.image_width == W
    assert math.isclose(cam.fy, H / (2 * math.tan(0.5 * fov))) and cam.fx == cam.fy and cam.cx == 0.5 * W
    assert math.isclose(cam.FoVy, fov, rel_tol=1e-6)
    if not behind:                                                              # view_dir is the tracked camera itself
        assert torch.allclose(Tv, T, atol=1e-5)


# ---- time shader -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_time_colors_mirror_against_the_formula(K):
    v = V()
    g = torch.Generator().manual_seed(5)
    N = 300
    feats = torch.randn(N, K, 3, generator=g)
    ids = torch.randint(3, 40, (N,), generator=g, dtype=torch.int32)
    ids[0], ids[1] = 3, 39
    got = v.time_colors_torch(feats, ids)
    t = (ids.numpy().astype(np.float32) - np.float32(3)) / np.float32(36)
    idx = np.minimum(255, (np.clip(t, 0, 1) * np.float32(256)).astype(np.int64))
    tint = np.float32(0.9) * (v.JET_LUT[idx].astype(np.float32) / np.float32(255))
    want = np.float32(0.1) * feats.numpy() + tint[:, None, :]
    assert got.shape == (N, K, 3) and np.array_equal(got.numpy(), want)
    same = v.time_colors_torch(feats, torch.full((N,), 7, dtype=torch.int32))          # all ids equal: t = 0
    tint0 = np.float32(0.9) * (v.JET_LUT[0].astype(np.float32) / np.float32(255))
    assert np.array_equal(same.numpy(), np.float32(0.1) * feats.numpy() + tint0[None, None, :])


# ---- the CPU route, saving -------------------------------------------------------------------------------------------
def test_view_frame_torch_cpu_route_and_save(tmp_path):
    from monogs_amd import synthetic as S
    from monogs_amd.slam_loops import GaussianParams
    v = V()
    W, H = 48, 32
    sc = S.make_scene(200, W, H, seed=2)
    gm = GaussianParams(sc.means3D, sc.log_scales, sc.rot, sc.opacity_logit + 2.0, sc.features_dc)
    gm.unique_kfIDs = torch.arange(200, dtype=torch.int32) // 40
    cam = v.make_view_camera(torch.eye(4), H, W, sc.cam.fx, sc.cam.fy, sc.cam.cx, sc.cam.cy)
    pose = torch.eye(4)
    pose[2, 3] = 1.0                                                     # a keyframe one metre ahead
    frames = {m: v.view_frame_torch(m, gaussians=gm, camera=cam, keyframes=pose[None], frustum_size=0.1) for m in v.MODES}
    for m, f in frames.items():
        assert f.dtype == torch.uint8 and f.shape == (H, W, 3), m
        assert (f == torch.tensor(v.COLOR_KEYFRAME, dtype=torch.uint8)).all(dim=2).sum() > 8, m     # the frustum is drawn
    assert not torch.equal(frames["rgb"], frames["time"]) and not torch.equal(frames["rgb"], frames["flat_ball"])
    # the brute-force blend against the oracle's rasteriser
    from conftest import oracle_settings
    from oracle import torch_raster as O
    m3, s, r, o, sh = S.activated(sc._replace(opacity_logit=sc.opacity_logit + 2.0))
    img = O.rasterize(m3, None, sh, None, o, s, r, None, oracle_settings(sc.cam, sc.bg))[0]
    proj = v.project_torch(gm, cam)
    assert (v.blend_torch(proj, H, W, sc.bg)[0] - img).abs().max() < 1e-4
    path = v.save_frame(str(tmp_path / "a.ppm"), frames["rgb"])
    raw = open(path, "rb").read()
    assert raw.startswith(b"P6\n48 32\n255\n") and raw[13:] == frames["rgb"].numpy().tobytes()
    png = v.save_frame(str(tmp_path / "a.png"), frames["depth"])
    assert os.path.getsize(png) > 0
    with pytest.raises(ValueError):
        v.save_frame(str(tmp_path / "b.ppm"), torch.zeros(3, 4, 4))


# ---- exports ---------------------------------------------------------------------------------------------------------
def test_exports_and_abi_version():
    from monogs_amd import _cabi
    names = ("mgs_view_compose", "mgs_view_ellipsoid", "mgs_view_time_colors", "mgs_view_overlay",
             "mgs_view_compose_args_size", "mgs_view_ellipsoid_args_size", "mgs_view_time_colors_args_size",
             "mgs_view_overlay_args_size", "mgs_view_compose_scratch_bytes", "mgs_view_time_colors_scratch_bytes",
             "mgs_view_overlay_scratch_bytes")
    for n in names:
        assert n in _cabi.EXPORTS, n
    assert _cabi.ABI_VERSION == 10


def test_view_entry_points_reject_bad_arguments(built):
    import ctypes as C
    from monogs_amd import _cabi
    L = _cabi.lib()
    assert L.mgs_view_compose(None, None) == -1 and L.mgs_view_overlay(None, None) == -1
    assert L.mgs_view_time_colors(None, None) == -1 and L.mgs_view_ellipsoid(None, None) == -1
    a = _cabi.ViewComposeArgs()
    a.width, a.height, a.mode = 46341, 46341, _cabi.VIEW_RGB                     # H * W * 3 past 2^31
    a.src = a.out = 4096
    assert L.mgs_view_compose(C.byref(a), None) == -3
    assert L.mgs_view_overlay_scratch_bytes(46341, 46341) == 0 and L.mgs_view_overlay_scratch_bytes(64, 48) == 64 * 48 * 4
    assert L.mgs_view_compose_scratch_bytes() == 256 and L.mgs_view_time_colors_scratch_bytes() == 512
