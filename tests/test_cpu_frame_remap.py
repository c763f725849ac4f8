"""Undistortion / rectification without a GPU: the mirror alone (frame_prepare.remap_build_numpy, remap_torch,
remap_depth_torch) against arithmetic written out here, and TUMSequence(calibration=...).  Parity with cv2 is unpinned
(DESIGN.md "Undistort and rectify on the device"): what is checked is this repository's own contract."""
import os

import numpy as np
import pytest
import torch

from monogs_amd import frame_prepare as FP
import remap_cases as RC


def grid(H, W):
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    return u, v


@pytest.mark.parametrize("H,W", [(2, 2), (45, 70), (480, 640)])
def test_identity_map_returns_the_input(H, W):
    cal = RC.calibration_for(H, W)
    K = RC.camera_matrix(*RC.intrinsics(cal))
    ir, m = FP.remap_build_numpy(H, W, K, (0.0,) * 5, R=np.eye(3), new_K=K)
    u, v = grid(H, W)
    assert m.dtype == np.int32 and m.shape == (H, W, 2) and ir.shape == (9,)
    assert np.array_equal(m[..., 0], 32 * u) and np.array_equal(m[..., 1], 32 * v)
    f = RC.make_image(H, W, 7)
    q = RC.make_image(H, W, 7, quantised=True)
    got_f, got_q = FP.remap_torch(f, m), FP.remap_torch(q, m)
    assert got_f.dtype == torch.float32 and torch.equal(got_f.view(torch.int32), f.view(torch.int32))
    assert got_q.dtype == torch.uint8 and torch.equal(got_q, q)


def shift_map(H=45, W=70):
    K, new_K = RC.shift_case(H, W)
    ir, m = FP.remap_build_numpy(H, W, K, (0.0,) * 5, new_K=new_K)
    return m


def test_subpixel_shift_against_hand_arithmetic():
    H, W = 45, 70
    m = shift_map(H, W)
    u, v = grid(H, W)
    assert np.array_equal(m[..., 0], 32 * u - 168) and np.array_equal(m[..., 1], 32 * v - 80)
    assert int((m[..., 0] < 0).sum()) == 270 and int((m[..., 1] < 0).sum()) == 210
    q = RC.make_image(H, W, 11, quantised=True)
    assert torch.equal(FP.remap_torch(q, m), RC.shift_by_hand(q))
    f = RC.make_image(H, W, 11)
    assert torch.equal(FP.remap_torch(f, m).view(torch.int32), RC.shift_by_hand(f).view(torch.int32))


def model_fp64(H, W, cal):
    """The distortion model written plainly: where the test calibration puts destination pixel (u, v) in the source."""
    u, v = grid(H, W)
    x, y = (u - cal["cx"]) / cal["fx"], (v - cal["cy"]) / cal["fy"]
    r2 = x * x + y * y
    k1, k2, p1, p2, k3 = RC.FR1_DIST
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return cal["fx"] * xd + cal["cx"], cal["fy"] * yd + cal["cy"]


@pytest.mark.parametrize("H,W", [(45, 70), (480, 640)])
def test_map_follows_the_distortion_model(H, W):
    cal = RC.calibration_for(H, W)
    _, m = RC.distorted_map(H, W)
    none, partly = RC.coverage(m)
    u, v = grid(H, W)
    scale = float(W + 2 * H)
    ramp = torch.from_numpy(((u + 2 * v) / scale).astype(np.float32))
    got = FP.remap_torch(ramp[None].expand(3, H, W).contiguous(), m)
    mx, my = model_fp64(H, W, cal)
    want = (mx + 2 * my) / scale
    inside = ~(none | partly)
    assert inside.sum() > 0.8 * H * W
    # one 1/64-pixel quantisation per axis times the ramp's slopes (bilinear blending reproduces a linear image), plus
    # the fp32 rounding of four products and three sums
    bound = 3 / 64 / scale + 1e-6
    err = np.abs(got.numpy().astype(np.float64) - want[None])[:, inside].max()
    print(f"{H}x{W}: ramp through the map against the model: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    assert bool((got[:, torch.from_numpy(none)] == 0).all())


def test_depth_nearest_against_hand_arithmetic():
    H, W = 45, 70
    m = shift_map(H, W)
    d = torch.rand(H, W, generator=torch.Generator().manual_seed(5)) + 0.5
    got = FP.remap_depth_torch(d, m)
    assert torch.equal(got, RC.shift_depth_by_hand(d))
    assert torch.equal(FP.remap_depth_torch(d[None], m), RC.shift_depth_by_hand(d)[None])
    out = FP.prepare_frame_torch(RC.make_image(H, W, 3), d, dataset_type="tum", edge_threshold=1.1, remap=m,
                                 remap_depth=True)
    assert torch.equal(out["gt_depth"][0], RC.shift_depth_by_hand(d))
    assert torch.equal(out["image"], RC.shift_by_hand(RC.make_image(H, W, 3)))
    keep = FP.prepare_frame_torch(RC.make_image(H, W, 3), d, dataset_type="tum", edge_threshold=1.1, remap=m)
    assert torch.equal(keep["gt_depth"][0], d)                   # the default: the reference remaps the image only


def test_sentinel_for_a_vanishing_denominator():
    H, W = 8, 12
    ir = np.array([1 / 64, 0, -0.1, 0, 1 / 64, -0.05, 0, 0.25, -0.75])          # Wd = 0 on row 3
    _, m = FP.remap_build_numpy(H, W, (64.0, 64.0, 6.0, 4.0), RC.FR1_DIST, ir=ir)
    assert (m[3] == -FP.MAP_CLAMP).all() and not (m[[0, 1, 2, 4, 5, 6, 7]] == -FP.MAP_CLAMP).all(axis=-1).any()
    assert np.abs(m.astype(np.int64)).max() <= FP.MAP_CLAMP
    img = RC.make_image(H, W, 1, quantised=True)
    assert bool((FP.remap_torch(img, m)[3] == 0).all())


def write_sequence(folder, n=3, H=16, W=24):
    from PIL import Image
    os.makedirs(os.path.join(folder, "rgb"))
    os.makedirs(os.path.join(folder, "depth"))
    rng = np.random.default_rng(0)
    lines = {"rgb.txt": [], "depth.txt": [], "groundtruth.txt": []}
    images = []
    for k in range(n):
        t = 1.0 + k / 10.0                                       # (below the reader's 32 frames per second)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(img).save(os.path.join(folder, "rgb", f"{k}.png"))
        Image.fromarray(rng.integers(500, 30000, (H, W)).astype(np.uint16)).save(os.path.join(folder, "depth", f"{k}.png"))
        lines["rgb.txt"].append(f"{t:.4f} rgb/{k}.png")
        lines["depth.txt"].append(f"{t:.4f} depth/{k}.png")
        lines["groundtruth.txt"].append(f"{t:.4f} {0.01 * k} 0 0 0 0 0 1")
        images.append(img)
    for name, rows in lines.items():
        with open(os.path.join(folder, name), "w") as f:
            f.write("# header\n" + "\n".join(rows) + "\n")
    return images


def test_tum_sequence_undistorts_on_the_host(tmp_path):
    from monogs_amd.eval_metrics import TUMSequence
    H, W = 16, 24
    folder = str(tmp_path / "seq")
    images = write_sequence(folder, 3, H, W)
    cal = RC.calibration_for(H, W)
    plain = TUMSequence(folder)
    flat = TUMSequence(folder, calibration=RC.calibration_for(H, W, distorted=False))
    und = TUMSequence(folder, calibration=cal)
    assert len(plain) == len(und) == 3
    _, m = FP.remap_build_numpy(H, W, RC.intrinsics(cal), RC.FR1_DIST)
    none, partly = RC.coverage(m)          # (at 16x24 the distortion pushes no destination pixel wholly outside)
    assert partly.any() and not none.all()
    for k in range(3):
        raw = torch.from_numpy(images[k])
        for seq in (plain, flat, und):
            assert torch.equal(seq.image_u8(k), raw)
        as_float = lambda u8: torch.from_numpy(u8.numpy().astype(np.float32) / 255.0).permute(2, 0, 1)
        assert torch.equal(plain.image(k), as_float(raw)) and torch.equal(flat.image(k), as_float(raw))
        want = as_float(FP.remap_torch(raw, m))
        assert torch.equal(und.image(k), want) and not torch.equal(want, as_float(raw))
        assert torch.equal(und[k][0], want) and torch.equal(und[k][1], plain[k][1])


def test_load_sequence_passes_the_calibration_on(tmp_path, monkeypatch):
    from monogs_amd import slam_surrogate as SS
    H, W = 16, 24
    folder = str(tmp_path / "seq")
    images = write_sequence(folder, 3, H, W)
    monkeypatch.setenv("MONOGS_TUM_DIR", folder)
    cal = RC.calibration_for(H, W)
    frames, cam, _ = SS.load_sequence(3, W, H, "cpu", calibration=cal)
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == RC.intrinsics(cal) and (cam.H, cam.W) == (H, W)
    _, m = FP.remap_build_numpy(H, W, RC.intrinsics(cal), RC.FR1_DIST)
    for k, fr in enumerate(frames):
        want = FP.remap_torch(torch.from_numpy(images[k]), m).numpy().astype(np.float32) / 255.0
        assert torch.equal(fr.image, torch.from_numpy(want).permute(2, 0, 1))
        assert fr.undistorted
    as_float = lambda a: torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1)
    plain, plain_cam, _ = SS.load_sequence(3, W, H, "cpu")
    assert torch.equal(plain[0].image, as_float(images[0])) and not plain[0].undistorted and plain_cam.fx != cam.fx
    # raw=True: the frames as they are on disk with the calibration's camera - run_sequence's native remap takes these
    raw, raw_cam, _ = SS.load_sequence(3, W, H, "cpu", calibration=cal, raw=True)
    assert (raw_cam.fx, raw_cam.cy) == (cam.fx, cam.cy)
    assert all(torch.equal(f.image, as_float(images[k])) and not f.undistorted for k, f in enumerate(raw))
    flat, _, _ = SS.load_sequence(3, W, H, "cpu", calibration=RC.calibration_for(H, W, distorted=False))
    assert not flat[0].undistorted and torch.equal(flat[0].image, as_float(images[0]))
