"""CPU tests of the offline evaluation helpers."""
import os

import numpy as np
import torch

from monogs_amd import eval_metrics as E


def _rand_rot(g):
    q = torch.randn(4, generator=g).double().numpy()
    return E._quat_xyzw_to_matrix(q)


def test_umeyama_recovers_a_similarity_and_ate_is_zero():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 40, generator=g).double().numpy()
    R0, t0, c0 = _rand_rot(g), np.array([0.3, -1.2, 2.0]), 1.7
    y = c0 * R0 @ x + t0[:, None]
    R, t, c = E.umeyama_alignment(x, y, with_scale=True)
    assert np.allclose(R, R0, atol=1e-10) and np.allclose(t, t0, atol=1e-10) and abs(c - c0) < 1e-10
    # rigid-only alignment of a scaled copy leaves a residual; of an unscaled copy none
    R, t, c = E.umeyama_alignment(x, R0 @ x + t0[:, None], with_scale=False)
    assert c == 1.0 and np.allclose(R, R0, atol=1e-10)

    def poses(pts):
        out = []
        for k in range(pts.shape[1]):
            T = np.eye(4)
            T[:3, 3] = pts[:, k]
            out.append(T)
        return out
    s = E.ate_statistics(poses(y), poses(x), monocular=True)
    assert s["rmse"] < 1e-9
    s = E.ate_statistics(poses(y), poses(x), monocular=False)     # scale 1.7 not corrected
    assert s["rmse"] > 0.1
    noisy = y + 0.01 * torch.randn(3, 40, generator=g).double().numpy()
    s = E.ate_statistics(poses(noisy), poses(x), monocular=True)
    assert 0.005 < s["rmse"] < 0.03 and s["min"] <= s["median"] <= s["max"]


def test_reflection_case_returns_a_proper_rotation():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 12, generator=g).double().numpy()
    x[2] *= 1e-3                                   # nearly planar: the SVD sign is ambiguous
    y = np.diag([1.0, 1.0, -1.0]) @ x
    R, t, c = E.umeyama_alignment(x, y, with_scale=False)
    assert abs(np.linalg.det(R) - 1.0) < 1e-9


def test_psnr_matches_the_reference_helper_and_ssim_properties():
    g = torch.Generator().manual_seed(1)
    a = torch.rand(2, 3, 24, 32, generator=g)
    b = (a + 0.05 * torch.randn(2, 3, 24, 32, generator=g)).clamp(0, 1)
    want = 20 * torch.log10(1.0 / torch.sqrt(((a - b) ** 2).reshape(2, -1).mean(1, keepdim=True)))
    assert torch.allclose(E.psnr(a, b), want)
    # what the reference's own PSNR returned on the same inputs (tests/golden/make_psnr_golden.py)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_psnr.npz"))
    ga, gb = torch.from_numpy(gold["a"]), torch.from_numpy(gold["b"])
    assert torch.allclose(a, ga, rtol=0, atol=1e-6) and torch.allclose(b, gb, rtol=0, atol=1e-6)
    assert torch.allclose(E.psnr(ga, gb), torch.from_numpy(gold["psnr"]))
    assert abs(E.ssim(a, a).item() - 1.0) < 1e-6
    s_ab = E.ssim(a, b).item()
    assert 0.3 < s_ab < 1.0 and abs(s_ab - E.ssim(b, a).item()) < 1e-6
    assert E.ssim(a, b, size_average=False).shape == (2,)
    # The definition (ref gaussian_splatting/utils/loss_utils.py:61-101 - pure torch, but the module
    # imports cv2, so it is restated here rather than imported) evaluated by hand at an interior
    # pixel and at two border pixels, where the window hangs over the ZERO padding.
    img1, img2 = a[:1, :1], b[:1, :1]
    H, W = img1.shape[-2:]
    w = E._gauss_window(11, 1.5, 1, img1)[0, 0]
    smap = E.ssim_map(img1, img2)
    assert smap.shape == img1.shape

    def by_hand(y, x):
        p1, p2 = torch.zeros(11, 11), torch.zeros(11, 11)
        for dy in range(11):
            for dx in range(11):
                yy, xx = y + dy - 5, x + dx - 5
                if 0 <= yy < H and 0 <= xx < W:
                    p1[dy, dx], p2[dy, dx] = img1[0, 0, yy, xx], img2[0, 0, yy, xx]
        mu1, mu2 = (w * p1).sum(), (w * p2).sum()
        s11, s22 = (w * p1 * p1).sum() - mu1 ** 2, (w * p2 * p2).sum() - mu2 ** 2
        s12 = (w * p1 * p2).sum() - mu1 * mu2
        return ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s11 + s22 + 9e-4))

    for (y, x) in ((10, 13), (0, 0), (H - 1, 3)):
        want = by_hand(y, x)
        assert torch.isfinite(want) and abs(smap[0, 0, y, x].item() - want.item()) < 2e-5, (y, x)
    assert abs(E.ssim(img1, img2).item() - smap.mean().item()) < 1e-7
    assert torch.allclose(E.ssim(a, b, size_average=False), E.ssim_map(a, b).reshape(2, -1).mean(1), atol=1e-6)


def test_tum_sequence_reader(tmp_path):
    from PIL import Image
    d = tmp_path / "seq"
    (d / "rgb").mkdir(parents=True)
    (d / "depth").mkdir()
    rgb_lines, dep_lines, gt_lines = ["# color images"], ["# depth maps"], ["# ground truth trajectory"]
    for i in range(6):
        t = 100.0 + i * 0.02              # 50 Hz: the 32 fps sub-sampling drops every other frame
        Image.fromarray(np.full((4, 6, 3), 40 * i, np.uint8)).save(d / "rgb" / f"{i}.png")
        Image.fromarray(np.full((4, 6), 5000 * (i + 1), np.uint16)).save(d / "depth" / f"{i}.png")
        rgb_lines.append(f"{t:.4f} rgb/{i}.png")
        dep_lines.append(f"{t + 0.003:.4f} depth/{i}.png")
        gt_lines.append(f"{t + 0.001:.4f} {i * 0.1} 0 0 0 0 0 1")
    rgb_lines.append("200.0 rgb/0.png")     # no depth / pose within 0.08 s: dropped
    (d / "rgb.txt").write_text("\n".join(rgb_lines))
    (d / "depth.txt").write_text("\n".join(dep_lines))
    (d / "groundtruth.txt").write_text("\n".join(gt_lines))
    seq = E.TUMSequence(str(d))
    assert len(seq) == 3 and seq.color_paths[1].endswith("2.png")
    img, dep, T = seq[1]
    assert img.shape == (3, 4, 6) and abs(img[0, 0, 0].item() - 80 / 255) < 1e-6
    assert abs(dep[0, 0].item() - 3.0) < 1e-6
    assert torch.allclose(T[:3, 3], torch.tensor([-0.2, 0.0, 0.0]))      # inverse of the camera-to-world pose


def test_eval_ate_and_rendering_drivers(tmp_path):
    class F_:
        pass
    g = torch.Generator().manual_seed(4)
    frames = []
    for i in range(8):
        f = F_()
        f.uid = i
        Tg = torch.eye(4)
        Tg[:3, 3] = torch.randn(3, generator=g)
        f.T_gt = Tg
        f.T = Tg.clone()
        f.T[:3, 3] += 0.01 * torch.randn(3, generator=g)
        frames.append(f)
    rmse = E.eval_ate(frames, [0, 2, 4, 6, 7], save_dir=str(tmp_path), final=True, monocular=False)
    assert 0 < rmse < 0.05 and (tmp_path / "plot" / "stats_final.json").exists()
    gt = [torch.rand(3, 16, 20, generator=g) for _ in range(8)]
    dataset = [(im, None, None) for im in gt]

    def render_fn(frame, gaussians, pipe, bg):
        return {"render": gt[frame.uid] * 0.9}
    out = E.eval_rendering(frames, None, dataset, render_fn, None, None, kf_indices=[0], interval=5)
    assert out["mean_lpips"] is None and 15 < out["mean_psnr"] < 40 and 0.8 < out["mean_ssim"] < 1.0


def test_tracking_best_iterate_bookkeeping_on_a_toy_renderer(monkeypatch):
    """slam_loops.track_frame (the reference-shaped loop of slam_frontend.py:455-822) on the CPU with
    a differentiable toy `render`: the criterion is torch.norm(residual, p=1) of
    losses.get_loss_tracking_per_pixel (:510), the returned state is the best iterate's and the
    returned render_pkg is the one rendered there (:523-528, :819-822)."""
    import math
    from monogs_amd import slam_loops as SL
    from monogs_amd.losses import get_loss_tracking_per_pixel
    H, W = 12, 16
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")

    def toy_render(vp, gaussians, pipe, bg, forward_sketch_args=None):
        t = vp.T[:3, 3] + vp.cam_trans_delta + 0.3 * vp.cam_rot_delta
        img = torch.stack([torch.sigmoid(0.3 * (xs - 8) + 4 * t[0]), torch.sigmoid(0.3 * (ys - 6) + 4 * t[1]),
                           torch.sigmoid(0.2 * (xs + ys - 14) + 4 * t[2])])
        return {"render": img, "depth": torch.ones(1, H, W), "opacity": torch.ones(1, H, W),
                "n_touched": torch.zeros(1), "viewspace_points": None, "visibility_filter": None, "radii": None}

    monkeypatch.setattr(SL, "render", toy_render)
    P = torch.eye(4)
    fov = 2 * math.atan(1.0)

    def cam(T):
        v = SL.ViewCamera(1, torch.zeros(3, H, W), T, P, fov, fov, H, W, "cpu")
        v.original_image = toy_render(SL.ViewCamera(0, torch.zeros(3, H, W), torch.eye(4), P, fov, fov, H, W, "cpu"),
                                      None, None, None)["render"].detach()
        v.rgb_pixel_mask_mapping = torch.ones(1, H, W, dtype=torch.bool)
        return v

    T0 = torch.eye(4)
    T0[:3, 3] = torch.tensor([0.05, -0.04, 0.03])
    cfg = {"Training": dict(SL.DEFAULT_CONFIG["Training"])}
    cfg["Training"]["lr"] = {"cam_rot_delta": 0.05, "cam_trans_delta": 0.05, "exposure_a": 0.02, "exposure_b": 0.02}
    # by hand
    v = cam(T0)
    opt = SL.make_pose_optimizer(v, cfg)
    l1s, Ts = [], []
    for _ in range(20):
        Ts.append(v.T.clone())
        pk0 = toy_render(v, None, None, None)
        want = torch.norm(get_loss_tracking_per_pixel(cfg, pk0["render"], pk0["depth"], pk0["opacity"], v).flatten(), p=1)
        _, _, pkg = SL.tracking_step_first_order(v, None, opt, None, SL.Pipe, cfg)
        assert abs(float(pkg["tracking_l1"]) - float(want.detach())) <= 1e-5 * float(want.detach())
        l1s.append(float(want.detach()))
    k = min(range(20), key=lambda i: l1s[i])
    assert 0 < k < 19 and l1s[-1] > l1s[k]                   # overshoot: the last iterate is not the best
    v2 = cam(T0)
    pkg, best, it, n = SL.track_frame(v2, None, None, first_order_iters=20, second_order_iters=0, config=cfg)
    assert it == k and n == 20 and abs(best - l1s[k]) <= 1e-6 * l1s[k]
    assert torch.allclose(v2.T, Ts[k]) and float(v2.cam_trans_delta.abs().sum()) == 0.0
    v2.cam_trans_delta.data.zero_()
    assert torch.allclose(pkg["render"], toy_render(v2, None, None, None)["render"], atol=1e-6)
    v3 = cam(T0)
    SL.track_frame(v3, None, None, first_order_iters=20, second_order_iters=0, use_best_loss=False, config=cfg)
    assert torch.allclose(v3.T, v.T)
