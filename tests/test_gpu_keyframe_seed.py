"""mgs_keyframe_seed (keyframe_seed.hip) on the MI355X against the torch mirror of the same five steps
(monogs_amd/keyframe_seed.seed_torch, itself pinned to the reference by tests/test_cpu_keyframe_seed.py) with replayed
noise and keys, the k-nn scale against the oracle (including the Replica-shaped point counts that take the Q = 2 and
Q = 4 k-nn kernels), the call's own generator, argument checks, and run_sequence through the seeder end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from monogs_amd import _cabi
from monogs_amd import keyframe_seed as KS
from test_cpu_keyframe_seed import BAND_CAP, EPS, make_cam, threshold_band

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def f32_bits(x):
    return np.float32(x).view(np.uint32)


def make_frame(H, W, seed, holes=True):
    """A frame with a dark border, a rendered depth with far outliers and holes, regions that are not opaque."""
    g = torch.Generator().manual_seed(seed)
    image = 0.05 + 0.9 * torch.rand(3, H, W, generator=g)
    b = max(1, H // 12)
    image[:, :b, :] = 0.0
    image[:, :, -b:] = 0.003
    depth = 1.0 + 3.0 * torch.rand(H, W, generator=g)
    far = torch.rand(H, W, generator=g) < 0.03
    depth[far] *= 3.0
    opacity = 0.955 + 0.045 * torch.rand(H, W, generator=g)
    if holes:
        depth[torch.rand(H, W, generator=g) < 0.05] = 0.0
        depth[H // 3:H // 2, W // 4:W // 2] = 0.0
        opacity[H // 2:, :W // 3] = 0.5
        depth[H - 1, 0] = float("nan")               # in the region that is not opaque: never behind the statistics
        depth[H - 1, 1] = float("inf")
        depth[H - 1, 2] = -1.0
    noise = torch.randn(H, W, generator=g)
    keys = torch.randint(0, 2 ** 32, (H * W,), generator=g, dtype=torch.int64)
    return tuple(t.to(DEV) for t in (image, depth, opacity, noise, keys))


def config(downsample=64, downsample_init=32, adaptive=True):
    return {"Dataset": {"pcd_downsample": downsample, "pcd_downsample_init": downsample_init, "point_size": 0.01,
                        "adaptive_pointsize": adaptive}, "Training": {"rgb_boundary_threshold": 0.01}}


def log_scale_bound(dist2_want, point_size):
    """(expected log-scale, tolerance): test_knn_dist2's tolerance on dist2 (rtol 1e-4, atol 1e-7) carried through
    0.5 log(max(dist2, 1e-7) point_size), plus four fp32 roundings (product, sqrt, log, the point size itself)."""
    w = dist2_want.double()
    wc = w.clamp_min(1e-7)
    want = 0.5 * torch.log(wc * float(point_size))
    tol = 0.5 * torch.log1p((1e-7 + 1e-4 * w) / wc) + 4 * EPS * want.abs().clamp_min(1.0)
    return want, tol


def check_log_scales(log_scales, xyz, point_size):
    from oracle import torch_raster as O
    want, tol = log_scale_bound(O.dist2_knn3(xyz.cpu()), point_size)
    err = (log_scales[:, 0].double().cpu() - want).abs()
    print(f"log_scales: {xyz.shape[0]} points, max |err| {float(err.max()):.3g}, min slack {float((tol - err).min()):.3g}")
    assert bool((err <= tol).all())
    assert bool((log_scales == log_scales[:, :1]).all())


def close16(a, b):
    return bool(((a - b).abs() <= 16 * EPS * b.abs().clamp_min(1.0)).all())


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("size", [(120, 160), (480, 640), (53, 75)])
def test_replay_matches_the_torch_mirror(built, mode, size):
    H, W = size
    image, depth, opacity, noise, keys = make_frame(H, W, seed=H + mode)
    cam = make_cam(H, W, DEV)
    init = mode == 1
    S = KS.KeyframeSeeder(H, W, DEV, config())
    ds = 32 if init else 64
    xyz, feats, ls, rots, opac, r = S.seed(cam, image, depth, opacity, mode, init, seed=1, noise=noise, keys=keys)
    m = KS.seed_torch(cam, image, depth, opacity, mode, downsample=ds, noise=noise, keys=keys)
    K = int(r.num_points)
    band = torch.zeros(H, W, dtype=torch.bool)
    if mode == 0:
        v = depth[m["valid_mask"]]
        std64, std_ref = float(v.double().std()), float(v.std())          # fp64 evaluation; torch's own fp32 reduction
        dist, dist_ref = abs(r.std_depth - std64), abs(std_ref - std64)
        band = threshold_band(depth, m["median_depth"].item(), m["std_depth"].item(), r.std_depth)
        print(f"{H}x{W}: std native {r.std_depth:.9g} mirror {float(m['std_depth']):.9g} torch fp32 {std_ref:.9g} fp64 "
              f"{std64:.12g}: |native - fp64| {dist:.3g}, |fp32 - fp64| {dist_ref:.3g}; band {int(band.sum())} pixels")
        assert f32_bits(r.median_depth) == f32_bits(m["median_depth"].item())
        assert r.n_valid == m["n_valid"]
        assert dist <= 4 * dist_ref
        assert int(band.sum()) <= BAND_CAP * H * W
        if not band.any():
            assert r.n_outliers == m["n_outliers"]
    else:
        assert math.isnan(r.median_depth) and math.isnan(r.std_depth) and r.n_valid == 0
    assert torch.equal(S.depth_out.cpu()[~band], m["depth"].cpu()[~band])
    # a flipped outlier test would move everything below; for these (deterministic) inputs no pixel sits on the threshold
    assert not band.any()
    assert f32_bits(r.median_all) == f32_bits(m["median_all"].item())
    assert r.n_depth == m["n_depth"] and K == int(m["n_depth"] / ds) == m["sel"].numel()
    assert K > 0
    assert torch.equal(S.pixel_index[:K].long(), m["sel"])
    assert abs(r.point_size - m["point_size"]) <= EPS * m["point_size"]
    assert close16(xyz, m["xyz"])
    assert close16(feats[:, :, 0], m["features_dc"])
    assert torch.equal(rots, m["rots"]) and torch.equal(opac, m["opacity_logit"])
    assert feats.shape == (K, 3, 1) and ls.shape == (K, 1)
    check_log_scales(ls, xyz, r.point_size)


def test_median_all_edge_cases(built):
    """Odd and even pixel counts, more than half of the map zero, negative sensor values, the two middle values in
    different radix buckets."""
    for H, W, kind in ((5, 7, "odd"), (6, 8, "even"), (48, 64, "mostly_zero"), (48, 64, "negative"), (2, 2, "far_apart")):
        g = torch.Generator().manual_seed(H * W)
        image = torch.full((3, H, W), 0.5, device=DEV)
        d = (0.5 + 3 * torch.rand(H, W, generator=g)).to(DEV)
        if kind == "mostly_zero":
            d[torch.rand(H, W, generator=g).to(DEV) < 0.7] = 0.0
        if kind == "negative":
            d[torch.rand(H, W, generator=g).to(DEV) < 0.6] *= -1.0
        if kind == "far_apart":
            d = torch.tensor([[0.001, 3.0], [700.0, 1e-30]], device=DEV)
        S = KS.KeyframeSeeder(H, W, DEV, config(downsample=2, downsample_init=2))
        r = S.seed(make_cam(H, W, DEV), image, d, None, KS.MODE_SENSOR, False, seed=0)[-1]
        want = np.median(d.cpu().numpy())
        assert f32_bits(r.median_all) == f32_bits(want), (kind, r.median_all, want)
        assert abs(r.point_size - min(0.05, 0.01 * float(want))) <= EPS * 0.05
        n = int(((d > 0) & (d <= 100)).sum())
        assert r.n_depth == n and r.num_points == n // 2


TIE_KEY = 0x40000000
SELECT_EDGE_CASES = ("ties_at_threshold", "all_keys_equal", "prior_0_valid", "prior_1_valid", "prior_2_valid",
                     "no_depth_zero", "no_depth_beyond_trunc", "downsample_1")


@pytest.mark.parametrize("case", SELECT_EDGE_CASES)
def test_select_outputs_at_their_edges(built, case):
    """Where the radix select's rank, `any` and total decide the result: sampling keys tied at the K-th smallest (the
    ties cross wave segments: 53 x 75 is 63 segments of 64 pixels), one key for every pixel, a depth prior of 0 / 1 / 2
    valid pixels, no usable depth at all, and K = n (the rank is the last element)."""
    H, W = (5, 7) if case == "downsample_1" else (53, 75)
    ds = 1 if case == "downsample_1" else 2
    g = torch.Generator().manual_seed(len(case) + H)
    cam = make_cam(H, W, DEV)
    image = torch.full((3, H, W), 0.5)
    depth = 0.5 + 3 * torch.rand(H, W, generator=g)
    noise = torch.randn(H, W, generator=g)
    keys = torch.randint(0, 2 ** 32, (H * W,), generator=g, dtype=torch.int64)
    S = KS.KeyframeSeeder(H, W, DEV, config(downsample=ds, downsample_init=ds))

    if case.startswith("prior_"):
        n = int(case.split("_")[1])
        image[:, :4, :] = 0.0                              # no image content: never valid, depth 0 afterwards
        opacity = torch.full((H, W), 0.5)
        opacity[2, 9] = 0.99                               # opaque, but without image content
        for y, x in ((7, 70), (40, 3))[:n]:                # in different wave segments
            opacity[y, x] = 0.99
        image, depth, opacity, noise = (t.to(DEV) for t in (image, depth, opacity, noise))
        r = S.seed(cam, image, depth, opacity, KS.MODE_RENDERED, False, seed=1, noise=noise, keys=keys)[-1]
        d, info = KS.depth_prior_torch(image, depth, opacity, KS.MODE_RENDERED, noise)
        assert info["n_valid"] == n and r.n_valid == n
        if n == 0:
            assert math.isnan(r.median_depth)
        else:
            assert f32_bits(r.median_depth) == f32_bits(info["median_depth"].item())
        if n < 2:
            assert math.isnan(r.std_depth)
        else:
            # two values: both sides hold the same exact fp64 sums, so only the fp64 square root and the one rounding
            # to fp32 can differ
            want = info["std_depth"].item()
            print(f"std native {r.std_depth:.9g} mirror {want:.9g}")
            assert abs(r.std_depth - want) <= EPS * want
        assert torch.equal(S.depth_out, d)
        usable = int(((d > 0) & (d <= 100)).sum())
        assert r.n_depth == usable and r.num_points == usable // ds
        return

    if case == "no_depth_zero":
        depth = torch.zeros(H, W)
    if case == "no_depth_beyond_trunc":
        depth = depth + 150.0
    if case in ("ties_at_threshold", "all_keys_equal", "downsample_1"):
        depth.view(-1)[torch.randperm(H * W, generator=g)[: max(2, H * W // 5)]] = 0.0
    if case == "ties_at_threshold":
        keys[torch.rand(H * W, generator=g) < 0.5] = TIE_KEY
    if case == "all_keys_equal":
        keys[:] = TIE_KEY
    image, depth = image.to(DEV), depth.to(DEV)
    out = S.seed(cam, image, depth, None, KS.MODE_SENSOR, False, seed=1, keys=keys)      # raises unless the call is OK
    r = out[-1]
    want_med = np.median(depth.cpu().numpy())
    assert f32_bits(r.median_all) == f32_bits(want_med)
    flat = depth.reshape(-1).cpu()
    usable = (flat > 0) & (flat <= 100)
    n = int(usable.sum())
    K = int(n / ds)
    assert r.n_depth == n and r.num_points == K == out[0].shape[0]
    if case.startswith("no_depth"):
        assert n == 0 and K == 0
        return
    sel, n_sel = KS.select_torch(depth, keys, ds)
    assert n_sel == n and sel.numel() == K > 0
    if case == "ties_at_threshold":
        below, upto = int((keys[usable] < TIE_KEY).sum()), int((keys[usable] <= TIE_KEY).sum())
        print(f"usable {n}, K {K}, keys below the tie {below}, up to it {upto}")
        assert below < K <= upto
    if case == "all_keys_equal":
        assert torch.equal(sel.cpu(), torch.nonzero(usable).reshape(-1)[:K])          # the first K in pixel order
    if case == "downsample_1":
        assert K == n < H * W
    assert torch.equal(S.pixel_index[:K].long(), sel)


@pytest.mark.parametrize("downsample,holes", [(64, False), (32, False), (64, True)])
def test_replica_shape_scales_against_the_oracle(built, downsample, holes):
    """1200x680 sensor depth: 12 750 / 25 500 points take k_knn_partial<2> / <4>; the hole pattern makes the count a
    non-multiple of 256 and of 8."""
    H, W = 680, 1200
    g = torch.Generator().manual_seed(downsample + holes)
    image = (0.1 + 0.8 * torch.rand(3, H, W, generator=g)).to(DEV)
    u = torch.linspace(-1, 1, W)[None, :]
    v = torch.linspace(-1, 1, H)[:, None]
    depth = (2.5 + 0.8 * u + 0.5 * v * v + 0.05 * torch.rand(H, W, generator=g))
    want_n = H * W
    if holes:
        depth.view(-1)[: 64 * 251 + 63] = 0.0            # n = 816 000 - 16 127: K = 12 498 = 48 * 256 + 210, 210 % 8 = 2
        want_n -= 64 * 251 + 63
    S = KS.KeyframeSeeder(H, W, DEV, config(downsample=downsample, downsample_init=downsample))
    xyz, feats, ls, rots, opac, r = S.seed(make_cam(H, W, DEV), image, depth.to(DEV), None, KS.MODE_SENSOR, False, seed=9)
    K = want_n // downsample
    assert r.n_depth == want_n and r.num_points == K == xyz.shape[0]
    if holes:
        assert K % 256 and K % 8
    else:
        assert K == {64: 12750, 32: 25500}[downsample]
    assert bool(torch.isfinite(xyz).all())
    check_log_scales(ls, xyz, r.point_size)


def chi_square_quantile(dof, z):
    """Wilson-Hilferty: the chi-square quantile at the normal deviate z."""
    return dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3


def test_own_generator(built):
    H, W = 480, 640
    image, depth, opacity, _, _ = make_frame(H, W, seed=77)
    cam = make_cam(H, W, DEV)
    S = KS.KeyframeSeeder(H, W, DEV, config())

    def call(mode, init, seed):
        out = S.seed(cam, image, depth, opacity, mode, init, seed=seed)
        K = out[-1].num_points
        return [t.clone() for t in out[:5]] + [S.depth_out.clone(), S.pixel_index[:K].clone(),
                                                bytes(memoryview(out[-1]))]

    a, b, c = call(0, False, 5), call(0, False, 5), call(0, False, 6)
    for x, y in zip(a[:-1], b[:-1]):
        assert torch.equal(x, y)                                  # bit-identical, every output
    assert a[-1] == b[-1]
    assert not torch.equal(a[6], c[6]) and not torch.equal(a[5], c[5])        # another seed: other pixels, other noise
    r = _cabi.KeyframeSeedResult.from_buffer_copy(a[-1])
    assert r.num_points == int(r.n_depth / 64) == a[6].numel()
    assert r.n_depth == int(((a[5] > 0) & (a[5] <= 100)).sum())
    assert bool((a[6][1:] > a[6][:-1]).all())                     # ascending pixel order, no pixel twice
    # the normal draws, recovered from mode 1: d = 2 + 0.3 z on every pixel
    m1 = call(1, True, 1234)
    r1 = _cabi.KeyframeSeedResult.from_buffer_copy(m1[-1])
    z = ((m1[5].double() - 2.0) / 0.3).reshape(-1)
    n = z.numel()
    mean, var = float(z.mean()), float(z.var())
    print(f"noise: n {n} mean {mean:.3g} (bound {5 / math.sqrt(n):.3g}) var {var:.6g} (bound {5 * math.sqrt(2 / n):.3g})")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1.0) <= 5 * math.sqrt(2 / n)
    # the selection over a 16 x 16 grid of image blocks against uniform: every pixel is usable in mode 1, the blocks
    # hold 40 x 30 pixels each, so each expects K / 256 (37.5) points; 255 degrees of freedom, level 1e-6 (z = 4.7534)
    K = r1.num_points
    assert r1.n_depth == H * W and K == H * W // 32
    sel = m1[6].long()
    cell = (sel // W) // (H // 16) * 16 + (sel % W) // (W // 16)
    counts = torch.bincount(cell, minlength=256).double()
    chi2 = float(((counts - K / 256) ** 2 / (K / 256)).sum())
    bound = chi_square_quantile(255, 4.7534)
    print(f"selection: chi-square {chi2:.1f} over 256 blocks (bound {bound:.1f})")
    assert chi2 <= bound


def test_bad_arguments_leave_everything_untouched(built):
    H, W = 48, 64
    image, depth, opacity, noise, keys = make_frame(H, W, seed=3)
    cam = make_cam(H, W, DEV)
    S = KS.KeyframeSeeder(H, W, DEV, config())
    outs = (S.xyz, S.features_dc, S.log_scales, S.rots, S.opacity_logit, S.depth_out)
    for t in outs:
        t.fill_(-7.0)
    S.pixel_index.fill_(-7)
    S.result.fill_(0xA5)
    C.memset(C.byref(S.record), 0x5A, C.sizeof(S.record))
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    cases = (("xyz", None), ("log_scales", None), ("result", None), ("row_capacity", H * W // 64 - 1),
             ("downsample", 0.0), ("downsample", -1.0), ("downsample", 0.5), ("downsample", float("nan")),
             ("depth", None), ("mode", 7), ("scratch", S.scratch.data_ptr() + 8))
    for field, bad in cases:
        a, keep = S.native_args(cam, image, depth, opacity, 0, False, 1, noise, keys)
        setattr(a, field, bad)
        assert _cabi.lib().mgs_keyframe_seed(C.byref(a), stream) == -1, field
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == -7.0).all())
    assert bool((S.pixel_index == -7).all()) and bool((S.result == 0xA5).all())
    assert bytes(memoryview(S.record)) == b"\x5a" * C.sizeof(S.record)
    # and the same seeder still works
    r = S.seed(cam, image, depth, opacity, 0, False, 1, noise, keys)[-1]
    assert r.num_points == int(r.n_depth / 64) > 0


def test_run_sequence_through_the_seeder_640x480(built, monkeypatch):
    from monogs_amd import keyframe_policy as KP
    from monogs_amd import slam_surrogate as SS
    from monogs_amd.gaussian_model import GaussianModel
    n = 21
    frames, cam, source = SS.load_sequence(n, 640, 480, DEV)
    added = {}
    inner = GaussianModel.extend_from_keyframe

    def counted(self, *a, **k):
        before = len(self)
        rec = inner(self, *a, **k)
        added[k["kf_id"]] = (len(self) - before, rec)
        return rec

    monkeypatch.setattr(GaussianModel, "extend_from_keyframe", counted)
    P = KP.KeyframePolicy(monocular=True)
    res = SS.run_sequence(frames, cam, DEV, init_iters=300, mapping_iters=60, keyframe_policy=P,
                          native_keyframe_seed=True)
    torch.cuda.synchronize()
    kfs = res["kf_ids"]
    print(source, "keyframes", kfs, "resets", res["resets"],
          {k: (rows, rec.n_depth, round(rec.median_depth, 3), round(rec.point_size, 5)) for k, (rows, rec) in added.items()})
    assert res["capacity_ok"]
    assert set(kfs) <= set(added) and set(added) == set(res["seed_records"])
    for k, (rows, rec) in added.items():
        first = k == 0 or k in res["resets"]
        assert rows == rec.num_points == int(rec.n_depth / (32 if first else 64)) > 0
        assert first or (rec.n_valid > 0 and math.isfinite(rec.median_depth) and math.isfinite(rec.std_depth))
    assert len(added) >= 2
    assert all(torch.isfinite(c.T).all() for c in res["cameras"].values())
    ev = SS.evaluate(res, frames, DEV, monocular=True)
    print(ev)
    assert ev["ate_rmse_m"] < 0.03 * ev["path_length_m"]
