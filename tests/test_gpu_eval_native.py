"""Evaluation on the device: the scorer mgs_eval_score against the reference's own numbers (tests/golden/
refine_loss_ref.npz, map_update_ref.npz) and against eval_metrics.psnr / ssim evaluated in double on the same fp32
inputs; NativeEvaluator, eval_rendering_native and slam_surrogate.evaluate(native=True) against the PyTorch paths.

Bounds.  PSNR 1e-3 dB: an fp32 sum of at most 1e6 non-negative terms in any fixed order is within 2.3e-4 relative even
for a 1024-term serial run per thread, and d(dB) = 4.34 x the relative error.  L1 and depth L1 1e-4 relative by the same
argument.  SSIM 2e-5 (the bound test_gpu_color_refinement.py holds k_ssim_loss to); 2e-6 on map_update_ref.npz's cases,
that file's existing bound.  Sizes: 7x9 is smaller than the window, 33x65 is one pixel past a tile edge in both
directions (the tile is 32x16), 45x70 is off the tile grid, 64x96 is whole tiles only."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_mapping import _window_fixture

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "refine_loss_ref.npz")
MAP_GOLD = os.path.join(HERE, "golden", "map_update_ref.npz")
SIZES = ((7, 9), (33, 65), (45, 70), (64, 96))
PSNR_TOL, REL_TOL, SSIM_TOL = 1e-3, 1e-4, 2e-5
EXPOSURE = (-0.9, 0.03, 1e-4)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def score_args(image, gt, depth=None, gt_depth=None, exposure=None, row=0, table=None, partial=None):
    from monogs_amd import _cabi
    dev = image.device
    _, H, W = image.shape
    if table is None:
        table = torch.zeros(1, _cabi.EVAL_RECORD_DOUBLES, dtype=torch.float64, device=dev)
    if partial is None:
        partial = torch.zeros(int(_cabi.lib().mgs_eval_score_partial_count(H, W)), device=dev)
    a = _cabi.EvalScoreArgs()
    a.height, a.width, a.row, a.num_rows = H, W, row, table.shape[0]
    a.gt_format = _cabi.EVAL_GT_U8_HWC if gt.dtype == torch.uint8 else _cabi.EVAL_GT_F32_CHW
    a.image, a.gt, a.partial, a.table = image.data_ptr(), gt.data_ptr(), partial.data_ptr(), table.data_ptr()
    keep = [image, gt, depth, gt_depth, table, partial]
    if depth is not None:
        a.depth, a.gt_depth = depth.data_ptr(), gt_depth.data_ptr()
    if exposure is not None:
        ea, eb = torch.tensor([exposure[0]], device=dev), torch.tensor([exposure[1]], device=dev)
        a.apply_exposure, a.exposure_eps, a.exposure_a, a.exposure_b = 1, exposure[2], ea.data_ptr(), eb.data_ptr()
        keep += [ea, eb]
    return a, table, partial, keep


def score(image, gt, **kw):
    """Raw ABI call: the record table as a NumPy array (the ticket is checked to be restored)."""
    from monogs_amd import _cabi
    image = image.float().contiguous()
    gt = gt.contiguous()
    for k in ("depth", "gt_depth"):
        if kw.get(k) is not None:
            kw[k] = kw[k].float().contiguous()
    a, table, partial, keep = score_args(image, gt, **kw)
    _cabi.check(_cabi.lib().mgs_eval_score(C.byref(a), _stream(image.device)), "mgs_eval_score")
    torch.cuda.synchronize()
    assert int(partial[-1:].view(torch.int32)) == 0          # the ticket is restored
    return table.cpu().numpy()


def scores(rec, H, W):
    from monogs_amd.eval_native import scores_from_records
    return {k: v[0] for k, v in scores_from_records(rec, H * W).items()}


def fp64_reference(image, gt, exposure=None):
    """eval_metrics.psnr over gt > 0 and eval_metrics.ssim in double, on the fp32 x the kernel is specified to form."""
    from monogs_amd import eval_metrics as E
    x = image.float()
    if exposure is not None:
        a, b, eps = (torch.tensor(v, dtype=torch.float32, device=x.device) for v in exposure)
        x = (torch.abs(a) + eps) * x + b
    x, y = x.clamp(0, 1).double(), gt.double()
    mask = y > 0
    with np.errstate(all="ignore"):
        p = float(E.psnr(x[mask].unsqueeze(0), y[mask].unsqueeze(0)))
    return {"psnr": p, "ssim": float(E.ssim(x.unsqueeze(0), y.unsqueeze(0))), "l1": float((x - y).abs().mean()),
            "n_mask": int(mask.sum())}


def check_scores(got, want):
    if math.isnan(want["psnr"]) or math.isinf(want["psnr"]):
        assert str(got["psnr"]) == str(want["psnr"]), (got["psnr"], want["psnr"])
    else:
        assert abs(got["psnr"] - want["psnr"]) <= PSNR_TOL, (got["psnr"], want["psnr"])
    assert abs(got["ssim"] - want["ssim"]) <= SSIM_TOL, (got["ssim"], want["ssim"])
    assert abs(got["l1"] - want["l1"]) <= REL_TOL * abs(want["l1"]), (got["l1"], want["l1"])


def make_case(H, W, kind, dev):
    g = torch.Generator(device=dev).manual_seed(1000 * H + W)
    img = -0.2 + 1.5 * torch.rand(3, H, W, device=dev, generator=g)          # the clamp is live at both ends
    u8 = torch.randint(1, 256, (H, W, 3), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    u8 = torch.where(torch.rand(H, W, 3, device=dev, generator=g) < 0.3, torch.zeros_like(u8), u8)   # ~30 % exactly 0
    if kind == "zero_channel":
        u8[:, :, 1] = 0
    elif kind == "empty_mask":
        u8.zero_()
    # the dataset's conversion (eval_metrics.TUMSequence.image): NumPy's IEEE fp32 division on the host - a GPU tensor's
    # `/ 255` multiplies by the rounded reciprocal and is one ulp off for some values
    gt = torch.from_numpy(u8.cpu().numpy().astype(np.float32) / 255.0).permute(2, 0, 1).contiguous().to(dev)
    if kind == "equal_on_mask":
        img = torch.where(gt > 0, gt, img)
    return img, gt, u8


@pytest.mark.parametrize("case", ("c3_120x160", "c3_45x70", "c3_7x9", "same_45x70"))
def test_scorer_matches_the_reference_loss_numbers(built, case):
    G = np.load(GOLD)
    dev = _dev()
    img = torch.from_numpy(G[f"{case}_image"]).to(dev)
    gt = torch.from_numpy(G[f"{case}_gt"]).to(dev) if f"{case}_gt" in G.files else img.clone()
    assert float(img.min()) >= 0 and float(img.max()) <= 1           # the clamp is the identity
    _, H, W = img.shape
    s = scores(score(img, gt), H, W)
    want_ssim = float(G[f"{case}_ssim"]) if f"{case}_ssim" in G.files else 1.0
    want_l1 = float(G[f"{case}_l1"]) if f"{case}_l1" in G.files else 0.0
    print(case, "ssim", s["ssim"], want_ssim, "l1", s["l1"], want_l1)
    assert abs(s["ssim"] - want_ssim) <= 2e-5
    assert abs(s["l1"] - want_l1) <= 1e-6


def test_scorer_matches_the_reference_scoring_numbers(built):
    G = np.load(MAP_GOLD)
    dev = _dev()
    for i in range(G["ssim_a"].shape[0]):
        a, b = torch.from_numpy(G["ssim_a"][i]).to(dev), torch.from_numpy(G["ssim_b"][i]).to(dev)
        s = scores(score(a.clamp(0, 1), b), a.shape[1], a.shape[2])
        assert float(a.min()) >= 0 and float(a.max()) <= 1
        assert abs(s["ssim"] - float(G["ssim_per_image"][i])) <= 2e-6, (i, s["ssim"], float(G["ssim_per_image"][i]))


CASES = [(H, W, "base") for H, W in SIZES] + [(45, 70, k) for k in ("zero_channel", "empty_mask", "equal_on_mask")]


@pytest.mark.parametrize("H,W,kind", CASES)
def test_scorer_against_fp64(built, H, W, kind):
    from monogs_amd import _cabi
    dev = _dev()
    img, gt, u8 = make_case(H, W, kind, dev)
    rec = score(img, gt)
    want = fp64_reference(img, gt)
    got = scores(rec, H, W)
    print(H, W, kind, got, want)
    assert int(rec[0, _cabi.EVAL_N_MASK]) == want["n_mask"]
    if kind == "empty_mask":
        assert math.isnan(want["psnr"])
    if kind == "equal_on_mask":
        assert math.isinf(want["psnr"]) and want["psnr"] > 0
    check_scores(got, want)
    # psnr_all: image_utils.py:19-21 over every element
    x, y = img.clamp(0, 1).double(), gt.double()
    assert abs(got["psnr_all"] - float(10 * torch.log10(1.0 / ((x - y) ** 2).mean()))) <= PSNR_TOL
    # a uint8 [H,W,3] ground truth gives the record of the float gt = u8 / 255, bit for bit
    rec8 = score(img, u8)
    assert np.array_equal(rec8.view(np.uint64), rec.view(np.uint64))
    # exposure: the record of the pre-transformed image
    a, b, eps = (torch.tensor(v, dtype=torch.float32, device=dev) for v in EXPOSURE)
    pre = (torch.abs(a) + eps) * img + b
    rec_e = score(img, gt, exposure=EXPOSURE)
    check_scores(scores(rec_e, H, W), scores(score(pre, gt), H, W))
    check_scores(scores(rec_e, H, W), fp64_reference(img, gt, EXPOSURE))


@pytest.mark.parametrize("H,W", ((33, 65), (45, 70)))
def test_depth_sums(built, H, W):
    from monogs_amd import _cabi
    dev = _dev()
    img, gt, _ = make_case(H, W, "base", dev)
    g = torch.Generator(device=dev).manual_seed(H)
    depth = 0.5 + 4 * torch.rand(H, W, device=dev, generator=g)
    gd = 0.5 + 4 * torch.rand(H, W, device=dev, generator=g)
    gd[:3], gd[-3:], gd[:, :3], gd[:, -3:] = 0, 0, 0, 0                      # a zero border
    gd[torch.rand(H, W, device=dev, generator=g) < 0.1] = 0                   # zero holes
    rec = score(img, gt, depth=depth, gt_depth=gd)
    plain = score(img, gt)
    m = gd > 0
    want = float((depth.double() - gd.double()).abs()[m].sum())
    assert int(rec[0, _cabi.EVAL_N_DEPTH]) == int(m.sum()) > 0
    assert abs(rec[0, _cabi.EVAL_DEPTH_ABS] - want) <= REL_TOL * want
    assert abs(scores(rec, H, W)["depth_l1"] - want / int(m.sum())) <= REL_TOL * want / int(m.sum())
    colour = [_cabi.EVAL_SSE, _cabi.EVAL_SSE_ALL, _cabi.EVAL_ABS, _cabi.EVAL_SSIM, _cabi.EVAL_N_MASK]
    assert np.array_equal(rec[:, colour].view(np.uint64), plain[:, colour].view(np.uint64))
    assert plain[0, _cabi.EVAL_DEPTH_ABS] == 0 and plain[0, _cabi.EVAL_N_DEPTH] == 0 and plain[0, _cabi.EVAL_PAIRS] == 0


def test_scorer_crosses_the_group_limit(built):
    """283x325 has 3 x 11 x 18 = 594 tiles of 32x16, more than the 512 workgroups of a launch: 82 workgroups walk a
    second tile (the staged tile and the moment planes in LDS are reused behind the loop's closing barrier)."""
    from monogs_amd import _cabi
    dev = _dev()
    H, W = 283, 325
    assert int(_cabi.lib().mgs_eval_score_partial_count(H, W)) == 7 * 512 + 1 and 3 * 11 * 18 > 512
    img, gt, u8 = make_case(H, W, "base", dev)
    g = torch.Generator(device=dev).manual_seed(9)
    depth, gd = 4 * torch.rand(H, W, device=dev, generator=g), 4 * torch.rand(H, W, device=dev, generator=g)
    gd[torch.rand(H, W, device=dev, generator=g) < 0.2] = 0
    rec = score(img, u8, depth=depth, gt_depth=gd)
    want = fp64_reference(img, gt)
    print(H, W, scores(rec, H, W), want)
    assert int(rec[0, _cabi.EVAL_N_MASK]) == want["n_mask"] and int(rec[0, _cabi.EVAL_N_DEPTH]) == int((gd > 0).sum())
    check_scores(scores(rec, H, W), want)
    d = float((depth.double() - gd.double()).abs()[gd > 0].sum())
    assert abs(rec[0, _cabi.EVAL_DEPTH_ABS] - d) <= REL_TOL * d
    assert np.array_equal(score(img, u8, depth=depth, gt_depth=gd).view(np.uint64), rec.view(np.uint64))


def test_scorer_is_deterministic_and_writes_one_row(built):
    from monogs_amd import _cabi
    dev = _dev()
    H, W = 120, 160
    img, gt, _ = make_case(H, W, "base", dev)
    table = torch.full((4, _cabi.EVAL_RECORD_DOUBLES), -7.0, dtype=torch.float64, device=dev)
    a, table, partial, keep = score_args(img, gt, row=2, table=table)
    lib = _cabi.lib()
    _cabi.check(lib.mgs_eval_score(C.byref(a), _stream(dev)), "mgs_eval_score")
    first = table.cpu().numpy().copy()
    assert int(partial[-1:].view(torch.int32)) == 0
    table[2] = -7.0
    _cabi.check(lib.mgs_eval_score(C.byref(a), _stream(dev)), "mgs_eval_score")     # the same partial buffer again
    second = table.cpu().numpy()
    assert int(partial[-1:].view(torch.int32)) == 0
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    assert (first[[0, 1, 3]] == -7.0).all() and (first[2, :_cabi.EVAL_N_DEPTH] != -7.0).all()
    assert np.array_equal(first[2:3].view(np.uint64), score(img, gt).view(np.uint64))


def test_argument_checks_launch_nothing(built):
    from monogs_amd import _cabi
    dev = _dev()
    lib = _cabi.lib()
    img, gt, _ = make_case(7, 9, "base", dev)
    table = torch.full((2, _cabi.EVAL_RECORD_DOUBLES), -7.0, dtype=torch.float64, device=dev)

    def status(change, **kw):
        a, _, _, keep = score_args(img, gt, table=table, **kw)
        change(a)
        return lib.mgs_eval_score(C.byref(a), _stream(dev))

    assert lib.mgs_eval_score(None, _stream(dev)) == -1
    for field in ("image", "gt", "partial", "table"):
        assert status(lambda a: setattr(a, field, None)) == -1, field
    assert status(lambda a: setattr(a, "row", 2)) == -1 and status(lambda a: setattr(a, "row", -1)) == -1
    assert status(lambda a: setattr(a, "gt_format", 2)) == -1
    assert status(lambda a: setattr(a, "depth", img.data_ptr())) == -1          # depth without gt_depth
    assert status(lambda a: setattr(a, "apply_exposure", 1)) == -1              # exposure without a / b
    assert status(lambda a: setattr(a, "height", 0)) == -1
    # more tiles than an int indexes: unsupported.  The size function is asked FIRST, so that a size the library does
    # accept never reaches a launch on these small buffers.
    big = 1 << 20
    assert lib.mgs_eval_score_partial_count(big, big) == -1

    def too_big(a):
        a.height, a.width = big, big

    assert status(too_big) == -3
    # mgs_eval_view: null blocks (a score block whose H x W is not the forward's: below, on a valid block)
    assert lib.mgs_eval_view(None, _stream(dev)) == -1
    v = _cabi.EvalViewArgs()
    assert lib.mgs_eval_view(C.byref(v), _stream(dev)) == -1
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == -7.0).all()
    from monogs_amd.eval_native import NativeEvaluator
    _, gm, views = _window_fixture(N=500, W=64, H=48, n_views=1, seed=3, dev=dev)
    ev = NativeEvaluator(gm, torch.zeros(3, device=dev), 48, 64, dev, max_views=1)
    with pytest.raises(RuntimeError, match="begin"):
        ev.score(views[0], views[0].original_image)
    ev.begin()
    with pytest.raises(ValueError, match="gt_image"):
        ev.score(views[0], torch.zeros(3, 48, 63))
    with pytest.raises(ValueError, match="gt_depth"):
        ev.score(views[0], views[0].original_image, gt_depth=torch.zeros(47, 64))
    # H x W mismatch at the ABI: the block a score() would send, valid in everything but the score block's size (only
    # ever SMALLER than the buffers), returns a status and launches nothing - table and outputs keep their sentinels
    job = ev._make_job(views[0], views[0].original_image, None, False)
    ev.table.fill_(-7.0)
    for t in (ev.color, ev.depth, ev.opacity, ev.view_m, ev.full_m):
        t.fill_(-7.0)
    for field, value in (("width", 63), ("height", 47)):
        a = ev._view_args(0, job)
        setattr(a.score, field, value)
        assert lib.mgs_eval_view(C.byref(a), _stream(dev)) == -1, field
    a = ev._view_args(0, job)
    a.T = None
    assert lib.mgs_eval_view(C.byref(a), _stream(dev)) == -1
    a = ev._view_args(0, job)
    a.score.row = 1                                              # beyond the one-row table
    assert lib.mgs_eval_view(C.byref(a), _stream(dev)) == -1
    torch.cuda.synchronize()
    for t in (ev.table, ev.color, ev.depth, ev.opacity, ev.view_m, ev.full_m):
        assert bool((t == -7.0).all())
    a = ev._view_args(0, job)                                    # and the same block untouched is accepted
    assert lib.mgs_eval_view(C.byref(a), _stream(dev)) == 0
    torch.cuda.synchronize()
    assert bool((ev.table[0, :4] != -7.0).all()) and bool((ev.color != -7.0).any())
    ev.score(views[0], views[0].original_image)
    with pytest.raises(RuntimeError, match="max_views"):
        ev.score(views[0], views[0].original_image)
    assert len(ev.finish()["psnr"]) == 1


# ---------------------------------------------------------------------------------------------- views of a map
@pytest.fixture(scope="module")
def world(built):
    """A small seeded map at 160x120 with 11 sensor-depth views, and the PyTorch path's scores of every view
    (computed once, shared, left unchanged)."""
    from monogs_amd import eval_metrics as E
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    dev = _dev()
    _, gm, views = _window_fixture(N=4000, W=160, H=120, n_views=11, seed=21, dev=dev, rgbd=True)
    bg = torch.zeros(3, device=dev)
    ref = []
    with torch.no_grad():
        for v in views:
            pkg = render(v, gm, Pipe, bg)
            x, y = pkg["render"].clamp(0, 1).double(), v.original_image.double()
            mask = y > 0
            gd = v.gt_depth[0].double()
            ref.append({"psnr": float(E.psnr(x[mask].unsqueeze(0), y[mask].unsqueeze(0))),
                        "ssim": float(E.ssim(x.unsqueeze(0), y.unsqueeze(0))), "l1": float((x - y).abs().mean()),
                        "depth_l1": float((pkg["depth"][0].double() - gd).abs()[gd > 0].mean())})
    return gm, views, bg, ref


def test_one_view_without_a_host_synchronisation(world, monkeypatch):
    from monogs_amd.eval_native import NativeEvaluator
    gm, views, bg, ref = world
    dev = _dev()
    ev = NativeEvaluator(gm, bg, 120, 160, dev, max_views=3)
    calls = {"sync": 0, "item": 0, "cpu": 0}
    T = torch.Tensor

    def counted(key, fn):
        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return f

    def counted_to(fn):                      # .to(...) counts when it brings a device tensor to the host
        def f(self, *a, **k):
            out = fn(self, *a, **k)
            if self.is_cuda and not out.is_cuda:
                calls["cpu"] += 1
            return out
        return f

    monkeypatch.setattr(torch.cuda, "synchronize", counted("sync", torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted("sync", torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", counted("sync", torch.cuda.Event.synchronize))
    for name in ("item", "tolist", "__float__", "__int__", "__bool__", "__index__"):    # every scalar read of a tensor
        monkeypatch.setattr(T, name, counted("item", getattr(T, name)))
    for name in ("cpu", "numpy"):
        monkeypatch.setattr(T, name, counted("cpu", getattr(T, name)))
    monkeypatch.setattr(T, "to", counted_to(T.to))
    ev.begin()
    v = views[3]
    assert ev.score(v, v.original_image, gt_depth=v.gt_depth) == 0
    assert ev.score(v, v.original_image) == 1
    assert ev.score(v, v.original_image, apply_exposure=True) == 2          # reads exposure_a / b / eps of the view
    assert calls == {"sync": 0, "item": 0, "cpu": 0}
    res = ev.finish()
    assert calls == {"sync": 0, "item": 0, "cpu": 2}           # the one copy of the table: .cpu().numpy()
    monkeypatch.undo()
    print({k: res[k] for k in ("psnr", "ssim", "l1", "depth_l1", "pairs")}, ref[3])
    got = {k: res[k][0] for k in ("psnr", "ssim", "l1", "depth_l1")}
    check_scores(got, ref[3])
    assert abs(got["depth_l1"] - ref[3]["depth_l1"]) <= REL_TOL * ref[3]["depth_l1"]
    assert math.isnan(res["depth_l1"][1]) and res["psnr"][1] == res["psnr"][0] and res["ssim"][1] == res["ssim"][0]
    assert 0 < res["pairs"][0] <= ev.capacity and ev.overflow_regrows == 0
    # the exposed row against the PyTorch path with the view's exposure (1.21, 0.05 in the fixture)
    from monogs_amd import eval_metrics as E
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    with torch.no_grad():
        x = ((torch.abs(v.exposure_a) + v.exposure_eps) * render(v, gm, Pipe, bg)["render"] + v.exposure_b).clamp(0, 1).double()
    y = v.original_image.double()
    check_scores({k: res[k][2] for k in ("psnr", "ssim", "l1")},
                 {"psnr": float(E.psnr(x[y > 0].unsqueeze(0), y[y > 0].unsqueeze(0))),
                  "ssim": float(E.ssim(x.unsqueeze(0), y.unsqueeze(0))), "l1": float((x - y).abs().mean())})
    assert res["psnr"][2] != res["psnr"][0]


@pytest.mark.parametrize("sh_degree,active", ((1, 1), (2, 1), (3, 3)))
def test_views_with_spherical_harmonics(built, sh_degree, active):
    """K > 1 stored coefficients: features_rest through mgs_map_activate, the shs buffer, an active degree above 0 (the
    view direction from campos, which render() and the evaluator both hand over as the view matrix, as the reference's
    camera_center is) - against render() through the scores."""
    from monogs_amd import eval_metrics as E
    from monogs_amd.eval_native import NativeEvaluator
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    dev = _dev()
    _, gm, views = _window_fixture(N=3000, W=96, H=64, n_views=2, seed=5 + sh_degree, dev=dev, rgbd=True,
                                   sh_degree=sh_degree, active_degree=active)
    bg = torch.full((3,), 0.1, device=dev)
    ev = NativeEvaluator(gm, bg, 64, 96, dev, max_views=2)
    ev.begin()
    for v in views:
        ev.score(v, v.original_image, gt_depth=v.gt_depth)
    res = ev.finish()
    for k, v in enumerate(views):
        with torch.no_grad():
            pkg = render(v, gm, Pipe, bg)
        x, y, gd = pkg["render"].clamp(0, 1).double(), v.original_image.double(), v.gt_depth[0].double()
        want = {"psnr": float(E.psnr(x[y > 0].unsqueeze(0), y[y > 0].unsqueeze(0))),
                "ssim": float(E.ssim(x.unsqueeze(0), y.unsqueeze(0))), "l1": float((x - y).abs().mean())}
        print(sh_degree, active, k, {n: res[n][k] for n in ("psnr", "ssim", "l1", "depth_l1")}, want)
        check_scores({n: res[n][k] for n in ("psnr", "ssim", "l1")}, want)
        d = float((pkg["depth"][0].double() - gd).abs()[gd > 0].mean())
        assert abs(res["depth_l1"][k] - d) <= REL_TOL * d
    # the colour does depend on the higher bands here: dropping them changes the score
    if active > 0:
        gm.active_sh_degree = 0
        ev.begin()
        ev.score(views[0], views[0].original_image)
        assert ev.finish()["l1"][0] != res["l1"][0]


def test_capacity_overflow_is_scored_again(world):
    from monogs_amd import _cabi
    from monogs_amd.eval_native import NativeEvaluator
    gm, views, bg, ref = world
    dev = _dev()
    out = {}
    for name, cap in (("small", 1024), ("large", 1 << 20)):
        ev = NativeEvaluator(gm, bg, 120, 160, dev, capacity=cap, max_views=3)
        ev.begin()
        for v in views[:3]:
            ev.score(v, v.original_image, gt_depth=v.gt_depth)
        out[name] = (ev.finish(), ev)
    small, large = out["small"], out["large"]
    assert (small[1].first_pass[:, _cabi.EVAL_PAIRS] > 1024).all() and small[1].overflow_regrows >= 1
    assert small[1].capacity >= small[0]["pairs"].max() and large[1].overflow_regrows == 0
    assert np.array_equal(small[0]["records"].view(np.uint64), large[0]["records"].view(np.uint64))
    for k in range(3):
        check_scores({n: small[0][n][k] for n in ("psnr", "ssim", "l1")}, ref[k])


@pytest.mark.parametrize("interval", (5, 2))
def test_eval_rendering_native_matches_eval_rendering(world, tmp_path, interval):
    from monogs_amd import eval_metrics as E
    from monogs_amd.eval_native import eval_rendering_native
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import Pipe
    gm, views, bg, ref = world
    dataset = [(v.original_image, v.gt_depth[0], None) for v in views]
    kf = [0, 5]
    want = E.eval_rendering(views, gm, dataset, render, Pipe, bg, kf, save_dir=str(tmp_path / "a"), interval=interval)
    got = eval_rendering_native(views, gm, dataset, Pipe, bg, kf, save_dir=str(tmp_path / "b"), interval=interval)
    print(interval, want, got)
    assert got["mean_lpips"] is None and want["mean_lpips"] is None
    chosen = [i for i in range(0, 10, interval) if i not in kf]
    if not chosen:                       # interval 5 with keyframes 0 and 5: nothing is left to score, on either path
        assert math.isnan(want["mean_psnr"]) and math.isnan(got["mean_psnr"]) and math.isnan(got["mean_ssim"])
        assert "mean_depth_l1" not in got
    else:
        assert abs(got["mean_psnr"] - want["mean_psnr"]) <= PSNR_TOL
        assert abs(got["mean_ssim"] - want["mean_ssim"]) <= SSIM_TOL
        d = float(np.mean([ref[i]["depth_l1"] for i in chosen]))
        assert abs(got["mean_depth_l1"] - d) <= REL_TOL * d
        # scored in batches of three views (two begin / finish pairs): the same records, so the same means
        assert eval_rendering_native(views, gm, dataset, Pipe, bg, kf, interval=interval, chunk=3) == got
    for sub in ("a", "b"):
        assert os.path.isfile(os.path.join(str(tmp_path / sub), "psnr", "final", "final_result.json"))


def test_surrogate_evaluate_native(built):
    from monogs_amd import slam_surrogate as SS
    dev = _dev()
    H, W, n = 48, 64, 7
    frames, cam, _ = SS.load_sequence(n, W, H, dev, world_gaussians=3000)
    cfg = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01},
           "Dataset": {"type": "tum", "pcd_downsample": 4, "pcd_downsample_init": 2}}
    res = SS.run_sequence(frames, cam, dev, sensor_depth=True, init_iters=20, mapping_iters=5, kf_interval=3,
                          first_order_iters=4, second_order_iters=0, config=cfg)
    torch.cuda.synchronize()
    a = SS.evaluate(res, frames, dev, monocular=False)
    b = SS.evaluate(res, frames, dev, monocular=False, native=True)
    print(a, b)
    assert set(a) <= set(b) and "ssim" not in a and "depth_l1_m" not in a
    assert a["psnr_frames"] == b["psnr_frames"] > 0 and a["gaussians"] == b["gaussians"]
    assert a["ate_rmse_m"] == b["ate_rmse_m"]
    assert abs(a["psnr_db"] - b["psnr_db"]) <= PSNR_TOL
    assert math.isfinite(b["ssim"]) and math.isfinite(b["depth_l1_m"]) and b["depth_l1_m"] > 0
    mono = SS.evaluate(res, frames, dev, monocular=True, native=True)
    assert "depth_l1_m" not in mono and mono["ssim"] == b["ssim"]
