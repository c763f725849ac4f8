"""mgs_keyframe_decide (keyframe_policy.hip) on the MI355X against the torch mirrors of the reference's keyframe policy
(monogs_amd/keyframe_policy.py): the radix-selected median bit for bit with torch.median, the covisibility counts
exactly, the decision on the reference fixture cases, run-to-run determinism, argument checks, and run_sequence with
the policy end to end (including a monocular reset)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from monogs_amd import _cabi
from monogs_amd import keyframe_policy as KP
from test_cpu_keyframe_policy import case_inputs, config_of, load_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def f32_bits(x):
    return np.float32(x).view(np.uint32)


def native(policy, cur, cams, window, n_touched, depth, opacity, occ, initialized=True):
    trk = types.SimpleNamespace(n_touched=n_touched, depth=depth, opacity=opacity)
    return policy._decide_native(cur, cams, window, trk, occ, initialized)


def single_view(N, depth, opacity, n_touched=None, rows=None):
    cams = {1: types.SimpleNamespace(T=torch.eye(4, device=DEV)), 0: types.SimpleNamespace(T=torch.eye(4, device=DEV))}
    nt = torch.ones(N, dtype=torch.int32, device=DEV) if n_touched is None else n_touched
    occ = {0: torch.ones(N, dtype=torch.uint8, device=DEV)} if rows is None else rows
    return cams, nt, occ


@pytest.mark.parametrize("kind", ["random_640x480", "ties", "n0", "n1", "n2", "odd", "even", "low_mantissa",
                                  "nan_and_inf", "tiny_image"])
def test_median_is_torch_median_bit_for_bit(built, kind):
    g = torch.Generator(device=DEV).manual_seed(sum(map(ord, kind)))
    H, W = (480, 640) if kind != "tiny_image" else (3, 5)
    depth = 0.2 + 6.0 * torch.rand(H, W, device=DEV, generator=g)
    opacity = torch.rand(H, W, device=DEV, generator=g)
    if kind == "ties":
        depth = torch.tensor([1.0, 1.25, 3.0], device=DEV)[torch.randint(0, 3, (H, W), device=DEV, generator=g)]
    elif kind in ("n0", "n1", "n2"):
        opacity.fill_(0.5)
        n = int(kind[1])
        opacity.view(-1)[torch.randperm(H * W, device=DEV, generator=g)[:n]] = 0.99
    elif kind in ("odd", "even"):
        opacity.fill_(0.5)
        n = 1001 if kind == "odd" else 1000
        opacity.view(-1)[torch.randperm(H * W, device=DEV, generator=g)[:n]] = 0.99
    elif kind == "low_mantissa":
        depth = (torch.full((H, W), 1.5, device=DEV).view(torch.int32)
                 + torch.randint(0, 7, (H, W), device=DEV, generator=g, dtype=torch.int32)).view(torch.float32)
    elif kind == "nan_and_inf":
        depth.view(-1)[::7] = float("nan")
        depth.view(-1)[::11] = float("inf")
        depth.view(-1)[::13] = -1.0
    if kind not in ("n0", "n1", "n2", "odd", "even"):
        depth[0, :3] = 0.0
    P = KP.KeyframePolicy()
    cams, nt, occ = single_view(17, depth, opacity)
    d = native(P, 1, cams, [0], nt, depth[None], opacity[None], occ)
    want = KP.median_depth(depth[None], opacity[None])
    n_valid = int(((depth > 0) & (opacity > 0.95)).sum())
    assert d.n_valid == n_valid
    if n_valid == 0:
        assert math.isnan(d.median_depth) and math.isnan(want.item())
    else:
        assert f32_bits(d.median_depth) == f32_bits(want.item()), (d.median_depth, want.item())


@pytest.mark.parametrize("N", [1, 63, 64, 65, 300_000, 1_000_003])
def test_counts_are_exact(built, N):
    g = torch.Generator(device=DEV).manual_seed(N)
    depth = torch.ones(1, 8, 8, device=DEV)
    opacity = torch.ones(1, 8, 8, device=DEV)
    P = KP.KeyframePolicy()
    for W in (1, 3, 7, 10):
        nt = torch.randint(-1, 3, (N,), device=DEV, generator=g, dtype=torch.int32)
        window = list(range(W, 0, -1))
        occ = {}
        for k, kf in enumerate(window):
            kind = k % 3
            if kind == 0:
                occ[kf] = torch.randint(0, 3, (N,), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
            elif kind == 1:
                occ[kf] = torch.zeros(N, dtype=torch.uint8, device=DEV)
            else:
                occ[kf] = torch.full((N,), 255, dtype=torch.uint8, device=DEV)
        if W == 7:   # rows at odd addresses: the scalar path
            big = torch.zeros(N + 1, dtype=torch.uint8, device=DEV)
            big[1:] = occ[window[0]]
            occ[window[0]] = big[1:]
        cams = {i: types.SimpleNamespace(T=torch.eye(4, device=DEV)) for i in window + [W + 5]}
        d = native(P, W + 5, cams, window, nt, depth, opacity, occ)
        cur = nt > 0
        assert d.n_cur == int(cur.sum())
        for k, kf in enumerate(window):
            row = occ[kf] != 0
            assert d.n_row[k] == int(row.sum()), (W, k)
            assert d.n_inter[k] == int((cur & row).sum()), (W, k)


@pytest.mark.parametrize("name", load_cases()[1])
def test_decision_matches_the_mirror_on_the_fixture(built, name):
    z, _ = load_cases()
    c = case_inputs(z, name, DEV)
    cfg = config_of(z)
    P = KP.KeyframePolicy(cfg, monocular=c["monocular"], single_thread=c["single_thread"])
    nt = c["cur_vis"].to(torch.int32) * 2
    d = native(P, c["cur"], c["cams"], c["window"], nt, c["depth"][None], c["opacity"][None], c["occ"],
               c["initialized"])
    med = KP.median_depth(c["depth"][None], c["opacity"][None])
    trace = {}
    m = KP.loop_decision(cfg, c["cams"], med, c["initialized"], c["monocular"], c["single_thread"], c["cur"],
                         c["window"], (nt > 0).long(), c["occ"], trace)
    assert d.create_kf == m["create_kf"] == bool(z[f"{name}_create_kf"])
    assert d.window == m["window"] == [int(v) for v in z[f"{name}_new_window"]]
    assert d.removed == m["removed"]
    assert d.reset == m["reset"]
    assert f32_bits(d.median_depth) == f32_bits(med.item()) or (math.isnan(d.median_depth) and math.isnan(med.item()))
    got, want = np.float32(d.overlap), np.float32(trace["overlap"].item())
    assert got.view(np.uint32) == want.view(np.uint32) or (np.isnan(got) and np.isnan(want))
    for kf, r in trace.get("ss_ratio", {}).items():
        got, want = np.float32(d.ss_ratio[c["window"].index(kf)]), np.float32(r.item())
        assert got.view(np.uint32) == want.view(np.uint32) or (np.isnan(got) and np.isnan(want)), kf
    np.testing.assert_allclose(d.dist, float(trace["dist"]), rtol=1e-6)
    if "scores" in trace:
        want = np.full(len(c["window"]), -1.0)
        for kf, s in trace["scores"].items():
            want[c["window"].index(kf)] = s
        np.testing.assert_allclose(np.array(d.scores), want, rtol=1e-6)
        np.testing.assert_allclose(np.array(d.scores), z[f"{name}_scores"], rtol=1e-6)
    else:
        assert all(s == -1.0 for s in d.scores)


def _fixture_args(P, name):
    z, _ = load_cases()
    c = case_inputs(z, name, DEV)
    trk = types.SimpleNamespace(n_touched=c["cur_vis"].to(torch.int32), depth=c["depth"][None],
                                opacity=c["opacity"][None])
    a, keep = P.native_args(c["cur"], c["cams"], c["window"], trk, c["occ"], c["initialized"])
    return a, keep


def test_two_calls_give_bit_identical_records(built):
    P = KP.KeyframePolicy()
    a, keep = _fixture_args(P, "over_full_cut_evict")
    lib = _cabi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    recs = []
    for _ in range(3):
        _cabi.check(lib.mgs_keyframe_decide(C.byref(a), stream), "mgs_keyframe_decide")
        torch.cuda.synchronize()
        recs.append(P._result.cpu().clone())
    assert torch.equal(recs[0], recs[1]) and torch.equal(recs[1], recs[2])
    # the scratch is left as it was found: histograms and ticket zero
    assert int(P._scratch[:20480 + 4].count_nonzero()) == 0


def test_bad_arguments_launch_nothing(built):
    P = KP.KeyframePolicy()
    a, keep = _fixture_args(P, "full_evict")
    lib = _cabi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P._result.fill_(0xAB)
    torch.cuda.synchronize()

    def status(mut):
        b = _cabi.KeyframeArgs.from_buffer_copy(a)
        mut(b)
        return lib.mgs_keyframe_decide(C.byref(b), stream)

    assert lib.mgs_keyframe_decide(None, stream) == -1
    assert status(lambda b: setattr(b, "n_touched", None)) == -1
    assert status(lambda b: setattr(b, "depth", None)) == -1
    assert status(lambda b: setattr(b, "scratch", None)) == -1
    assert status(lambda b: b.T_window.__setitem__(3, None)) == -1
    assert status(lambda b: b.visibility.__setitem__(2, None)) == -1
    assert status(lambda b: b.visibility_len.__setitem__(1, b.num_gaussians - 1)) == -1
    assert status(lambda b: setattr(b, "window_len", 17)) == -3
    assert status(lambda b: setattr(b, "window_len", 0)) == -1
    assert status(lambda b: setattr(b, "num_pixels", 0)) == -1
    torch.cuda.synchronize()
    assert bool((P._result == 0xAB).all())
    assert lib.mgs_keyframe_scratch_bytes(100, 100, 17) == 0
    assert lib.mgs_keyframe_scratch_bytes(100, 100, 16) > 0


class CheckedPolicy(KP.KeyframePolicy):
    """The native decision, checked at every frame against the torch mirror on the same inputs."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.checked = 0

    def _decide_native(self, cur_idx, cameras, window, tracker, occ, initialized):
        d = super()._decide_native(cur_idx, cameras, window, tracker, occ, initialized)
        m = self._decide_torch(cur_idx, cameras, window, tracker, occ, initialized)
        assert (d.create_kf, d.window, d.removed, d.reset) == (m.create_kf, m.window, m.removed, m.reset), (
            cur_idx, d, m)
        assert f32_bits(d.median_depth) == f32_bits(m.median_depth) or (
            math.isnan(d.median_depth) and math.isnan(m.median_depth))
        self.checked += 1
        return d


def test_run_sequence_with_the_policy_640x480(built):
    from monogs_amd import slam_surrogate as SS
    n = 21
    frames, cam, source = SS.load_sequence(n, 640, 480, DEV)
    P = CheckedPolicy(monocular=True)
    res = SS.run_sequence(frames, cam, DEV, init_iters=300, mapping_iters=60, keyframe_policy=P)
    torch.cuda.synchronize()
    assert P.checked == n - 1 and len(res["decisions"]) == n - 1 and len(res["windows"]) == n - 1
    kfs = res["kf_ids"]
    print(source, "keyframes", kfs, "resets", res["resets"], "windows", res["windows"][-1],
          [round(d.median_depth, 3) for d in res["decisions"]])
    assert res["capacity_ok"]
    assert all(b - a >= P.kf_interval for a, b in zip(kfs, kfs[1:]))
    for k, w in zip(range(1, n), res["windows"]):
        assert len(w) <= P.window_size and w[0] <= k and w[0] == max(w)
    for k, d in zip(range(1, n), res["decisions"]):
        if d.create_kf and not d.reset:
            assert res["windows"][k - 1][0] == k
    assert all(torch.isfinite(c.T).all() for c in res["cameras"].values())
    ev = SS.evaluate(res, frames, DEV, monocular=True)
    print(ev)
    assert ev["ate_rmse_m"] < 0.03 * ev["path_length_m"]


def test_run_sequence_resets_on_lost_overlap(built):
    """A fast rotation: the monocular map loses its overlap with the first keyframe before the window fills; the
    frame that triggered the reset re-initialises a fresh map at its ground-truth pose and the run goes on."""
    from monogs_amd import slam_surrogate as SS
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.slam_loops import GaussianParams, Pipe, ViewCamera
    from monogs_amd import synthetic as S
    n, W, H = 18, 320, 240
    cam = S.make_camera(W, H)
    poses = SS.trajectory(n, step=(0.01, 0.0, 0.0, 0.0, 0.05, 0.0))          # ~2.9 deg per frame
    world = SS.make_world(60_000, W, H, poses, seed=1)
    world = GaussianParams(*(t.to(DEV) for t in (world._xyz.data, world._scaling.data, world._rotation.data,
                                                 world._opacity.data, world._features_dc.data)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    frames = []
    with torch.no_grad():
        for k, T in enumerate(poses):
            v = ViewCamera(k, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, DEV)
            pkg = render(v, world, Pipe, torch.zeros(3, device=DEV))
            frames.append(SS.Frame(k, pkg["render"].clamp(0, 1).clone(), pkg["depth"][0].clone(), T))
    P = CheckedPolicy({"Training": {"kf_interval": 3}}, monocular=True)
    res = SS.run_sequence(frames, cam, DEV, init_iters=100, mapping_iters=20, keyframe_policy=P)
    torch.cuda.synchronize()
    print("resets", res["resets"], "windows", res["windows"])
    assert len(res["resets"]) >= 1 and P.checked == n - 1
    r = res["resets"][0]
    assert torch.equal(res["cameras"][r].T.cpu(), frames[r].T_gt.float())
    assert res["windows"][r - 1] == [r] and res["kf_ids"][0] == r
    assert all(torch.isfinite(c.T).all() for c in res["cameras"].values())
