"""The keyframe seeding path on a machine without a GPU: the torch mirror (monogs_amd/keyframe_seed.py) against what the
reference's own FrontEnd.add_new_keyframe / get_median_depth / np.median returned (tests/golden/keyframe_seed_ref.npz,
written by tests/golden/make_keyframe_seed_golden.py), the sub-sample rule, the back-projection against the existing
create_pcd_from_image_and_depth arithmetic with the selection injected, and the C ABI of mgs_keyframe_seed.

Distances observed on the fixture (printed by test_depth_prior_reproduces_the_reference): the mirror's std (fp64 sums,
rounded once) sits 2e-8 .. 6e-8 from the fp64 value, exactly where the reference's fp32 std sits; no pixel of any case
lies in the band where the outlier test could flip."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from monogs_amd import _cabi
from monogs_amd import keyframe_seed as KS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_seed_ref.npz")
EPS = float(np.finfo(np.float32).eps)
BAND_CAP = 1e-3          # at most 0.1 % of a case's pixels may sit on the outlier threshold


def load_cases():
    z = np.load(GOLDEN)
    return z, [str(n) for n in z["names"]]


def case_inputs(z, name, dev="cpu"):
    """The fp32 inputs of a fixture case (stored as integers: image and opacity in 1/255 steps, depth in mm)."""
    g = lambda k: z[f"{name}_{k}"] if f"{name}_{k}" in z.files else None
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth = None if g("depth_mm") is None else g("depth_mm").astype(np.float32) * np.float32(0.001)
    opacity = None if g("opacity_u8") is None else g("opacity_u8").astype(np.float32) / np.float32(255.0)
    return dict(H=int(g("H")), W=int(g("W")), mode=int(g("mode")),
                image=t(g("image_u8").astype(np.float32) / np.float32(255.0)), depth=t(depth), opacity=t(opacity),
                noise=t(g("noise")), thr=float(z["rgb_boundary_threshold"]))


def threshold_band(depth, med, std_ref, std_got):
    """Pixels whose outlier test may flip between two values of std: |d - (med +- std_ref)| <= |std_got - std_ref|."""
    d = depth.double().cpu()
    band = abs(float(std_got) - float(std_ref))
    return ((d - (float(med) + float(std_ref))).abs() <= band) | ((d - (float(med) - float(std_ref))).abs() <= band)


def make_cam(H, W, dev="cpu", seed=5):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(3, generator=g, dtype=torch.float64) * 0.2
    th = w.norm()
    Kx = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + torch.sin(th) / th * Kx + (1 - torch.cos(th)) / th ** 2 * Kx @ Kx
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = R
    T[:3, 3] = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64)
    return types.SimpleNamespace(fx=0.82 * W, fy=0.83 * W, cx=0.5 * W - 0.3, cy=0.5 * H + 0.2, T=T.float().to(dev),
                                 exposure_a=torch.tensor([0.93], device=dev), exposure_b=torch.tensor([0.021], device=dev),
                                 exposure_eps=1e-8, image_height=H, image_width=W)


def test_fixture_covers_the_required_cases():
    z, names = load_cases()
    modes = [int(z[f"{n}_mode"]) for n in names]
    assert {0, 1, 2} <= set(modes)
    sizes = [(int(z[f"{n}_H"]), int(z[f"{n}_W"])) for n, m in zip(names, modes) if m == 0]
    assert (120, 160) in sizes and any(h % 16 and w % 16 for h, w in sizes)
    thr = float(z["rgb_boundary_threshold"])
    dark = [n for n in names if (case_inputs(z, n)["image"].sum(dim=0) <= thr).any()]
    assert any(int(z[f"{n}_mode"]) == 0 for n in dark)                                      # valid_rgb bites
    assert any(int(z[f"{n}_mode"]) == 0 and (z[f"{n}_depth_mm"] == 0).any() and (z[f"{n}_opacity_u8"] < 243).any()
               for n in names)                                                              # holes, low opacity
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", load_cases()[1])
def test_depth_prior_reproduces_the_reference(name):
    z, _ = load_cases()
    c = case_inputs(z, name)
    d, info = KS.depth_prior_torch(c["image"], c["depth"], c["opacity"], c["mode"], c["noise"], c["thr"])
    want = torch.from_numpy(z[f"{name}_initial_depth"])
    if c["mode"] != 0:
        assert torch.equal(d, want)
        return
    med_ref, std_ref, std64 = z[f"{name}_median_depth"], z[f"{name}_std"], float(z[f"{name}_std_fp64"])
    assert np.float32(info["median_depth"].item()).view(np.uint32) == np.float32(med_ref).view(np.uint32)
    valid_ref = np.unpackbits(z[f"{name}_valid_mask"])[:c["H"] * c["W"]].astype(bool).reshape(c["H"], c["W"])
    assert np.array_equal(info["valid_mask"].numpy(), valid_ref)
    assert info["n_valid"] == int(valid_ref.sum())
    std = float(info["std_depth"])
    # both are evaluations of one formula on the same data: the mirror may be as far from the fp64 value as the
    # reference's fp32 reduction is, times four (the tree shape)
    dist_ref, dist = abs(float(std_ref) - std64), abs(std - std64)
    out = threshold_band(c["depth"], med_ref, std_ref, std)
    print(f"{name}: std mirror {std:.9g} reference {float(std_ref):.9g} fp64 {std64:.12g}: |mirror - fp64| {dist:.3g}, "
          f"|reference - fp64| {dist_ref:.3g}; {int(out.sum())} of {out.numel()} pixels in the threshold band")
    assert dist <= 4 * dist_ref
    assert int(out.sum()) <= BAND_CAP * out.numel()
    assert torch.equal(d[~out], want[~out])


@pytest.mark.parametrize("name", load_cases()[1])
def test_median_all_is_numpys_median(name):
    z, _ = load_cases()
    d = torch.from_numpy(z[f"{name}_initial_depth"])
    got = KS.median_all_torch(d)
    assert got.dtype == torch.float32
    assert np.float32(got.item()).view(np.uint32) == np.float32(z[f"{name}_median_all"]).view(np.uint32)


def test_median_all_where_the_two_middle_values_differ():
    z, names = load_cases()
    seen = 0
    for name in names:
        s = np.sort(z[f"{name}_initial_depth"].reshape(-1))
        n = s.size
        if n % 2 == 0 and s[n // 2 - 1] != s[n // 2]:
            seen += 1
            got = KS.median_all_torch(torch.from_numpy(z[f"{name}_initial_depth"]))
            assert s[n // 2 - 1] < got.item() < s[n // 2] or got.item() in (s[n // 2 - 1], s[n // 2])
            assert np.float32(got.item()) == np.float32(z[f"{name}_median_all"])
            assert np.float32(got.item()) != torch.from_numpy(s).median().numpy()      # not torch's lower median
    assert seen >= 1
    x = torch.tensor([[0.0, 4.0], [1.0, 2.0]])
    assert KS.median_all_torch(x).item() == 1.5 == float(np.median(x.numpy()))
    assert KS.median_all_torch(torch.tensor([3.0, 1.0, 2.0])).item() == 2.0


@pytest.mark.parametrize("downsample", [64, 32, 7.5])
def test_selection_is_the_k_smallest_key_index_pairs(downsample):
    g = torch.Generator().manual_seed(11)
    H, W = 53, 75
    d = 0.5 + 3 * torch.rand(H, W, generator=g)
    d[torch.rand(H, W, generator=g) < 0.2] = 0.0
    d[3, 4] = 150.0                                           # beyond depth_trunc
    keys = torch.randint(0, 2 ** 32, (H * W,), generator=g, dtype=torch.int64)
    keys[torch.rand(H * W, generator=g) < 0.5] = int(keys[17])          # many ties, around the threshold too
    sel, n = KS.select_torch(d, keys, downsample)
    flat = d.reshape(-1).numpy()
    idx = np.nonzero((flat > 0) & (flat <= 100.0))[0]
    K = int(len(idx) / downsample)
    order = np.lexsort((idx, keys.numpy()[idx]))              # by key, then by pixel index
    want = np.sort(idx[order[:K]])
    assert n == len(idx) and sel.numel() == K
    assert np.array_equal(sel.numpy(), want)


@pytest.mark.parametrize("name", ["mono_160x120", "mono_off_grid", "mono_dark_border"])
def test_backprojection_agrees_with_the_existing_torch_path(name, monkeypatch):
    """create_pcd_from_image_and_depth with the selection injected (its randperm replaced by the order that yields the
    mirror's pixels) and the k-nn stubbed: xyz, colours and features_dc to 16 eps max(1, |value|) - at most eight
    roundings per coordinate, a factor two for contraction differences."""
    from monogs_amd import keyframe_init as KI
    z, _ = load_cases()
    c = case_inputs(z, name)
    H, W = c["H"], c["W"]
    cam = make_cam(H, W)
    d = torch.from_numpy(z[f"{name}_initial_depth"])
    g = torch.Generator().manual_seed(3)
    keys = torch.randint(0, 2 ** 32, (H * W,), generator=g, dtype=torch.int64)
    out = KS.seed_torch(cam, c["image"], d, None, KS.MODE_SENSOR, downsample=16, rgb_boundary_threshold=-1.0,
                        keys=keys, dist2_fn=lambda p: torch.ones(p.shape[0]))
    sel = out["sel"]
    assert torch.equal(out["depth"], d) and sel.numel() == int(out["n_depth"] / 16) > 100
    idx = torch.nonzero(((d > 0) & (d <= 100.0)).reshape(-1)).reshape(-1)
    pos = torch.searchsorted(idx, sel)
    rest = torch.ones(idx.numel(), dtype=torch.bool)
    rest[pos] = False
    perm = torch.cat([pos, torch.nonzero(rest).reshape(-1)])
    monkeypatch.setattr(KI.torch, "randperm", lambda n, **k: perm)
    monkeypatch.setattr(KI, "distCUDA2", lambda p: torch.ones(p.shape[0]))
    xyz, feats, scales, rots, opac = KI.create_pcd_from_image_and_depth(cam, c["image"], d, downsample_factor=16,
                                                                         adaptive_pointsize=False)
    monkeypatch.undo()

    def close(a, b):
        return bool(((a - b).abs() <= 16 * EPS * torch.clamp_min(b.abs(), 1.0)).all())

    assert close(out["xyz"], xyz)
    assert close(out["features_dc"], feats[:, :, 0])
    assert close(out["colour"], feats[:, :, 0] * 0.28209479177387814 + 0.5)
    assert torch.equal(out["rots"], rots) and torch.equal(out["opacity_logit"], opac)
    assert out["log_scales"].shape == scales.shape


def test_struct_mirror_and_exports(built):
    L = _cabi.lib()
    assert L.mgs_struct_size(25) == C.sizeof(_cabi.KeyframeSeedArgs)
    assert L.mgs_struct_size(26) == -1
    assert _cabi.struct_mirrors()[25] is _cabi.KeyframeSeedArgs
    assert C.sizeof(_cabi.KeyframeSeedResult) == 32
    assert {"mgs_keyframe_seed_scratch_bytes", "mgs_keyframe_seed"} <= set(_cabi.EXPORTS)
    assert L.mgs_abi_version() == 10
    assert L.mgs_keyframe_seed_scratch_bytes(0, 10) == 0 and L.mgs_keyframe_seed_scratch_bytes(10, 0) == 0
    assert L.mgs_keyframe_seed_scratch_bytes(640 * 480, 9600) >= L.mgs_knn_scratch_bytes(9600) + 2 * 4 * 640 * 480


def test_bad_arguments_are_refused_without_a_gpu(built):
    """Validation happens before the first HIP call: these return on a machine without a device."""
    L = _cabi.lib()
    assert L.mgs_keyframe_seed(None, None) == -1
    rec = _cabi.KeyframeSeedResult()
    a = _cabi.KeyframeSeedArgs()
    a.width, a.height, a.mode, a.downsample = 64, 48, 1, 32.0
    for f in ("image", "T", "exposure_a", "exposure_b", "xyz", "features_dc", "log_scales", "rots", "opacity_logit",
              "scratch", "result"):
        setattr(a, f, 4096)                      # never dereferenced: every case below is refused first
    a.result_host = C.pointer(rec)
    a.row_capacity = 64 * 48 // 32 - 1           # one row short of floor(H*W / downsample)
    assert L.mgs_keyframe_seed(C.byref(a), None) == -1
    a.row_capacity = 64 * 48 // 32
    for field, bad in (("downsample", 0.0), ("downsample", -2.0), ("downsample", 0.5), ("scratch", 4104), ("width", 0), ("mode", 3), ("xyz", None),
                       ("result_host", None)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert L.mgs_keyframe_seed(C.byref(a), None) == -1, field
        setattr(a, field, keep)
    a.mode = 0                                   # rendered depth without depth / opacity
    assert L.mgs_keyframe_seed(C.byref(a), None) == -1
    assert rec.num_points == 0
