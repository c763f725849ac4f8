"""Frame preparation without a GPU: the torch mirror (monogs_amd/frame_prepare.prepare_frame_torch) against what the
reference's own Camera.compute_grad_mask left behind (tests/golden/frame_prepare_ref.npz, written by
tests/golden/make_frame_prepare_golden.py), the uint8 / uint16 conversions exhaustively against NumPy, the C ABI's new
exports and struct mirror, and the argument errors.

The comparison rule (`compare`, shared with tests/test_gpu_frame_prepare.py).  The kernel, the mirror and the reference
round differently (the mean is a divide here and a multiply by 1/3 there, conv2d sums in its own order), so:
  * exact: rgb_pixel_mask_mapping; intensity == 0 wherever the fixture's is (the validity pattern); the zero fringe of
    patch mode; the converted image / depth;
  * intensities to 1e-5 relative + 1e-7 absolute, medians to 1e-5 relative: each carries about ten fp32 roundings;
  * a grad_mask / rgb_pixel_mask pixel may differ ONLY where the fixture's intensity is within 1e-5 relative of the
    fixture's threshold m * edge_threshold, and at most 0.1 % of the image may (the generator asserts that the
    reference's own band is inside that cap: a condition, not a measurement)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from monogs_amd import _cabi
from monogs_amd import frame_prepare as FP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_prepare_ref.npz")
BAND_REL, BAND_CAP = 1e-5, 1e-3
INT_REL, INT_ABS, MED_REL = 1e-5, 1e-7, 1e-5
PATCH = 32

_ref = None


def golden():
    global _ref
    if _ref is None:
        with np.load(GOLDEN) as z:
            _ref = {k: z[k] for k in z.files}
    return _ref


CASE_NAMES = ("global_48x80_float", "global_96x72_u8", "patch_70x100_float", "patch_70x100_u8",
              "patch_70x100_float_et1p1", "patch_64x96_u8_et1p1", "patch_64x96_float_depth", "rgbd_48x64_u8_u16")


def case(name):
    """One fixture case: the inputs as the entry points take them and what the reference left."""
    z = golden()
    get = lambda k: z.get(f"{name}_{k}")
    c = {k: get(k) for k in ("H", "W", "edge_threshold", "patch", "image", "image_u8", "depth_u16", "depth_scale",
                             "grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping", "gt_depth", "intensity", "median")}
    c["name"], c["H"], c["W"] = name, int(c["H"]), int(c["W"])
    c["dataset_type"] = "replica" if int(c["patch"]) else "tum"
    c["edge_threshold"] = float(c["edge_threshold"])
    c["rgb_boundary_threshold"] = float(z["rgb_boundary_threshold"])
    c["input_image"] = torch.from_numpy(c["image"] if c["image_u8"] is None else c["image_u8"])
    c["input_depth"] = c["depth_u16"]              # NumPy uint16, or None
    c["depth_scale"] = None if c["depth_scale"] is None else float(c["depth_scale"])
    return c


def fixture_threshold(c):
    """[H,W] the fixture's m * edge_threshold (fp32 product), +inf where no whole patch lies."""
    H, W = c["H"], c["W"]
    med = torch.from_numpy(np.atleast_1d(c["median"]))
    thr = torch.full((H, W), float("inf"))
    if c["dataset_type"] == "replica":
        ny, nx = H // PATCH, W // PATCH
        t = (med * c["edge_threshold"]).reshape(ny, nx)
        thr[:ny * PATCH, :nx * PATCH] = t.repeat_interleave(PATCH, 0).repeat_interleave(PATCH, 1)
    else:
        thr[:] = med[0] * c["edge_threshold"]
    return thr


def compare(got, c, what):
    """`got`: the dict prepare_frame_torch / FramePreparer.prepare return (any device), with `intensity`."""
    H, W = c["H"], c["W"]
    cpu = lambda t: t.detach().cpu()
    want_i = torch.from_numpy(c["intensity"])
    got_i = cpu(got["intensity"]).reshape(H, W)
    thr = fixture_threshold(c)
    # exact
    assert torch.equal(cpu(got["rgb_pixel_mask_mapping"]).reshape(H, W),
                       torch.from_numpy(c["rgb_pixel_mask_mapping"]).float()), f"{what}: rgb_pixel_mask_mapping"
    assert bool((got_i[want_i == 0] == 0).all()), f"{what}: the validity pattern"
    covered = torch.isfinite(thr)
    for k in ("grad_mask", "rgb_pixel_mask"):
        assert bool((cpu(got[k]).reshape(H, W)[~covered] == 0).all()), f"{what}: {k} outside the whole patches"
    if c["image_u8"] is not None:
        want_img = (c["image_u8"] / 255.0).astype(np.float32).transpose(2, 0, 1)
        assert np.array_equal(cpu(got["image"]).numpy().view(np.uint32), np.ascontiguousarray(want_img).view(np.uint32))
    if c["gt_depth"] is not None:
        assert tuple(got["gt_depth"].shape) == (1, H, W)
        assert np.array_equal(cpu(got["gt_depth"])[0].numpy().view(np.uint32), c["gt_depth"].view(np.uint32))
    else:
        assert got["gt_depth"] is None
    # to tolerance
    err = (got_i - want_i).abs()
    tol = INT_REL * want_i.abs() + INT_ABS
    med_got, med_want = cpu(got["median"]).reshape(-1).double(), torch.from_numpy(np.atleast_1d(c["median"])).double()
    assert med_got.shape == med_want.shape, f"{what}: median count"
    med_err = ((med_got - med_want).abs() / med_want.abs().clamp_min(1e-30)).max()
    # masks: a differing pixel only inside the band, and few of them
    band = covered & ((want_i - thr).abs() <= BAND_REL * thr)
    n_diff = 0
    for k in ("grad_mask", "rgb_pixel_mask"):
        g = cpu(got[k]).reshape(H, W)
        assert set(g.unique().tolist()) <= {0.0, 1.0} and g.dtype == torch.float32
        diff = g != torch.from_numpy(c[k]).float()
        n_diff = max(n_diff, int(diff.sum()))
        assert not bool((diff & ~band).any()), f"{what}: {k} differs outside the threshold band"
    print(f"{what} {c['name']}: intensity max err / tol {float((err / tol).max()):.3g}, median rel err "
          f"{float(med_err):.3g}, mask pixels differing {n_diff} (band holds {int(band.sum())})")
    assert bool((err <= tol).all()), f"{what}: intensity"
    assert float(med_err) <= MED_REL, f"{what}: median"
    assert n_diff <= BAND_CAP * H * W


def mirror(c, device="cpu"):
    img = c["input_image"].to(device)
    return FP.prepare_frame_torch(img, c["input_depth"], dataset_type=c["dataset_type"],
                                  edge_threshold=c["edge_threshold"],
                                  rgb_boundary_threshold=c["rgb_boundary_threshold"], depth_scale=c["depth_scale"])


def test_fixture_holds_the_cases_the_contract_names():
    z = golden()
    assert tuple(z["names"].tolist()) == CASE_NAMES
    assert os.path.getsize(GOLDEN) < 1 << 20
    for name in CASE_NAMES:
        c = case(name)
        cover = float(c["grad_mask"].mean())
        assert 0.05 <= cover <= 0.95
        assert int((c["intensity"] == 0).sum()) > 0            # a region of exact zeros / failed validity
        assert (c["rgb_pixel_mask"] == c["rgb_pixel_mask_mapping"] * c["grad_mask"]).all()
    fr = case("patch_70x100_float")
    assert not fr["grad_mask"][64:, :].any() and not fr["grad_mask"][:, 96:].any() and fr["median"].shape == (6,)
    assert case("patch_64x96_float_depth")["median"].shape == (6,)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_mirror_matches_the_reference(name):
    c = case(name)
    compare(mirror(c), c, "mirror")


def test_uint8_conversion_is_numpys_for_all_256_values():
    k = np.arange(256, dtype=np.uint8)
    want = (k / 255.0).astype(np.float32)
    got = FP.convert_image_torch(torch.from_numpy(np.stack([k, k, k], axis=-1).reshape(16, 16, 3)))
    assert got.shape == (3, 16, 16)
    for ch in range(3):
        assert np.array_equal(got[ch].reshape(-1).numpy().view(np.uint32), want.view(np.uint32))
    # a single-precision divide happens to agree too (the kernel still takes the double quotient)
    assert np.array_equal((k.astype(np.float32) / np.float32(255.0)).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("depth_scale", [5000.0, 6553.5])
def test_uint16_conversion_is_numpys_for_all_65536_values(depth_scale):
    d = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    want = (d / depth_scale).astype(np.float32)
    got = FP.convert_depth_torch(FP._as_tensor(d), depth_scale).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    single = d.astype(np.float32) / np.float32(depth_scale)
    print(f"depth_scale {depth_scale}: a single-precision divide differs from NumPy's value at "
          f"{int((single.view(np.uint32) != want.view(np.uint32)).sum())} of 65536 inputs")
    out = FP.prepare_frame_torch(torch.full((3, 256, 256), 0.5), d, dataset_type="tum", edge_threshold=1.1,
                                 depth_scale=depth_scale)
    assert np.array_equal(out["gt_depth"][0].numpy().view(np.uint32), want.view(np.uint32))


def test_cabi_exports_and_struct_mirror(built):
    L = _cabi.lib()
    assert {"mgs_frame_prepare_scratch_bytes", "mgs_frame_prepare"} <= set(_cabi.EXPORTS)
    assert "mgs_frame_prepare_args_size" in _cabi.EXPORTS
    assert L.mgs_frame_prepare_args_size() == C.sizeof(_cabi.FramePrepareArgs) == 8 * 4 + 8 + 10 * 8
    assert L.mgs_abi_version() == _cabi.ABI_VERSION
    assert L.mgs_frame_prepare_scratch_bytes(480, 640) >= 480 * 640 * 4 + (2048 + 2048 + 1024) * 4
    assert L.mgs_frame_prepare_scratch_bytes(1, 640) == 0 and L.mgs_frame_prepare_scratch_bytes(480, 0) == 0


def _args(H, W, mode):
    """Non-null addresses that are never dereferenced: every check below fails before anything is launched."""
    a = _cabi.FramePrepareArgs()
    a.width, a.height, a.mode = W, H, mode
    a.edge_threshold, a.rgb_boundary_threshold = 1.1, 0.01
    for f in ("image_in", "grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping", "scratch"):
        setattr(a, f, 4096)
    return a


def test_argument_errors(built):
    L = _cabi.lib()
    call = lambda a: L.mgs_frame_prepare(C.byref(a), None)
    assert L.mgs_frame_prepare(None, None) == -1
    for H, W in ((31, 64), (64, 31), (16, 16)):                       # no whole patch: the reference's unfold raises
        assert call(_args(H, W, _cabi.FRAME_MODE_PATCH)) == -1
        with pytest.raises(ValueError, match="patch"):
            FP.prepare_frame_torch(torch.rand(3, H, W), dataset_type="replica", edge_threshold=4)
    assert call(_args(1, 64, _cabi.FRAME_MODE_GLOBAL)) == -1          # no reflect padding of a single row
    with pytest.raises(ValueError):
        FP.prepare_frame_torch(torch.rand(3, 1, 64), dataset_type="tum", edge_threshold=1.1)
    assert call(_args(48, 64, 2)) == -1                               # unknown mode
    a = _args(48, 64, 0)
    a.image_format = 7
    assert call(a) == -1
    a = _args(48, 64, 0)
    a.image_format = _cabi.FRAME_IMAGE_U8_HWC                         # uint8 input without a float image to write
    assert call(a) == -1
    a = _args(48, 64, 0)
    a.depth_format = _cabi.FRAME_DEPTH_U16                            # depth announced, none given
    assert call(a) == -1
    a.depth_in, a.gt_depth, a.depth_scale = 4096, 4096, 0.0           # ... and a scale that is not positive
    assert call(a) == -1
    a = _args(48, 64, 0)
    a.scratch = 4100                                                  # not 16-byte aligned
    assert call(a) == -1
    a = _args(48, 64, 0)
    a.grad_mask = None
    assert call(a) == -1
    with pytest.raises(ValueError, match="depth_scale"):
        FP.prepare_frame_torch(torch.rand(3, 48, 64), np.zeros((48, 64), np.uint16), dataset_type="tum",
                               edge_threshold=1.1)


def test_preparer_has_no_cpu_fallback(built):
    with pytest.raises(RuntimeError, match="GPU only"):
        FP.FramePreparer(48, 64, "cpu")
