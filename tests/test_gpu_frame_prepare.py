"""mgs_frame_prepare (frame_prepare.hip) on the MI355X: against what the reference left behind
(tests/golden/frame_prepare_ref.npz), against the torch mirror at the kernels' own trip boundaries (DESIGN.md "Frame
preparation on the device" names them), determinism, a reused scratch, a side stream, the input formats, and the two
opt-in consumers (NativeTracker(mask=...), run_sequence(native_frame_prepare=True)).  The comparison rule is
test_cpu_frame_prepare.compare's."""
import numpy as np
import pytest
import torch

from monogs_amd import frame_prepare as FP
from test_cpu_frame_prepare import BAND_CAP, BAND_REL, CASE_NAMES, case, compare, fixture_threshold

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping", "median", "intensity")


def config(dataset_type, edge_threshold, rgb_boundary_threshold=0.01):
    return {"Training": {"edge_threshold": edge_threshold, "rgb_boundary_threshold": rgb_boundary_threshold},
            "Dataset": {"type": dataset_type}}


def make_image(H, W, seed, quantised=False):
    """Noise over a slow ramp with a corner of exact zeros and a strip too dark for the validity test: float [3,H,W]
    on the CPU, or uint8 [H,W,3]."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H)[:, None]
    img = (0.15 + 0.3 * y + 0.5 * torch.rand(3, H, W, generator=g)).clamp(0.05, 0.95)
    if H >= 16 and W >= 16:             # (a 2x2 image keeps all its pixels valid: a median of 0 has no band to speak of)
        img[:, :H // 4, :W // 5] = 0.0
        img[:, H // 2:H // 2 + 2, W // 3:W // 3 + 5] = 1.0 / 255.0
    if quantised:
        return img.mul(255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    return img


def snapshot(res):
    return {k: res[k].clone() for k in KEYS if res.get(k) is not None}


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in KEYS)


def as_case(m, H, W, dataset_type, edge_threshold, name):
    """A mirror result in the shape of a fixture case, for `compare`."""
    u8 = lambda k: m[k].reshape(H, W).cpu().numpy().astype(np.uint8)
    c = {"name": name, "H": H, "W": W, "dataset_type": dataset_type, "edge_threshold": float(edge_threshold),
         "intensity": m["intensity"].cpu().numpy(), "median": m["median"].cpu().numpy(), "image_u8": None,
         "gt_depth": None, "grad_mask": u8("grad_mask"), "rgb_pixel_mask": u8("rgb_pixel_mask"),
         "rgb_pixel_mask_mapping": u8("rgb_pixel_mask_mapping")}
    want_i, thr = torch.from_numpy(c["intensity"]), fixture_threshold(c)
    band = torch.isfinite(thr) & (thr > 0) & ((want_i - thr).abs() <= BAND_REL * thr)       # (0 against 0 cannot flip)
    assert int(band.sum()) <= BAND_CAP * H * W, "the test image itself puts too many pixels on the threshold"
    return c


@pytest.mark.parametrize("name", CASE_NAMES)
def test_native_matches_the_reference(built, name):
    c = case(name)
    P = FP.FramePreparer(c["H"], c["W"], DEV, config(c["dataset_type"], c["edge_threshold"],
                                                     c["rgb_boundary_threshold"]), keep_intensity=True)
    got = P.prepare(c["input_image"], c["input_depth"], c["depth_scale"])
    torch.cuda.synchronize()
    compare(got, c, "native")


# global mode: a 64x16 tile per workgroup of k_fp_intensity; 1024 pixels per workgroup and trip of the 1-D passes,
# 256 workgroups at the most.  patch mode: a 32x32 tile per workgroup.
BOUNDARY_SHAPES = [
    ("tum", 2, 2),             # the smallest image reflect padding allows: every neighbour is a reflected one
    ("tum", 16, 64),           # exactly one tile
    ("tum", 17, 65),           # one more row and column than a tile: 2 x 2 tiles, a second 1-D workgroup (1105 px)
    ("tum", 33, 31),           # narrower than a tile row, odd sizes
    ("tum", 48, 67),           # a width that is no multiple of the 64 lanes a tile row takes
    ("tum", 5, 52429),         # 256 * 1024 + 1 pixels: the 1-D passes take a second trip
    ("replica", 33, 35),       # one patch, a fringe of 1 row and 3 columns
    ("replica", 65, 97),       # 2 x 3 patches, a fringe of 1 row and 1 column
    ("replica", 32, 32),       # exactly one patch, no fringe
]


@pytest.mark.parametrize("dataset_type,H,W", BOUNDARY_SHAPES)
def test_native_matches_the_mirror_at_the_trip_boundaries(built, dataset_type, H, W):
    et = 1.1
    P = FP.FramePreparer(H, W, DEV, config(dataset_type, et), keep_intensity=True)
    for quantised in (False, True):
        img = make_image(H, W, seed=H * 1000 + W, quantised=quantised).to(DEV)
        m = FP.prepare_frame_torch(img, dataset_type=dataset_type, edge_threshold=et)
        got = P.prepare(img)
        torch.cuda.synchronize()
        c = as_case(m, H, W, dataset_type, et, f"{dataset_type} {H}x{W} {'uint8' if quantised else 'float'}")
        compare(got, c, "native vs mirror")
        if quantised:
            assert torch.equal(got["image"], m["image"])


@pytest.mark.parametrize("dataset_type", ["tum", "replica"])
def test_calls_are_bit_reproducible_and_leave_the_scratch_clean(built, dataset_type):
    H, W, et = 120, 160, 1.1
    P = FP.FramePreparer(H, W, DEV, config(dataset_type, et), keep_intensity=True)
    a_img, b_img = make_image(H, W, 1).to(DEV), make_image(H, W, 2).to(DEV)
    a1 = snapshot(P.prepare(a_img))
    a2 = snapshot(P.prepare(a_img))
    assert same_bits(a1, a2)
    # another image through the same object: nothing of the first call's counting may be left behind
    b = P.prepare(b_img)
    torch.cuda.synchronize()
    m = FP.prepare_frame_torch(b_img, dataset_type=dataset_type, edge_threshold=et)
    compare(b, as_case(m, H, W, dataset_type, et, f"{dataset_type} second image"), "native vs mirror")
    assert not torch.equal(b["grad_mask"], a1["grad_mask"])
    b1 = snapshot(b)
    assert same_bits(snapshot(P.prepare(a_img)), a1)
    assert same_bits(snapshot(FP.FramePreparer(H, W, DEV, config(dataset_type, et), keep_intensity=True).prepare(b_img)),
                     b1)


def test_a_side_stream(built):
    H, W = 96, 130
    img = make_image(H, W, 3).to(DEV)
    P = FP.FramePreparer(H, W, DEV, config("tum", 1.1), keep_intensity=True)
    want = snapshot(P.prepare(img))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    Q = FP.FramePreparer(H, W, DEV, config("tum", 1.1), keep_intensity=True)
    with torch.cuda.stream(side):
        got = Q.prepare(img)
    side.synchronize()
    assert same_bits(snapshot(got), want)


@pytest.mark.parametrize("dataset_type", ["tum", "replica"])
def test_float_and_uint8_input_of_one_frame_agree(built, dataset_type):
    H, W = 70, 100
    u8 = make_image(H, W, 4, quantised=True)
    as_float = FP.convert_image_torch(u8)
    P = FP.FramePreparer(H, W, DEV, config(dataset_type, 1.1), keep_intensity=True)
    from_u8 = P.prepare(u8)
    image = from_u8["image"].clone()
    a = snapshot(from_u8)
    from_float = P.prepare(as_float)
    assert from_float["image"].data_ptr() != P.buffers["image"].data_ptr()      # handed back, not copied
    assert same_bits(snapshot(from_float), a)
    assert torch.equal(image.cpu(), as_float)


@pytest.mark.parametrize("depth_scale", [5000.0, 6553.5])
def test_device_conversions_are_numpys_for_every_value(built, depth_scale):
    H = W = 256
    d = np.arange(65536, dtype=np.uint16).reshape(H, W)
    k = (np.arange(H * W * 3) % 256).astype(np.uint8).reshape(H, W, 3)
    got = FP.FramePreparer(H, W, DEV, config("tum", 1.1)).prepare(k, d, depth_scale)
    want_d = (d / depth_scale).astype(np.float32)
    want_i = np.ascontiguousarray((k / 255.0).astype(np.float32).transpose(2, 0, 1))
    assert np.array_equal(got["gt_depth"][0].cpu().numpy().view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(got["image"].cpu().numpy().view(np.uint32), want_i.view(np.uint32))
    # a float depth is handed through
    f = FP.FramePreparer(H, W, DEV, config("tum", 1.1)).prepare(k, torch.from_numpy(want_d))
    assert torch.equal(f["gt_depth"][0].cpu(), torch.from_numpy(want_d))


def test_tracker_takes_an_explicit_mask(built):
    """NativeTracker(mask=rgb_pixel_mask) for one first-order iteration equals NativeTracker on a viewpoint whose
    rgb_pixel_mask_mapping attribute was set to that mask."""
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import Pipe
    from monogs_amd.tracking_native import NativeTracker
    from test_raster_gpu import _loop_fixture
    H, W = 48, 64
    sc, gauss, view, dev = _loop_fixture(N=1500, W=W, H=H)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(view(1, torch.eye(4)), gauss, Pipe, bg)["render"].clamp(0, 1).clone()
    P = FP.FramePreparer(H, W, dev, config("tum", 1.1))
    T0 = SE3_exp(torch.tensor((0.02, -0.015, 0.01, 0.004, -0.006, 0.003)))
    va, vb = view(2, T0), view(3, T0)
    ra = P.prepare_into(va, target)
    P.prepare_into(vb, target)
    edge = ra["rgb_pixel_mask"]
    assert 0 < float(edge.sum()) < float(ra["rgb_pixel_mask_mapping"].sum())
    vb.rgb_pixel_mask_mapping = edge.clone()
    a = NativeTracker(va, gauss, bg, mask=edge)
    b = NativeTracker(vb, gauss, bg)
    for t in (a, b):
        t.step()
    torch.cuda.synchronize()
    assert torch.equal(va.T, vb.T) and torch.equal(a.loss, b.loss)
    assert torch.equal(va.exposure_a, vb.exposure_a) and torch.equal(va.exposure_b, vb.exposure_b)
    assert not torch.equal(va.T, T0.to(dev))
    with pytest.raises(ValueError, match="mask"):
        NativeTracker(view(5, T0), gauss, bg, mask=edge[:, :10])


def test_run_sequence_prepares_every_frame(built):
    from monogs_amd import slam_surrogate as SS
    H, W, n = 48, 64, 3
    frames, cam, _ = SS.load_sequence(n, W, H, DEV, world_gaussians=3000)
    cfg = {"Training": {"edge_threshold": 1.1, "rgb_boundary_threshold": 0.01}, "Dataset": {"type": "tum",
           "pcd_downsample": 4, "pcd_downsample_init": 2}}
    kw = dict(init_iters=20, mapping_iters=5, kf_interval=1, first_order_iters=4, second_order_iters=0, config=cfg)
    res = SS.run_sequence(frames, cam, DEV, native_frame_prepare=True, **kw)
    torch.cuda.synchronize()
    assert sorted(res["cameras"]) == list(range(n)) and res["t_prepare"] > 0
    P = FP.FramePreparer(H, W, DEV, cfg)
    for k, vp in res["cameras"].items():
        want = snapshot({**P.prepare(frames[k].image), "intensity": None})
        for key in ("grad_mask", "rgb_pixel_mask", "rgb_pixel_mask_mapping"):
            assert torch.equal(getattr(vp, key), want[key]), (k, key)
        assert vp.original_image.data_ptr() == frames[k].image.data_ptr()
    masks = [res["cameras"][k].grad_mask for k in range(n)]
    assert masks[0].data_ptr() != masks[1].data_ptr()            # every camera owns its masks
    edges = SS.run_sequence(frames, cam, DEV, native_frame_prepare=True, track_on_edges=True, **kw)
    assert edges["frames_tracked"] == n - 1
    with pytest.raises(ValueError, match="native_frame_prepare"):
        SS.run_sequence(frames, cam, DEV, track_on_edges=True, **kw)
