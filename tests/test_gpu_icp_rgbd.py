"""GPU tests of the RGB-D alignment (csrc/icp.hip: k_icp_intensity, k_icp_rows_rgbd, mgs_icp_align_rgbd): the device against
the NumPy mirror bit for bit - intensity planes, sums, all counters, step, pivots, D, T_w2c, record and history - on partial
tiles, more than one trip, both normal and both colour layouts, other model intrinsics, hostile input around guarded planes;
two runs byte-equal; the textured plane through vol.track on both volumes, degenerate without and converged with the colour;
photo_weight = 0 against the bytes of mgs_icp_align; and run_sequence(icp_init=True, icp_kw=dict(photo_weight=...)).
The model planes are the device's own ray cast of volumes fused from coloured views on the device (icp_rgbd_cases.py)."""
import functools

import numpy as np
import pytest
import torch

import icp_cases as IC
import icp_rgbd_cases as RC

pytestmark = pytest.mark.gpu

GUARD = 256
EYE = np.eye(4, dtype=np.float32)
LAM = RC.PHOTO_WEIGHT


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def scrub(*tensors):
    """Zero device tensors that held NaN, inf or 1e30 before they go back to the caching allocator: a later test that
    allocates with torch.empty must not find them."""
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            t.zero_()
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def leave_the_device_memory_clean():
    """After this module: drop its volumes and planes, hand the cached blocks back and zero-fill as many bytes as were
    reserved, so that the tests after it start from memory without this module's values."""
    yield
    volume.cache_clear()
    model.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        reserved = torch.cuda.memory_reserved()
        torch.cuda.empty_cache()
        sweep = torch.zeros(max(reserved // 4, 1), device=_dev())
        torch.cuda.synchronize()
        del sweep
        torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def volume(kind, scene):
    """A dense or a sparse volume fused from the three coloured views of `scene`."""
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    from monogs_amd.tsdf import TSDFVolume
    dev = _dev()
    vol = TSDFVolume(IC.ORIGIN, IC.VS, IC.DIMS, device=dev) if kind == "dense" else SparseTSDFVolume(IC.ORIGIN, IC.VS, IC.MAX_BRICKS, device=dev)
    assert not vol.has_color
    for T, depth, image, intr in RC.fusion_views(scene):
        vol.integrate(depth.to(dev), torch.from_numpy(T).float().to(dev), *intr, image=image.to(dev))
    torch.cuda.synchronize()
    assert vol.has_color
    return vol


@functools.lru_cache(maxsize=None)
def model(kind, scene, h=IC.H, w=IC.W, intr=IC.INTR):
    """(the ray cast at T = I on the device, the same planes on the host)."""
    planes = volume(kind, scene).raycast(torch.eye(4, device=_dev()), *intr, h, w, z_far=IC.Z_FAR)
    torch.cuda.synchronize()
    return planes, {k: v.cpu() for k, v in planes.items()}


def run(model_, depth, image, **kw):
    from monogs_amd import icp
    kw.setdefault("read", False)
    kw.setdefault("photo_weight", LAM)
    view = kw.pop("view", IC.INTR)
    T_model = kw.pop("T_model", EYE)
    out = icp.align(model_, depth.to(_dev()), view, T_model, image=None if image is None else image.to(_dev()), **kw)
    torch.cuda.synchronize()
    return out


def same_bytes(a, b, keys=("record", "history", "D", "T_w2c")):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in keys)


# ---- 1. the intensity planes ------------------------------------------------------------------------------------------
def test_intensity_planes_bit_for_bit(built):
    from monogs_amd import icp
    dev = _dev()
    _, host = model("dense", "wavy")
    for rgb, valid in ((host["color"], host["depth"]), (RC.wavy_image(), None), (RC.wavy_image(), host["depth"] > 0)):
        rgb = rgb.clone()
        flat = rgb.view(-1)
        flat[100], flat[2000], flat[3500], flat[4100], flat[5000] = float("nan"), float("inf"), 1e30, -1e30, 1.0 + 2.0 ** -23
        g_rgb, buf = guarded(rgb.to(dev), 0.5)
        got = icp.intensity_planes(g_rgb, None if valid is None else valid.to(dev))
        want = icp.intensity_planes_torch(rgb, valid)
        torch.cuda.synchronize()
        bad = int((want[0] == icp.NO_INTENSITY).sum())
        print(tuple(rgb.shape), "invalid", bad, "no gx", int((want[1] == icp.NO_GRADIENT).sum()))
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.numpy().view(np.int32)) and bad >= 5
        assert bool((buf[:GUARD] == 0.5).all()) and bool((buf[-GUARD:] == 0.5).all())
        scrub(buf)
    with pytest.raises(RuntimeError, match="GPU only"):
        icp.intensity_planes(RC.wavy_image())


# ---- 2. one iteration on partial tiles --------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_one_iteration_equals_rows_and_solve(built, kind, stride):
    from monogs_amd import icp
    from monogs_amd.surface import depth_normal_torch
    dev_planes, host = model(kind, "wavy")
    got = run(dev_planes, IC.frame_depth(), RC.wavy_image(), levels=((stride, 1),))
    D0 = icp.initial_transform(EYE)
    photo = {"sensor": icp.intensity_planes_torch(RC.wavy_image()), "model": icp.intensity_planes_torch(host["color"], valid=host["depth"]),
             "weight": LAM}
    sn = depth_normal_torch(IC.frame_depth(), *IC.INTR, pixel_center=0.0)
    sums, counts, extra = icp.icp_rows_numpy(host, IC.frame_depth(), sn, D0, IC.INTR, stride=stride, photo=photo)
    s = icp.icp_solve_numpy(sums, counts[0] + extra[0], D0, last=True)
    rec = got["record"].cpu().numpy()
    info = icp.read_record(rec, rgbd=True)
    print(stride, info["status_name"], info["counts"], info["photo"], info["sum_ri2"], info["x"])
    assert np.array_equal(rec[:28], sums) and np.array_equal(rec[28:35], counts) and np.array_equal(rec[52:56], extra)
    assert int(counts.sum()) == -(-IC.H // stride) * -(-IC.W // stride) and counts[0] > 100 and extra[0] > 100
    assert int(extra[:3].sum()) == int(counts[0] + counts[4:].sum())
    assert np.array_equal(info["x"].view(np.int64), s["x"].view(np.int64))
    assert np.array_equal(info["pivots"].view(np.int64), s["pivots"].view(np.int64))
    assert info["status"] == s["status"] == icp.MAX_ITERATIONS and info["iterations_run"] == 1
    assert np.array_equal(got["D"].cpu().numpy().view(np.int64), s["D"].view(np.int64))
    assert np.array_equal(got["T_w2c"].cpu().numpy().view(np.int32), icp.pose_of(s["D"], EYE).view(np.int32))
    assert np.array_equal(got["history"].cpu().numpy()[0], [counts[0], sums[27], icp._f64_bits(s["xx"]), s["status"], 1, 0, 0, extra[3]])
    for name, want in (("intensity", photo["sensor"]), ("model_intensity", photo["model"])):
        assert np.array_equal(got[name].cpu().numpy().view(np.int32), want.numpy().view(np.int32)), name
    # the geometric row and its seven counters are mgs_icp_align's
    geo = run(dev_planes, IC.frame_depth(), None, levels=((stride, 1),), photo_weight=0.0)
    assert np.array_equal(geo["record"].cpu().numpy()[28:35], counts) and not geo["record"].cpu().numpy()[52:].any()


# ---- 3. schedules, determinism ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [None, ((3, 2), (1, 3))])
def test_schedules_equal_the_mirror_and_two_runs_are_byte_equal(built, levels):
    from monogs_amd import icp
    levels = icp.LEVELS if levels is None else levels
    dev_planes, host = model("dense", "wavy")
    want = icp.align_numpy(host, IC.frame_depth(), IC.INTR, EYE, levels=levels, image=RC.wavy_image(), photo_weight=LAM)
    got = run(dev_planes, IC.frame_depth(), RC.wavy_image(), levels=levels, read=True)
    h = icp.read_history(want["history"], rgbd=True)
    print(want["info"]["status_name"], "ran", h["ran"], "accepted", h["accepted"], want["info"]["photo"], "sum r_I^2", h["sum_ri2"])
    assert RC.same_result(got, want)
    assert got["info"]["status"] == want["status"] and icp.status_ok(want["status"]) and int(got["status"]) == want["status"]
    assert got["info"]["photo"] == want["info"]["photo"] and got["info"]["sum_ri2"] == want["info"]["sum_ri2"]
    assert np.array_equal(got["info"]["history"]["sum_ri2"], h["sum_ri2"]) and np.array_equal(got["info"]["history"]["ran"], h["ran"])
    assert np.array_equal(got["info"]["T_w2c"], want["T_w2c"]) and np.array_equal(got["info"]["D"], want["D"])
    again = run(dev_planes, IC.frame_depth(), RC.wavy_image(), levels=levels)
    assert same_bytes(again, got, ("record", "history", "D", "T_w2c", "intensity", "model_intensity"))


# ---- 4. more than one trip ---------------------------------------------------------------------------------------------
def test_more_than_one_trip_of_the_rows_kernel(built):
    """320 x 240 is 1200 tiles of 8 x 8 for the 1024 waves of the persistent grid: 176 waves make a second trip."""
    from monogs_amd import icp
    h, w, intr = 240, 320, (274.0, 274.0, 159.5, 119.5)
    assert (w // 8) * (h // 8) > icp.ROWS_TILES and h * w > icp.ROWS_LANES
    dev_planes, host = model("dense", "wavy", h, w, intr)
    depth = IC.frame_depth(h, w, intr)
    image = RC.painted(depth, IC.true_pose(), intr)
    levels = ((1, 2),)
    want = icp.align_numpy(host, depth, intr, EYE, levels=levels, image=image, photo_weight=LAM)
    got = run(dev_planes, depth, image, view=intr, levels=levels)
    print(want["info"]["counts"], want["info"]["photo"], want["info"]["status_name"])
    assert want["info"]["counts"]["accepted"] > 40000 and want["info"]["photo"]["accepted"] > 40000 and RC.same_result(got, want)


# ---- 5. layouts and intrinsics ----------------------------------------------------------------------------------------
def test_both_layouts_and_other_model_intrinsics(built):
    from monogs_amd import icp
    dev_planes, host = model("dense", "wavy")
    levels = ((2, 2), (1, 2))
    got = run(dev_planes, IC.frame_depth(), RC.wavy_image(), levels=levels)
    chw = {"depth": dev_planes["depth"], "normal": dev_planes["normal"].permute(2, 0, 1).contiguous(),
           "color": dev_planes["color"].permute(2, 0, 1).contiguous()}
    other = run(chw, IC.frame_depth(), RC.wavy_image().permute(1, 2, 0).contiguous(), levels=levels)
    assert same_bytes(other, got, ("record", "history", "D", "T_w2c", "intensity", "model_intensity"))
    h, w, mintr = 40, 56, (55.0, 57.0, 27.0, 19.5)         # a narrower model view: some frame pixels project outside it
    dev_m, host_m = model("sparse", "wavy", h, w, mintr)
    want = icp.align_numpy(host_m, IC.frame_depth(), IC.INTR, EYE, model_view=mintr, levels=levels, image=RC.wavy_image(), photo_weight=LAM)
    print(want["info"]["counts"], want["info"]["photo"], want["info"]["status_name"])
    assert want["info"]["counts"]["accepted"] > 1500 and want["info"]["counts"]["outside"] > 0 and want["info"]["photo"]["accepted"] > 1500
    assert RC.same_result(run(dev_m, IC.frame_depth(), RC.wavy_image(), model_view=mintr, levels=levels), want)


# ---- 6. hostile input -------------------------------------------------------------------------------------------------
def guarded(t, sentinel):
    """(a view of t's values inside a buffer with `sentinel` on both sides, the buffer)."""
    buf = torch.full((GUARD + t.numel() + GUARD,), sentinel, dtype=t.dtype, device=t.device)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return buf[GUARD:GUARD + t.numel()].view(t.shape), buf


HOSTILE_T = {
    "nan": lambda T: T.__setitem__((0, 1), float("nan")),
    "inf": lambda T: T.__setitem__((2, 3), float("inf")),
    "huge_t": lambda T: T.__setitem__((slice(0, 3), 3), 1e30),
    "huge_all": lambda T: T.mul_(3e38),
    "aside": lambda T: T.__setitem__((slice(0, 2), 3), torch.tensor([1.1, -0.8])),
    "none": lambda T: None,
}


@pytest.mark.parametrize("name", sorted(HOSTILE_T))
def test_hostile_input_stays_inside_the_planes(built, name):
    """An ordinary bounds test: NaN, inf and +-1e30 in the image, the model colour, both depths, the model normal and D
    (through T_init).  The guard bands around the planes hold values that WOULD be accepted (a depth on the surface, a
    normal of (-0.6, -0.6, -0.6), a grey of 0.5, with the gates wide open), so a read outside the planes changes the
    sums; the mirror reads inside only.  Everything must equal the mirror and end with a defined status."""
    from monogs_amd import icp
    from monogs_amd.surface import depth_normal_torch
    _, host = model("dense", "wavy")
    depth = IC.frame_depth().clone()
    depth[3:6, 10:20], depth[20:23, 30:40], depth[30:34, 5:15] = float("nan"), float("inf"), 1e30
    depth[10:14, 50:60], depth[40:42, 40:60], depth[25:27, 60:66] = -1e30, 3e38, 15.9
    image = RC.wavy_image().clone()
    image[0, 8:11, 30:50], image[1, 26:28, 10:30], image[2, 35:37, 20:40] = float("nan"), float("inf"), 1e30
    image[1, 15:17, 5:25], image[0, 2, :] = -1e30, 1.0001
    md, mn, mc = host["depth"].clone(), host["normal"].clone(), host["color"].clone()
    md[5:8, 5:30], md[12, 3:40], md[30:33, 20:50] = float("nan"), float("inf"), 1e30
    mn[18:20, 10:60], mn[24, :, 1], mn[36:38, 5:25] = float("nan"), 5.0, float("inf")
    mc[14:16, 20:60, 0], mc[27, 5:50, 1], mc[38:40, 30:65, 2], mc[21, 10:30, 0] = float("nan"), float("inf"), 1e30, -1e30
    hostile = {"depth": md, "normal": mn, "color": mc}
    T_init = torch.eye(4)
    HOSTILE_T[name](T_init)
    kw = dict(levels=((2, 2), (1, 2)), dist=2.0, cos_min=0.0, depth_max=16.0)
    want = icp.align_numpy(hostile, depth, IC.INTR, EYE, T_init=T_init.numpy(), image=image, photo_weight=LAM,
                           sensor_normal=depth_normal_torch(depth, *IC.INTR, pixel_center=0.0), **kw)
    dev = _dev()
    (gd, buf_d), (gn, buf_n), (gc, buf_c), (gi, buf_i) = guarded(md.to(dev), 1.45), guarded(mn.to(dev), -0.6), guarded(mc.to(dev), 0.5), \
        guarded(image.to(dev), 0.5)
    depth_d, T_d = depth.to(dev), T_init.to(dev)          # on the device here, so that they can be scrubbed below
    got = run({"depth": gd, "normal": gn, "color": gc}, depth_d, gi, T_init=T_d, **kw)
    rec = got["record"].cpu().numpy()
    info = icp.read_record(rec, rgbd=True)
    print(name, info["status_name"], info["counts"], info["photo"])
    assert 0 <= info["status"] <= icp.STEP_TOO_LARGE and info["status"] == want["status"]
    assert np.array_equal(rec, want["record"]) and np.array_equal(got["history"].cpu().numpy(), want["history"])
    assert np.array_equal(got["D"].cpu().numpy(), want["D"], equal_nan=True)
    assert np.array_equal(got["T_w2c"].cpu().numpy(), want["T_w2c"], equal_nan=True)
    for k in ("intensity", "model_intensity"):
        assert np.array_equal(got[k].cpu().numpy().view(np.int32), want[k].numpy().view(np.int32)), k
    assert sum(info["counts"].values()) == (23 * 35 if info["level"] == 0 else IC.H * IC.W)
    assert sum(info["photo"].values()) == info["counts"]["accepted"] + sum(info["counts"][k] for k in ("no_model", "distance", "normal"))
    for buf, sentinel, n in ((buf_d, 1.45, md.numel()), (buf_n, -0.6, mn.numel()), (buf_c, 0.5, mc.numel()), (buf_i, 0.5, image.numel())):
        assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())
    if name == "none":
        assert info["counts"]["accepted"] > 1000 and info["counts"]["no_model"] > 100 and info["photo"]["accepted"] > 1000
        assert info["photo"]["invalid"] > 300
    if name == "aside":
        assert info["counts"]["outside"] > 100
    scrub(buf_d, buf_n, buf_c, buf_i, depth_d, T_d, got["D"], got["T_w2c"], got["record"], got["history"])


def test_the_bound_gate_on_the_device(built):
    """p_z = 0.05 puts fx / p_z = 1200 on the texture's gradient: the photometric rows beyond |w_i| < 16 are counted and
    left out, the geometric rows stay - and the device agrees with the mirror on every one of them."""
    from monogs_amd import icp
    near = torch.full((IC.H, IC.W), 0.05)
    m = dict(RC.plane_model(), depth=near)
    image = RC.plane_frame()[1]
    kw = dict(levels=((1, 2),), depth_max=1.0, min_pivot_ratio=0.0, damping=1e-3)
    want = icp.align_numpy(m, near, IC.INTR, EYE, image=image, photo_weight=LAM, **kw)
    got = run({k: v.to(_dev()) for k, v in m.items()}, near, image, **kw)
    print(want["info"]["status_name"], want["info"]["counts"], want["info"]["photo"])
    assert want["info"]["photo"]["bound"] > 100 and want["info"]["photo"]["accepted"] > 100 and want["info"]["counts"]["accepted"] > 2000
    assert RC.same_result(got, want)


# ---- 7. the textured plane through both volumes -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_textured_plane_through_track(built, kind):
    """Geometry alone ends degenerate on the fused plane; with the colour the status is converged, within icp_cases' caps
    and within twice what the mirror measures on the same ray cast (the device is bit-equal to it)."""
    from monogs_amd import icp
    dev = _dev()
    vol = volume(kind, "plane")
    depth, image, _ = RC.plane_frame()
    view = (torch.eye(4, device=dev), *IC.INTR, IC.H, IC.W)
    kw = dict(z_far=IC.Z_FAR, levels=((1, 10),))
    geo = vol.track(depth.to(dev), torch.eye(4, device=dev), view, **kw)
    print(kind, "geometry alone:", geo["info"]["status_name"], geo["info"]["pivots"], geo["info"]["counts"])
    assert geo["info"]["status"] == icp.DEGENERATE and "photo" not in geo["info"] and torch.equal(geo["T_w2c"].cpu(), torch.eye(4))
    plain = icp.align(geo["model"], depth.to(dev), IC.INTR, EYE, levels=((1, 10),))
    assert same_bytes(plain, geo)                                   # photo_weight = 0: the bytes of mgs_icp_align
    off = vol.track(depth.to(dev), torch.eye(4, device=dev), view, image=image.to(dev), photo_weight=0.0, **kw)
    assert same_bytes(off, geo) and "intensity" not in off
    res = vol.track(depth.to(dev), torch.eye(4, device=dev), view, image=image, photo_weight=LAM, **kw)
    info = res["info"]
    want = icp.align_numpy({k: v.cpu() for k, v in res["model"].items()}, depth, IC.INTR, EYE, levels=((1, 10),), image=image,
                           photo_weight=LAM)
    et, er = IC.pose_error(info["T_w2c"], RC.plane_pose())
    mt, mr = IC.pose_error(want["T_w2c"], RC.plane_pose())
    print(f"{kind}: {info['status_name']} after {info['iterations_run']}, {et:.2e} m / {er:.2e} deg (mirror {mt:.2e} / {mr:.2e}), geometric "
          f"{info['counts']}, photometric {info['photo']}, pivots {info['pivots']}, sum r_I^2 {info['history']['sum_ri2'][:info['iterations_run']]}")
    assert info["ok"] and info["status"] == icp.CONVERGED and want["status"] == icp.CONVERGED
    assert et <= IC.CAP_T and er <= IC.CAP_R_DEG and et <= 2 * mt and er <= 2 * mr
    assert RC.same_result(res, want)
    dense, sparse = model("dense", "plane")[1], model("sparse", "plane")[1]
    planes_equal = all(torch.equal(dense[k], sparse[k]) for k in ("depth", "normal", "color"))
    print("the ray casts of the dense and the sparse volume are equal:", planes_equal)
    if kind == "sparse" and planes_equal:
        other = volume("dense", "plane").track(depth.to(dev), torch.eye(4, device=dev), view, image=image, photo_weight=LAM, **kw)
        assert same_bytes(other, res, ("record", "history", "D", "T_w2c", "intensity", "model_intensity"))


def test_a_volume_fused_without_colour_is_refused(built):
    from monogs_amd.tsdf import TSDFVolume
    dev = _dev()
    vol = TSDFVolume(IC.ORIGIN, IC.VS, IC.DIMS, device=dev)
    depth, image, _ = RC.plane_frame()
    vol.integrate(depth.to(dev), torch.eye(4, device=dev), *IC.INTR)
    view = (torch.eye(4, device=dev), *IC.INTR, IC.H, IC.W)
    with pytest.raises(ValueError, match="colour"):
        vol.track(depth.to(dev), torch.eye(4, device=dev), view, image=image, photo_weight=LAM, z_far=IC.Z_FAR)
    assert vol.track(depth.to(dev), torch.eye(4, device=dev), view, z_far=IC.Z_FAR, levels=((1, 1),))["info"]["iterations_run"] == 1


# ---- 8. run_sequence --------------------------------------------------------------------------------------------------
def test_run_sequence_with_photometric_icp_init(built):
    """Completes and returns the new counts; nothing is claimed about ATE."""
    from monogs_amd import icp, slam_surrogate as SS
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    dev = _dev()
    Hh, Ww, n = 120, 160, 4
    frames, cam, _ = SS.load_sequence(n, Ww, Hh, dev, world_gaussians=3000)
    kw = dict(sensor_depth=True, kf_interval=2, init_iters=20, mapping_iters=5, first_order_iters=5, second_order_iters=0)
    vol = SparseTSDFVolume((0.0, 0.0, 0.0), 0.1, 6000, device=dev)
    got = SS.run_sequence(frames, cam, dev, mesh_volume=vol, icp_init=True, icp_kw=dict(z_far=10.0, photo_weight=LAM), **kw)
    torch.cuda.synchronize()
    assert vol.has_color and sorted(got["icp_records"]) == [1, 2, 3] and sorted(got["cameras"]) == [0, 1, 2, 3]
    for k, rec in got["icp_records"].items():
        print(k, rec["status_name"], rec["counts"], rec["photo"], rec["sum_ri2"], rec["iterations_run"])
        assert 0 <= rec["status"] <= icp.STEP_TOO_LARGE and rec["iterations_run"] >= 1
        assert sum(rec["counts"].values()) > 0 and sum(rec["photo"].values()) > 0 and bool(torch.isfinite(got["cameras"][k].T).all())
        assert sum(rec["photo"].values()) == rec["counts"]["accepted"] + sum(rec["counts"][c] for c in ("no_model", "distance", "normal"))
