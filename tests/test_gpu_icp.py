"""GPU tests of the frame-to-model ICP (csrc/icp.hip): the device against the NumPy mirror bit for bit - one iteration, whole
schedules, more than one trip of the rows kernel, both normal layouts, other model intrinsics - the statuses, hostile input
around guarded model planes, recovery of a known motion through track_against_volume, and run_sequence(icp_init=True).
The model planes are the device's own ray cast of the wavy volume, fused on the device (icp_cases.py)."""
import functools

import numpy as np
import pytest
import torch

import icp_cases as IC

pytestmark = pytest.mark.gpu

GUARD = 256
EYE = np.eye(4, dtype=np.float32)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def volume(kind):
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    from monogs_amd.tsdf import TSDFVolume
    dev = _dev()
    vol = TSDFVolume(IC.ORIGIN, IC.VS, IC.DIMS, device=dev) if kind == "dense" else SparseTSDFVolume(IC.ORIGIN, IC.VS, IC.MAX_BRICKS, device=dev)
    for T in IC.fusion_poses():
        vol.integrate(IC.surface_depth(T).to(dev), torch.from_numpy(T).float().to(dev), *IC.INTR)
    torch.cuda.synchronize()
    return vol


@functools.lru_cache(maxsize=None)
def model(kind, h=IC.H, w=IC.W, intr=IC.INTR):
    """(the ray cast at T = I on the device, the same planes on the host)."""
    planes = volume(kind).raycast(torch.eye(4, device=_dev()), *intr, h, w, z_far=IC.Z_FAR)
    torch.cuda.synchronize()
    return planes, {k: v.cpu() for k, v in planes.items()}


def run(model_, depth, **kw):
    from monogs_amd import icp
    kw.setdefault("read", False)
    view = kw.pop("view", IC.INTR)
    T_model = kw.pop("T_model", EYE)
    out = icp.align(model_, depth.to(_dev()), view, T_model, **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. one iteration -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_one_iteration_equals_rows_and_solve(built, kind, stride):
    from monogs_amd import icp
    dev_planes, host = model(kind)
    hit = int((host["hit_step"] >= 0).sum())
    same = all(torch.equal(host[k], model("dense")[1][k]) for k in ("depth", "normal"))
    print(f"{kind}: {hit} of {IC.H * IC.W} rays hit; planes equal to the dense volume's: {same}")
    assert hit > 2500
    got = run(dev_planes, IC.frame_depth(), levels=((stride, 1),))
    D0 = icp.initial_transform(EYE)
    sums, counts = icp.icp_rows_numpy(host, IC.frame_depth(), IC.sensor_normal(), D0, IC.INTR, stride=stride)
    s = icp.icp_solve_numpy(sums, counts[0], D0, last=True)
    rec = got["record"].cpu().numpy()
    info = icp.read_record(rec)
    print(stride, info["status_name"], info["counts"], info["x"])
    assert np.array_equal(rec[:28], sums) and np.array_equal(rec[28:35], counts)
    assert int(counts.sum()) == -(-IC.H // stride) * -(-IC.W // stride) and counts[0] > 100
    assert np.array_equal(info["x"].view(np.int64), s["x"].view(np.int64))
    assert np.array_equal(info["pivots"].view(np.int64), s["pivots"].view(np.int64))
    assert info["status"] == s["status"] == icp.MAX_ITERATIONS and info["iterations_run"] == 1
    assert np.array_equal(got["D"].cpu().numpy().view(np.int64), s["D"].view(np.int64))
    assert np.array_equal(got["T_w2c"].cpu().numpy().view(np.int32), icp.pose_of(s["D"], EYE).view(np.int32))


# ---- 2. schedules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [None, ((1, 10),), ((3, 2), (1, 2))])
def test_schedules_equal_the_mirror(built, levels):
    from monogs_amd import icp
    levels = icp.LEVELS if levels is None else levels
    dev_planes, host = model("dense")
    want = icp.align_numpy(host, IC.frame_depth(), IC.INTR, EYE, levels=levels, sensor_normal=IC.sensor_normal())
    got = run(dev_planes, IC.frame_depth(), levels=levels, read=True)
    h = icp.read_history(want["history"])
    print(want["info"]["status_name"], "ran", h["ran"], "accepted", h["accepted"])
    assert IC.same_result(got, want)
    assert got["info"]["status"] == want["status"] and np.array_equal(got["info"]["history"]["ran"], h["ran"])
    assert np.array_equal(got["info"]["T_w2c"], want["T_w2c"]) and np.array_equal(got["info"]["D"], want["D"])
    assert int(got["status"]) == want["status"]
    if len(levels) == 3:
        assert 0 in h["ran"] and want["status"] == icp.CONVERGED              # launches after convergence returned at once
    again = run(dev_planes, IC.frame_depth(), levels=levels)
    for k in ("record", "history", "D", "T_w2c"):
        assert torch.equal(again[k].view(torch.uint8), got[k].view(torch.uint8)), k        # two runs are byte-equal


# ---- 3. more than one trip ---------------------------------------------------------------------------------------------
def test_more_than_one_trip_of_the_rows_kernel(built):
    """320 x 240 is 1200 tiles of 8 x 8 for the 1024 waves of the persistent grid (icp.ROWS_TILES, from MGS_ICP_ROWS_BLOCKS):
    176 waves make a second trip.  The CPU and GPU cases at 70 x 45 are 54 tiles, one trip."""
    from monogs_amd import icp
    h, w, intr = 240, 320, (274.0, 274.0, 159.5, 119.5)
    assert (w // 8) * (h // 8) > icp.ROWS_TILES and h * w > icp.ROWS_LANES and -(-IC.W // 8) * -(-IC.H // 8) < icp.ROWS_TILES
    dev_planes, host = model("dense", h, w, intr)
    depth = IC.frame_depth(h, w, intr)
    levels = ((1, 2),)
    want = icp.align_numpy(host, depth, intr, EYE, levels=levels, sensor_normal=IC.sensor_normal(h, w, intr))
    got = run(dev_planes, depth, view=intr, levels=levels)
    print(want["info"]["counts"], want["info"]["status_name"])
    assert want["info"]["counts"]["accepted"] > 40000 and IC.same_result(got, want)


# ---- 4. layouts and intrinsics ----------------------------------------------------------------------------------------
def test_both_normal_layouts_and_other_model_intrinsics(built):
    from monogs_amd import icp
    dev_planes, host = model("dense")
    levels = ((2, 2), (1, 2))
    got = run(dev_planes, IC.frame_depth(), levels=levels)
    chw = {"depth": dev_planes["depth"], "normal": dev_planes["normal"].permute(2, 0, 1).contiguous()}
    other = run(chw, IC.frame_depth(), levels=levels)
    for k in ("record", "history", "D", "T_w2c"):
        assert torch.equal(other[k].view(torch.uint8), got[k].view(torch.uint8)), k
    h, w, mintr = 40, 56, (55.0, 57.0, 27.0, 19.5)         # a narrower model view: some frame pixels project outside it
    dev_m, host_m = model("sparse", h, w, mintr)
    want = icp.align_numpy(host_m, IC.frame_depth(), IC.INTR, EYE, model_view=mintr, levels=levels, sensor_normal=IC.sensor_normal())
    print(want["info"]["counts"], want["info"]["status_name"])
    assert want["info"]["counts"]["accepted"] > 1500 and want["info"]["counts"]["outside"] > 0
    assert IC.same_result(run(dev_m, IC.frame_depth(), model_view=mintr, levels=levels), want)


# ---- 5. statuses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["degenerate", "too_few", "step_too_large"])
def test_statuses_on_the_device(built, name):
    from monogs_amd import icp
    model_, depth, kw, status = IC.status_cases()[name]
    Tm = np.eye(4, dtype=np.float32)
    Tm[0, 3] = 0.25
    levels = ((2, 2), (1, 3))
    mirror_kw = dict(kw)
    if "sensor_normal" not in kw:
        from monogs_amd.surface import depth_normal_torch
        mirror_kw["sensor_normal"] = depth_normal_torch(depth, *IC.INTR, pixel_center=0.0)
    want = icp.align_numpy(model_, depth, IC.INTR, Tm, levels=levels, **mirror_kw)
    dev_model = {k: v.to(_dev()) for k, v in model_.items()}
    got = run(dev_model, depth, T_model=Tm, levels=levels, **{k: (v.to(_dev()) if torch.is_tensor(v) else v) for k, v in kw.items()})
    assert want["status"] == status and IC.same_result(got, want)
    assert np.array_equal(got["D"].cpu().numpy(), np.eye(4)[:3]) and np.array_equal(got["T_w2c"].cpu().numpy(), Tm)


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
    "behind": lambda T: T.__setitem__((2, 2), -1.0),
    "aside": lambda T: T.__setitem__((slice(0, 2), 3), torch.tensor([1.1, -0.8])),
    "none": lambda T: None,
}


@pytest.mark.parametrize("name", sorted(HOSTILE_T))
def test_hostile_input_stays_inside_the_model_planes(built, name):
    """An ordinary bounds test: NaN, inf and huge values in the sensor depth, in the model planes and in D (through T_init).
    The guard bands around the model planes hold values that WOULD be accepted (a depth on the surface, a normal of
    (-0.6, -0.6, -0.6), with the gates wide open), so a gather outside the planes changes the sums; the mirror gathers
    inside only.  Everything must equal the mirror and end with a defined status."""
    from monogs_amd import icp
    from monogs_amd.surface import depth_normal_torch
    dev_planes, host = model("dense")
    depth = IC.frame_depth().clone()
    depth[3:6, 10:20] = float("nan")
    depth[20:23, 30:40] = float("inf")
    depth[30:34, 5:15] = 1e30
    depth[10:14, 50:60] = -1e30
    depth[40:42, 40:60] = 3e38
    depth[25:27, 60:66] = 15.9
    md, mn = host["depth"].clone(), host["normal"].clone()
    md[5:8, 5:30], md[12, 3:40], md[30:33, 20:50] = float("nan"), float("inf"), 1e30
    mn[18:20, 10:60], mn[24, :, 1], mn[36:38, 5:25] = float("nan"), 5.0, float("inf")
    hostile = {"depth": md, "normal": mn}
    T_init = torch.eye(4)
    HOSTILE_T[name](T_init)
    kw = dict(levels=((2, 2), (1, 2)), dist=2.0, cos_min=0.0, depth_max=16.0)
    want = icp.align_numpy(hostile, depth, IC.INTR, EYE, T_init=T_init.numpy(), sensor_normal=depth_normal_torch(depth, *IC.INTR, pixel_center=0.0), **kw)
    gd, buf_d = guarded(md.to(_dev()), 1.45)
    gn, buf_n = guarded(mn.to(_dev()), -0.6)
    got = run({"depth": gd, "normal": gn}, depth, T_init=T_init, **kw)
    rec = got["record"].cpu().numpy()
    info = icp.read_record(rec)
    print(name, info["status_name"], info["counts"])
    assert 0 <= info["status"] <= icp.STEP_TOO_LARGE and info["status"] == want["status"]
    assert np.array_equal(rec, want["record"]) and np.array_equal(got["history"].cpu().numpy(), want["history"])
    assert np.array_equal(got["D"].cpu().numpy(), want["D"], equal_nan=True)
    assert np.array_equal(got["T_w2c"].cpu().numpy(), want["T_w2c"], equal_nan=True)
    assert sum(info["counts"].values()) == (23 * 35 if info["level"] == 0 else IC.H * IC.W)
    for buf, sentinel, n in ((buf_d, 1.45, md.numel()), (buf_n, -0.6, mn.numel())):
        assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all())
    if name == "none":
        assert info["counts"]["accepted"] > 1000 and info["counts"]["no_model"] > 100 and info["counts"]["invalid"] > 200
    if name == "aside":
        assert info["counts"]["outside"] > 100


# ---- 7. recovery ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_recovery_through_track_against_volume(built, kind):
    """The CPU suite's recovery case against the FUSED surface: the caps are half a voxel and half a degree, and the
    device may not be further off than twice what the mirror measures on the same ray cast (it is bit-equal to it)."""
    from monogs_amd import icp
    vol = volume(kind)
    view = (torch.eye(4, device=_dev()), *IC.INTR, IC.H, IC.W)
    res = vol.track(IC.frame_depth().to(_dev()), torch.eye(4, device=_dev()), view, z_far=IC.Z_FAR, levels=((1, 10),))
    info = res["info"]
    et, er = IC.pose_error(info["T_w2c"], IC.true_pose())
    want = icp.align_numpy({k: v.cpu() for k, v in res["model"].items()}, IC.frame_depth(), IC.INTR, EYE, levels=((1, 10),),
                           sensor_normal=IC.sensor_normal())
    mt, mr = IC.pose_error(want["T_w2c"], IC.true_pose())
    h = info["history"]
    rms = np.sqrt(h["sum_r2"] / np.maximum(h["accepted"], 1))[:info["iterations_run"]]
    print(f"{kind}: {info['status_name']} after {info['iterations_run']}, {et:.2e} m / {er:.2e} deg (mirror {mt:.2e} / {mr:.2e}), accepted "
          f"{info['counts']['accepted']}, rms {rms}, pivot ratio "
          f"{info['pivots'].min() / max(int(info['sums'][icp.tri(i, i)]) / 2.0 ** 30 for i in range(6)):.2e}")
    assert info["ok"] and info["status"] == icp.CONVERGED
    assert et <= IC.CAP_T and er <= IC.CAP_R_DEG and et <= 2 * mt and er <= 2 * mr
    assert np.array_equal(info["T_w2c"], want["T_w2c"])
    full = vol.track(IC.frame_depth().to(_dev()), torch.eye(4, device=_dev()), view, z_far=IC.Z_FAR)
    et, er = IC.pose_error(full["info"]["T_w2c"], IC.true_pose())
    print(f"default schedule: {full['info']['status_name']}, {et:.2e} m / {er:.2e} deg, ran {full['info']['history']['ran']}")
    assert full["info"]["ok"] and et <= IC.CAP_T and er <= IC.CAP_R_DEG


def test_select_pose_takes_the_icp_pose_only_when_the_status_is_ok(built):
    """run_sequence's device-side choice, on a converged alignment and on the three failures."""
    from monogs_amd import icp
    dev_planes, _ = model("dense")
    fallback = torch.eye(4, device=_dev())
    fallback[1, 3] = 7.0
    good = run(dev_planes, IC.frame_depth(), levels=((1, 10),))
    assert int(good["status"]) == icp.CONVERGED and not torch.equal(good["T_w2c"], fallback)
    assert torch.equal(icp.select_pose(good, fallback), good["T_w2c"])
    out = run(dev_planes, IC.frame_depth(), levels=((1, 1),))
    assert int(out["status"]) == icp.MAX_ITERATIONS and torch.equal(icp.select_pose(out, fallback), out["T_w2c"])
    for name, (model_, depth, kw, status) in IC.status_cases().items():
        bad = run({k: v.to(_dev()) for k, v in model_.items()}, depth,
                  **{k: (v.to(_dev()) if torch.is_tensor(v) else v) for k, v in kw.items()})
        assert int(bad["status"]) == status, name
        assert torch.equal(icp.select_pose(bad, fallback), fallback), name
    mid = dict(good, status=torch.tensor(icp.ITERATING, device=_dev()))
    assert torch.equal(icp.select_pose(mid, fallback), fallback)


# ---- 8. run_sequence --------------------------------------------------------------------------------------------------
def test_run_sequence_with_icp_init(built, monkeypatch):
    from monogs_amd import icp, slam_surrogate as SS, tsdf_raycast
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    dev = _dev()
    Hh, Ww, n = 120, 160, 4
    frames, cam, _ = SS.load_sequence(n, Ww, Hh, dev, world_gaussians=3000)
    kw = dict(sensor_depth=True, kf_interval=2, init_iters=20, mapping_iters=5, first_order_iters=5, second_order_iters=0)
    new_volume = lambda: SparseTSDFVolume((0.0, 0.0, 0.0), 0.1, 6000, device=dev)
    with pytest.raises(ValueError, match="icp_init"):
        SS.run_sequence(frames, cam, dev, icp_init=True, **kw)                                    # no volume
    with pytest.raises(ValueError, match="icp_init"):
        SS.run_sequence(frames, cam, dev, icp_init=True, mesh_volume=new_volume(), **dict(kw, sensor_depth=False))
    got = SS.run_sequence(frames, cam, dev, mesh_volume=new_volume(), icp_init=True, icp_kw=dict(z_far=10.0), **kw)
    torch.cuda.synchronize()
    assert sorted(got["icp_records"]) == [1, 2, 3] and sorted(got["cameras"]) == [0, 1, 2, 3]
    for k, rec in got["icp_records"].items():
        print(k, rec["status_name"], rec["counts"], rec["iterations_run"])
        assert 0 <= rec["status"] <= icp.STEP_TOO_LARGE and rec["iterations_run"] >= 1
        assert sum(rec["counts"].values()) > 0 and bool(torch.isfinite(got["cameras"][k].T).all())
    ate = {}
    ate["icp"] = SS.evaluate(got, frames, dev, monocular=False)

    def refuse(*a, **k):
        raise AssertionError("icp_init=False may call neither icp.align nor the ray cast")

    monkeypatch.setattr(icp, "align", refuse)
    monkeypatch.setattr(icp, "track_against_volume", refuse)
    monkeypatch.setattr(tsdf_raycast, "raycast", refuse)
    plain = SS.run_sequence(frames, cam, dev, mesh_volume=new_volume(), **kw)
    assert "icp_records" not in plain
    ate["plain"] = SS.evaluate(plain, frames, dev, monocular=False)
    print("ATE with / without icp_init (one short synthetic sequence):", {k: v for k, v in ate.items()})
