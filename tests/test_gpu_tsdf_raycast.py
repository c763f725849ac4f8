"""GPU tests of the ray cast of the TSDF volumes (csrc/tsdf_raycast.hip): the device against the mirror bit for bit, with
and without skipping, sparse against dense, guards, the neighbour table's rebuild rule, the frames, the number held
against the mesh route, and the two hooks."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import sparse_tsdf_cases as SC
import tsdf_cases as K
import tsdf_raycast_cases as RC

pytestmark = pytest.mark.gpu

GUARD = 4
SENTINEL = 12345.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def cast(vol, T, **kw):
    r = vol.raycast(T.to(_dev()), *RC.INTR, RC.H, RC.W, **kw)
    torch.cuda.synchronize()
    return r


def integrate_views(vol, first, last):
    dev = _dev()
    depth, kw, image = SC.view_inputs(False, True)
    for T, vw, allocate in SC.views()[first:last]:
        vol.integrate(depth.to(dev), T.to(dev), SC.FX, SC.FY, SC.CX, SC.CY, image=image.to(dev), weight=vw, allocate=allocate, **kw)


@functools.lru_cache(maxsize=None)
def views_volume():
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    vol = SparseTSDFVolume(SC.ORIGIN, SC.VS, SC.MAX_BRICKS, device=_dev(), max_weight=SC.MAX_WEIGHT)
    integrate_views(vol, 0, 4)
    torch.cuda.synchronize()
    return vol


@functools.lru_cache(maxsize=None)
def sphere_volumes():
    """(sparse, dense, dense filled from the sparse volume's to_dense()) of the 24^3 sphere: one lattice, one origin."""
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    from monogs_amd.tsdf import TSDFVolume
    dev = _dev()
    planes = RC.sphere()
    sparse = SparseTSDFVolume.from_dense(K.ORIGIN, K.VOXEL, *planes, device=dev)
    dense, refill = (TSDFVolume(K.ORIGIN, K.VOXEL, RC.SPHERE_DIMS, device=dev) for _ in range(2))
    for plane, src in zip((dense.tsdf, dense.weight, dense.color), planes):
        plane.copy_(torch.from_numpy(src))
    origin, t, w, c = sparse.to_dense()
    assert origin == tuple(float(np.float32(v)) for v in K.ORIGIN) and tuple(t.shape) == RC.SPHERE_DIMS[::-1]
    for plane, src in zip((refill.tsdf, refill.weight, refill.color), (t, w, c)):
        plane.copy_(src)
    return sparse, dense, refill


@functools.lru_cache(maxsize=None)
def far_volume():
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    return SparseTSDFVolume.from_dense(K.ORIGIN, K.VOXEL, *RC.far_sphere(), lo=SC.FAR_LO, device=_dev())


# ---- device against mirror, skip against no skip ---------------------------------------------------------------------
@pytest.mark.parametrize("p", range(6))
def test_views_volume_equals_the_mirror(built, p):
    vol = views_volume()
    assert np.array_equal(vol.bricks().cpu().numpy(), RC.views_bricks()[0])
    T = RC.views_poses()[p]
    want = RC.views_mirror(p)
    hs = want["hit_step"]
    print(f"pose {p}: hit {int((hs >= 0).sum())}, ran out {int((hs == -1).sum())}, back face {int((hs == -2).sum())}")
    got = cast(vol, T, **RC.VIEWS_KW)
    assert RC.same_planes(got, want)
    plain = cast(vol, T, skip=False, **RC.VIEWS_KW)
    assert RC.same_planes(plain, got)
    again = cast(vol, T, **RC.VIEWS_KW)
    assert RC.same_planes(again, got)                                          # two runs are byte-equal
    if p == 4:
        assert RC.same_planes(cast(vol, T, frame="world", **RC.VIEWS_KW), RC.views_mirror(p, "world"))


@pytest.mark.parametrize("p", range(2))
def test_sphere_sparse_dense_and_mirror(built, p):
    """From outside (rays enter and leave the box, a third misses it) and from inside (back faces)."""
    sparse, dense, refill = sphere_volumes()
    T = RC.sphere_poses()[p]
    want = RC.sphere_mirror(p)
    hs = want["hit_step"]
    assert int((hs >= 0).sum()) > 500 and int((hs == -1).sum()) > 500 if p == 0 else bool((hs == -2).all())
    for vol in (sparse, dense, refill):
        got = cast(vol, T, **RC.SPHERE_KW)
        assert RC.same_planes(got, want), type(vol).__name__
        assert RC.same_planes(cast(vol, T, skip=False, **RC.SPHERE_KW), got), type(vol).__name__
    assert RC.same_planes(cast(dense, T, frame="world", **RC.SPHERE_KW), RC.sphere_mirror(p, "world"))


@pytest.mark.parametrize("p", range(2))
def test_far_sphere_equals_the_mirror(built, p):
    """Lattice indices around (-1500, 900, 1700): an ulp of l is 1.2e-4 voxel, the skip margin has to scale with it."""
    vol = far_volume()
    T = RC.far_poses()[p]
    want = RC.far_mirror(p)
    assert int((want["hit_step"] >= 0).sum()) > 1000 and int((want["hit_step"] == -1).sum()) > 500
    got = cast(vol, T, **RC.FAR_KW)
    assert RC.same_planes(got, want)
    assert RC.same_planes(cast(vol, T, skip=False, **RC.FAR_KW), got)


# ---- guards ----------------------------------------------------------------------------------------------------------
def guarded(vol):
    """Replaces every pool plane of `vol` by a view into a buffer with sentinels on both sides; returns the checks."""
    checks = []
    for name in ("tsdf", "weight", "color", "brick_coords"):
        old = getattr(vol, name)
        sentinel = SENTINEL if old.dtype == torch.float32 else 12345
        buf = torch.full((GUARD + old.numel() + GUARD,), sentinel, dtype=old.dtype, device=old.device)
        buf[GUARD:GUARD + old.numel()] = old.reshape(-1)
        setattr(vol, name, buf[GUARD:GUARD + old.numel()].view(old.shape))
        checks.append((name, buf, old.numel(), sentinel))
    return checks


def guards_intact(checks):
    return all(bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + n:] == s).all()) for _, buf, n, s in checks)


def test_guards_around_outputs_and_pool_stay_intact(built):
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    dev = _dev()
    vol = SparseTSDFVolume(SC.ORIGIN, SC.VS, SC.MAX_BRICKS, device=dev, max_weight=SC.MAX_WEIGHT)
    checks = guarded(vol)
    integrate_views(vol, 0, 4)
    shapes = {"depth": (RC.H, RC.W), "normal": (RC.H, RC.W, 3), "color": (RC.H, RC.W, 3), "hit_step": (RC.H, RC.W)}
    bufs, out = {}, {}
    for k, s in shapes.items():
        dt = torch.int32 if k == "hit_step" else torch.float32
        n = int(np.prod(s))
        bufs[k] = torch.full((GUARD + n + GUARD,), 12345, dtype=dt, device=dev)
        out[k] = bufs[k][GUARD:GUARD + n].view(s)
    pool = {n: getattr(vol, n).clone() for n in ("tsdf", "weight", "color", "brick_coords", "map_keys", "map_vals", "state")}
    for p in (0, 5):
        for skip in (True, False):
            got = cast(vol, RC.views_poses()[p], out=out, skip=skip, **RC.VIEWS_KW)
            assert got is out and RC.same_planes(got, RC.views_mirror(p))
    assert guards_intact(checks)
    for k, s in shapes.items():
        n = int(np.prod(s))
        assert bool((bufs[k][:GUARD] == 12345).all()) and bool((bufs[k][GUARD + n:] == 12345).all()), k
    for n, before in pool.items():
        assert torch.equal(getattr(vol, n), before), n                          # the ray cast writes nothing of the volume


# ---- the neighbour table's rule ---------------------------------------------------------------------------------------
def test_a_ray_cast_after_more_bricks_sees_them(built):
    from monogs_amd import tsdf_raycast as R
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    vol = SparseTSDFVolume(SC.ORIGIN, SC.VS, SC.MAX_BRICKS, device=_dev(), max_weight=SC.MAX_WEIGHT)
    integrate_views(vol, 0, 1)
    assert R.neighbor_table(vol)[1]                                             # no table yet
    first = cast(vol, RC.views_poses()[1], **RC.VIEWS_KW)
    assert RC.same_planes(first, RC.views_mirror(1, "camera", 0))
    table, build = R.neighbor_table(vol)
    assert not build                                                            # nothing was added: the table is kept
    kept = table.clone()
    assert RC.same_planes(cast(vol, RC.views_poses()[1], **RC.VIEWS_KW), first) and torch.equal(table, kept)
    integrate_views(vol, 1, 4)                                                  # the second view adds bricks
    assert len(RC.views_bricks(-1)[0]) > len(RC.views_bricks(0)[0]) and R.neighbor_table(vol)[1]
    got = cast(vol, RC.views_poses()[1], **RC.VIEWS_KW)
    assert RC.same_planes(got, RC.views_mirror(1)) and not RC.same_planes(got, first, show=False)
    assert not torch.equal(R.neighbor_table(vol)[0], kept)
    B = len(RC.views_bricks(-1)[0])
    nbr = R.neighbor_table(vol)[0].view(-1, 27).cpu()
    assert bool((nbr[:B, 13] == torch.arange(B, dtype=torch.int32)).all()) and bool((nbr[B:] == -1).all())


# ---- frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shaded", "normal", "color", "depth"])
def test_frames_equal_the_numpy_mirror(built, mode):
    from monogs_amd.tsdf_raycast import raycast_frame, raycast_frame_numpy
    vol = views_volume()
    bg = (0.2, 0.4, 0.9)
    for p in (0, 4):
        view = (RC.views_poses()[p].to(_dev()), *RC.INTR, RC.H, RC.W)
        frame = raycast_frame(vol, view, mode, bg, **RC.VIEWS_KW)
        torch.cuda.synchronize()
        want = raycast_frame_numpy(RC.views_mirror(p), view, mode, bg, (RC.VIEWS_KW["z_near"], RC.VIEWS_KW["z_far"]))
        assert frame.dtype == torch.uint8 and tuple(frame.shape) == (RC.H, RC.W, 3)
        assert np.array_equal(frame.cpu().numpy(), want)
        miss = RC.views_mirror(p)["hit_step"].numpy() < 0
        assert miss.any() and (want[miss] == np.array([51, 102, 229], np.uint8)).all() and len(np.unique(want[~miss])) > 3
    with pytest.raises(ValueError):
        raycast_frame(vol, view, "wireframe", bg, **RC.VIEWS_KW)


# ---- a number the test holds: the ray cast against the mesh route -----------------------------------------------------
MESH_MEASURED = 0.014272      # max |z_raycast - z_mesh| of the mirrors on this view (DESIGN.md "Ray cast of the volumes")


def test_depth_against_the_rendered_mesh(built):
    from monogs_amd.mesh_render import render_mesh_depth, render_mesh_depth_numpy
    from monogs_amd.tsdf import extract_mesh_numpy
    cap = np.sqrt(3.0) * K.VOXEL
    bound = 2.0 * MESH_MEASURED
    assert bound <= cap
    # the condition on the CPU: the mirrors stay inside the cap
    T = RC.sphere_poses()[0]
    v, f, _ = extract_mesh_numpy(*RC.sphere(), K.ORIGIN, K.VOXEL)
    zm, fid, _ = render_mesh_depth_numpy(v, f, T, *RC.INTR, RC.H, RC.W, RC.SPHERE_KW["z_near"])
    zr = RC.sphere_mirror(0)["depth"].numpy()
    both = (zr > 0) & (fid >= 0)
    mirror_max = float(np.abs(zr - zm)[both].max())
    print(f"mirrors: max |z_raycast - z_mesh| = {mirror_max:.6f} over {int(both.sum())} pixels (cap {cap:.6f})")
    assert mirror_max <= cap
    # the device: the parent's route against the ray cast
    _, dense, _ = sphere_volumes()
    verts, faces, _ = dense.extract_mesh()
    depth, face_id, _ = render_mesh_depth(verts, faces, T.to(_dev()), *RC.INTR, RC.H, RC.W, RC.SPHERE_KW["z_near"])
    got = cast(dense, T, **RC.SPHERE_KW)
    hr, hm = (got["hit_step"] >= 0).cpu().numpy(), (face_id >= 0).cpu().numpy()
    diff = (got["depth"] - depth).abs().cpu().numpy()
    both = hr & hm
    print(f"device: max |z_raycast - z_mesh| = {float(diff[both].max()):.6f} over {int(both.sum())} pixels, "
          f"{int((hr ^ hm).sum())} pixels hit by one only")
    assert both.sum() > 900 and float(diff[both].max()) <= bound
    pad = np.pad(hm, 1, mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + RC.H, 1 + dx:1 + dx + RC.W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    silhouette = nb.any(0) & ~nb.all(0)                                         # within one pixel of the mesh's outline
    assert not ((hr ^ hm) & ~silhouette).any()


def test_volume_depth_l1(built):
    from monogs_amd.tsdf_raycast import volume_depth_l1
    vol = views_volume()
    depth, _, _ = SC.view_planes()
    depth = torch.where(torch.isfinite(depth), depth, torch.zeros(()))          # a sensor marks what it did not measure with 0
    views = [(RC.views_poses()[p], *RC.INTR, RC.H, RC.W) for p in (0, 1)]
    got = volume_depth_l1(vol, views, [depth, depth], **RC.VIEWS_KW)
    s = n = 0.0
    for p in (0, 1):
        z = RC.views_mirror(p)["depth"]
        both = (z > 0) & (depth > 0)
        s += float((z - depth).abs()[both].double().sum())
        n += int(both.sum())
    assert got["pixels"] == n > 2000 and abs(got["l1"] - s / n) <= 1e-9 * max(1.0, s / n)
    assert np.isnan(volume_depth_l1(vol, views[:1], [torch.zeros(RC.H, RC.W)], **RC.VIEWS_KW)["l1"])


# ---- hooks -----------------------------------------------------------------------------------------------------------
def _count_frames(monkeypatch):
    from monogs_amd import tsdf_raycast as R
    calls = []
    real = R.raycast_frame

    def counted(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(R, "raycast_frame", counted)
    return calls


def test_save_mesh_writes_the_volume_preview(built, tmp_path, monkeypatch):
    from monogs_amd.eval_native import save_mesh
    calls = _count_frames(monkeypatch)
    sparse, dense, _ = sphere_volumes()
    view = (RC.sphere_poses()[0].to(_dev()), *RC.INTR, RC.H, RC.W)
    for n, vol in enumerate((sparse, dense)):
        plain = save_mesh(vol, str(tmp_path / f"plain{n}"))
        assert calls == [] and not glob.glob(str(tmp_path / f"plain{n}" / "point_cloud" / "final" / "volume_preview.*"))
        path = save_mesh(vol, str(tmp_path / f"with{n}"), volume_preview=view, volume_preview_kw=dict(z_far=2.0))
        assert len(calls) == 1 and calls.pop()["z_far"] == 2.0
        assert open(path, "rb").read() == open(plain, "rb").read()                 # the mesh file does not change
        files = glob.glob(os.path.join(os.path.dirname(path), "volume_preview.*"))
        assert len(files) == 1 and os.path.getsize(files[0]) > RC.H * RC.W // 4


def test_run_sequence_keeps_previews_of_the_volume(built, monkeypatch):
    from monogs_amd import slam_surrogate as SS
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    calls = _count_frames(monkeypatch)
    dev = _dev()
    Hh, Ww, n = 120, 160, 3
    frames, cam, _ = SS.load_sequence(n, Ww, Hh, dev, world_gaussians=3000)
    kw = dict(sensor_depth=True, kf_interval=1, init_iters=20, mapping_iters=5, first_order_iters=5, second_order_iters=0)
    vol = SparseTSDFVolume((0.0, 0.0, 0.0), 0.1, 6000, device=dev)
    plain = SS.run_sequence(frames, cam, dev, mesh_volume=vol, mesh_every=1, **kw)
    assert calls == [] and "mesh_previews" not in plain
    vol2 = SparseTSDFVolume((0.0, 0.0, 0.0), 0.1, 6000, device=dev)
    shown = SS.run_sequence(frames, cam, dev, mesh_volume=vol2, mesh_every=1, mesh_preview_every=2, **kw)
    torch.cuda.synchronize()
    assert shown["mesh_keyframes"] == [0, 1, 2] and sorted(shown["mesh_previews"]) == [0, 2] and len(calls) == 2
    for k in range(n):
        assert torch.equal(shown["cameras"][k].T, plain["cameras"][k].T), k          # the same trajectory
    assert torch.equal(vol.tsdf, vol2.tsdf) and torch.equal(vol.state, vol2.state)
    for k, frame in shown["mesh_previews"].items():
        assert frame.dtype == torch.uint8 and tuple(frame.shape) == (Hh, Ww, 3) and frame.device.type == "cuda"
    assert int((shown["mesh_previews"][2] > 0).any(-1).sum()) > Hh * Ww // 10         # the fused surface fills the view
