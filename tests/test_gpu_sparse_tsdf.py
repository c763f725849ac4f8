"""The sparse TSDF volume on the device against its mirrors (monogs_amd/sparse_tsdf.py): the brick list bit for bit in
order, the planes bit for bit, the extraction bit for bit (vertices, colours, and here the faces in order, too), and the
path from a map to a PLY file and through a run.

Sizes.  Images are 70 x 45; at a voxel of 0.05 the four views of sparse_tsdf_cases.views() hold about 240 bricks (a pool
of 400; 100 for the capacity test, below the 115 the first view alone asks for).  A view is 70 * 45 * 3 samples * 8
corners = 75 600 candidates: 296 blocks of the allocation's scan.  The extraction scans two blocks of 256 points per
brick, 1024 block totals per trip of the one-workgroup scan: the sphere on a brick corner has 8 bricks, the trip case
648 (1296 totals, the surface on both sides of brick 512)."""
import functools
import math

import numpy as np
import pytest
import torch

import sparse_tsdf_cases as SC
import tsdf_cases as K

pytestmark = pytest.mark.gpu

GUARD = 4          # floats on either side of a plane; keeps a plane at offset 0 of the guard 16-byte aligned
SENTINEL = 12345.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(torch.as_tensor(b)))


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


def snapshot(vol):
    n, dropped, out, _ = (int(v) for v in vol.state.cpu())
    return dict(n=n, dropped=dropped, out=out, bricks=vol.brick_coords[:n].cpu().numpy().copy(), tsdf=bits(vol.tsdf),
                weight=bits(vol.weight), color=bits(vol.color), keys=vol.map_keys.cpu().clone(),
                vals=vol.map_vals.cpu().clone())


def device_run(max_bricks, with_opacity, with_image, guard=False):
    """The four views of sparse_tsdf_cases.views() on the device: (vol, [snapshot after each view], guard checks)."""
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    dev = _dev()
    vol = SparseTSDFVolume(SC.ORIGIN, SC.VS, max_bricks, device=dev, max_weight=SC.MAX_WEIGHT)
    checks = guarded(vol) if guard else []
    depth, kw, image = SC.view_inputs(with_opacity, with_image)
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    snaps = []
    for T, vw, allocate in SC.views():
        vol.integrate(depth.to(dev), T.to(dev), SC.FX, SC.FY, SC.CX, SC.CY, image=None if image is None else image.to(dev),
                      weight=vw, allocate=allocate, **kw)
        torch.cuda.synchronize()
        snaps.append(snapshot(vol))
    return vol, snaps, checks


@functools.lru_cache(maxsize=None)
def cached_run(with_opacity, with_image):
    return device_run(SC.MAX_BRICKS, with_opacity, with_image)


def assert_step(snap, ref, step):
    bricks, dropped, out, t, w, c = ref
    assert snap["n"] == len(bricks) and snap["dropped"] == dropped and snap["out"] == out, (step, snap["n"], len(bricks))
    assert np.array_equal(snap["bricks"], bricks), step                       # the list, in order
    for name, want in (("tsdf", t), ("weight", w), ("color", c)):
        assert torch.equal(snap[name], bits(want)), (name, step, int((snap[name] != bits(want)).sum()))


# ---- A: allocation ---------------------------------------------------------------------------------------------------
def test_allocation_equals_the_mirror_in_order_and_is_reproducible(built):
    from monogs_amd.sparse_tsdf import SparseTSDFVolume, brick_keys
    vol, snaps, _ = cached_run(True, True)
    ref = SC.mirror_run(SC.MAX_BRICKS, True, True)
    for step, (snap, want) in enumerate(zip(snaps, ref)):
        assert np.array_equal(snap["bricks"], want[0]) and snap["dropped"] == 0 and snap["out"] == 0, step
    b = snaps[-1]["bricks"]
    assert (b.min(0) < 0).all() and (b.max(0) >= 0).all()                       # both signs on every axis
    assert len(np.unique(brick_keys(b))) == len(b)                              # the overlapping view duplicated none
    n0, n1 = snaps[0]["n"], snaps[1]["n"]
    assert 20 < n0 < n1 < SC.MAX_BRICKS and snaps[2]["n"] == n1 == snaps[3]["n"]
    assert np.array_equal(snaps[1]["bricks"][:n0], snaps[0]["bricks"])          # only new bricks, behind the old ones
    # the map holds exactly the list: every key once, its value the brick's id
    keys, vals = snaps[-1]["keys"].numpy(), snaps[-1]["vals"].numpy()
    held = keys != -1
    assert int(held.sum()) == n1
    order = np.argsort(vals[held])
    assert np.array_equal(vals[held][order], np.arange(n1)) and np.array_equal(keys[held][order], brick_keys(b))
    # a camera facing away into empty space adds none (and allocating is all it does: no plane changes)
    dev = _dev()
    T2 = SC.views()[2][0]
    vol.integrate(torch.zeros(SC.H, SC.W, device=dev), T2.to(dev), SC.FX, SC.FY, SC.CX, SC.CY, **SC.VIEW_KW)
    torch.cuda.synchronize()
    after = snapshot(vol)
    assert all(np.array_equal(np.asarray(after[k]), np.asarray(snaps[-1][k])) for k in after if k not in ("n", "dropped", "out"))
    assert (after["n"], after["dropped"], after["out"]) == (n1, 0, 0) and int(vol.state[3]) == 0
    # the whole sequence again, on a fresh volume: identical tensors.  (The map is compared as a map: which of two
    # colliding keys takes the earlier slot of a probe sequence depends on their arrival, what a lookup returns does not.)
    _, again, _ = device_run(SC.MAX_BRICKS, True, True)
    as_map = lambda snap: sorted(zip(snap["keys"][snap["keys"] != -1].tolist(), snap["vals"][snap["keys"] != -1].tolist()))
    for a, s in zip(again, snaps):
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(s[k])) for k in s if k not in ("keys", "vals"))
        assert as_map(a) == as_map(s)
    # out of range: a lattice so fine that the surface lies past 2^20 bricks is dropped and counted, not allocated
    depth, kw, _ = SC.view_inputs(False, False)
    tiny = SparseTSDFVolume((0.0, 0.0, -10.0), 1.0e-6, 16, device=dev)
    tiny.integrate(depth.to(dev), SC.views()[0][0].to(dev), SC.FX, SC.FY, SC.CX, SC.CY, **kw)
    valid = int(((depth > 0) & (depth <= 2.5)).sum())
    assert [int(v) for v in tiny.state.cpu()] == [0, 0, valid * 3 * 8, 0]


# ---- B: capacity -----------------------------------------------------------------------------------------------------
def test_capacity_keeps_the_first_bricks_and_counts_the_rest(built):
    from monogs_amd.sparse_tsdf import extract_mesh_bricks_numpy
    cap = 100
    vol, snaps, checks = device_run(cap, True, True, guard=True)
    ref = SC.mirror_run(cap, True, True)
    full = SC.mirror_run(SC.MAX_BRICKS, True, True)
    assert len(full[0][0]) > cap                                                # below what the first view alone needs
    for step, (snap, want) in enumerate(zip(snaps, ref)):
        assert_step(snap, want, step)
    last = snaps[-1]
    assert last["n"] == cap == vol.num_bricks and last["dropped"] == ref[-1][1] > 0 and vol.dropped == last["dropped"]
    assert np.array_equal(last["bricks"], full[0][0][:cap])                     # the first ones of the uncapped list
    assert guards_intact(checks)
    with pytest.raises(RuntimeError, match="not allocated"):
        vol.extract_mesh()
    verts, faces, colors = vol.extract_mesh(allow_dropped=True)
    torch.cuda.synchronize()
    assert guards_intact(checks)
    _, _, _, t, w, c = ref[-1]
    rv, rf, rc = extract_mesh_bricks_numpy(last["bricks"], t.numpy(), w.numpy(), c.numpy(), SC.ORIGIN, SC.VS, 1.0)
    assert len(rv) > 100 and same_bits(verts, rv) and same_bits(colors, rc) and np.array_equal(faces.cpu().numpy(), rf)
    assert vol.stats()["bricks"] == cap and vol.stats()["dropped"] == last["dropped"]


# ---- C: integration --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_image", [False, True])
@pytest.mark.parametrize("with_opacity", [False, True])
def test_integration_equals_the_mirror_bit_for_bit(built, with_opacity, with_image):
    vol, snaps, _ = cached_run(with_opacity, with_image)
    ref = SC.mirror_run(SC.MAX_BRICKS, with_opacity, with_image)
    for step, (snap, want) in enumerate(zip(snaps, ref)):
        assert_step(snap, want, step)
    # the view facing away culls every brick: unchanged bit for bit
    for name in ("tsdf", "weight", "color", "bricks", "keys", "vals"):
        assert np.array_equal(np.asarray(snaps[2][name]), np.asarray(snaps[1][name])), name
    changed = [int((snaps[s]["weight"] != snaps[s - 1]["weight"]).sum()) for s in (1, 3)]
    assert changed[0] > 1000 and changed[1] > 1000
    n = snaps[-1]["n"]
    w = vol.weight[:n]
    assert float(w.max()) == SC.MAX_WEIGHT                                      # 1 + 1.5 was clamped
    assert bool(torch.isfinite(vol.tsdf).all()) and float(vol.tsdf.min()) < 0.0 < float(vol.tsdf.max())
    assert (float(vol.color.max()) > 0.0) == with_image
    assert bool((vol.tsdf[n:] == 1).all()) and bool((vol.weight[n:] == 0).all())      # the pool past the count


# ---- D: extraction ---------------------------------------------------------------------------------------------------
def sparse_of(planes, lo, bricks=None, origin=K.ORIGIN, voxel=K.VOXEL):
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    return SparseTSDFVolume.from_dense(origin, voxel, *planes, lo=lo, bricks=bricks, device=_dev())


def assert_mesh_equals_mirror(vol, planes, lo, bricks, origin=K.ORIGIN, voxel=K.VOXEL):
    from monogs_amd.sparse_tsdf import extract_mesh_bricks_numpy
    verts, faces, colors = vol.extract_mesh()
    torch.cuda.synchronize()
    assert np.array_equal(vol.bricks().cpu().numpy(), np.asarray(bricks, np.int32))
    rv, rf, rc = extract_mesh_bricks_numpy(bricks, *SC.brick_rows(planes, lo, bricks), origin, voxel, 1.0)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
    assert tuple(verts.shape) == rv.shape and tuple(faces.shape) == rf.shape
    assert same_bits(verts, rv) and same_bits(colors, rc)                       # key order, bit for bit
    f = faces.cpu().numpy()
    assert np.array_equal(K.canonical_faces(f), K.canonical_faces(rf))          # as a set
    assert np.array_equal(f, rf)                                                # brick, cell, tetrahedron, triangle order
    v2, f2, c2 = vol.extract_mesh()
    assert torch.equal(bits(v2), bits(verts)) and torch.equal(f2, faces) and torch.equal(bits(c2), bits(colors))
    return verts.cpu().numpy(), f


def test_extraction_of_a_sphere_on_a_brick_corner(built):
    from monogs_amd.mesh_topology import mesh_topology
    planes, lo = SC.corner_sphere(), SC.CORNER_LO
    bricks = SC.box_bricks(lo, SC.CORNER_DIMS)
    vol = sparse_of(planes, lo)
    v, f = assert_mesh_equals_mirror(vol, planes, lo, bricks)
    lat = (v.astype(np.float64) - np.asarray(K.ORIGIN)) / K.VOXEL - np.asarray(lo)
    K.assert_closed_sphere(lat, f, origin=(0, 0, 0), voxel=1.0, c=SC.CORNER_C, r=SC.CORNER_R)
    # every one of the eight bricks holds vertices: the surface crosses their faces, edges and the corner
    assert len(np.unique(np.floor(lat / 8).clip(0, 1).astype(int) @ np.array([1, 2, 4]))) == 8
    # to_dense gives the planes back
    origin, t, w, c = vol.to_dense()
    assert same_bits(t, planes[0]) and same_bits(w, planes[1]) and same_bits(c, planes[2])
    want = np.asarray(K.ORIGIN, np.float32) + np.asarray(lo, np.float32) * np.float32(K.VOXEL)
    assert np.array_equal(np.asarray(origin, np.float32), want)
    _, t2, w2, _ = vol.to_dense(lo=(lo[0] - 3, lo[1] + 2, lo[2] + 5), dims=(25, 9, 6))
    assert tuple(t2.shape) == (6, 9, 25) and same_bits(t2[:, :, 3:19], planes[0][5:11, 2:11, :16])
    assert bool((w2[:, :, :3] == 0).all()) and bool((t2[:, :, 19:] == 1).all())
    # one brick removed: a hole with a boundary, nothing non-manifold
    kept = np.delete(bricks, 5, axis=0)
    hole = sparse_of(planes, lo, bricks=kept)
    hv, hf = assert_mesh_equals_mirror(hole, planes, lo, kept)
    info = mesh_topology(torch.from_numpy(hf).to(_dev()), len(hv))
    assert info["boundary_edges"] > 0 and info["nonmanifold_edges"] == 0 and not info["closed"]
    assert 0 < len(hf) < len(f)
    # a single brick with every neighbour absent
    one = sparse_of(planes, lo, bricks=bricks[6:7])
    ov, of = assert_mesh_equals_mirror(one, planes, lo, bricks[6:7])
    assert len(ov) > 0 and len(of) > 0
    # one sign everywhere: empty tensors
    t, w, c = planes
    flat = sparse_of((np.abs(t) + np.float32(0.25), w, c), lo)
    ev, ef, ec = flat.extract_mesh()
    assert tuple(ev.shape) == (0, 3) and tuple(ef.shape) == (0, 3) and tuple(ec.shape) == (0, 3)
    assert ev.dtype == torch.float32 and ef.dtype == torch.int32
    # no brick at all
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    none = SparseTSDFVolume(K.ORIGIN, K.VOXEL, 8, device=_dev()).extract_mesh()
    assert tuple(none[0].shape) == (0, 3) and tuple(none[1].shape) == (0, 3)


# ---- E: against the dense volume -------------------------------------------------------------------------------------
def test_six_views_of_a_sphere_give_the_dense_volumes_mesh(built):
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    from monogs_amd.tsdf import TSDFVolume
    dev = _dev()
    dense = TSDFVolume(SC.SIX_ORIGIN, SC.SIX_VS, SC.SIX_DIMS, device=dev)
    sparse = SparseTSDFVolume(SC.SIX_ORIGIN, SC.SIX_VS, 400, device=dev)
    g = torch.Generator().manual_seed(11)
    for T, depth in SC.six_views():
        image = torch.rand(3, SC.H, SC.W, generator=g).to(dev)
        for vol in (dense, sparse):
            vol.integrate(depth.to(dev), T.to(dev), SC.FX, SC.FY, SC.CX, SC.CY, image=image)
    dv, df, dc = (t.cpu().numpy() for t in dense.extract_mesh())
    sv, sf, sc_ = (t.cpu().numpy() for t in sparse.extract_mesh())
    assert len(dv) > 1000 and len(df) > 1000
    assert np.array_equal(SC.vertex_set(sv, sc_), SC.vertex_set(dv, dc))        # positions and colours, bit for bit
    assert np.array_equal(SC.face_position_set(sv, sf), SC.face_position_set(dv, df))
    n = sparse.num_bricks
    _, ref_bricks, _ = SC.six_views_mirror()
    assert np.array_equal(sparse.bricks().cpu().numpy(), ref_bricks)
    assert n * 512 < dense.tsdf.numel() // 4 and sparse.dropped == 0
    # the planes agree wherever a brick is allocated
    _, t, w, c = sparse.to_dense(lo=(0, 0, 0), dims=SC.SIX_DIMS)
    held = w > 0
    assert same_bits(t[held], dense.tsdf[held]) and same_bits(w[held], dense.weight[held])
    assert same_bits(c[:, held], dense.color[:, held])


# ---- F: two trips of the scan ----------------------------------------------------------------------------------------
def test_extraction_past_one_trip_of_the_scan(built):
    planes, lo = SC.trip_sphere(), SC.TRIP_LO
    bricks = SC.box_bricks(lo, SC.TRIP_DIMS)
    assert len(bricks) == 648 > 512
    vol = sparse_of(planes, lo)
    v, f = assert_mesh_equals_mirror(vol, planes, lo, bricks)
    lat = (v.astype(np.float64) - np.asarray(K.ORIGIN)) / K.VOXEL - np.asarray(lo)
    K.assert_closed_sphere(lat, f, origin=(0, 0, 0), voxel=1.0, c=SC.TRIP_C, r=SC.TRIP_R)
    rows = SC.brick_rows(planes, lo, bricks)[0]
    inside = np.flatnonzero((rows < 0).any(1))
    assert inside[0] < 512 < inside[-1]                                         # the surface spans both trips


# ---- G: beyond the dense limit ---------------------------------------------------------------------------------------
def test_a_sphere_where_no_dense_volume_reaches(built):
    from monogs_amd.mesh_topology import mesh_topology
    from monogs_amd.tsdf import check_dims
    planes, lo = SC.far_sphere(), SC.FAR_LO
    with pytest.raises(ValueError):                 # the box from the lattice's origin to the sphere
        check_dims(tuple(max(abs(l), abs(l + d)) + 1 for l, d in zip(lo, SC.FAR_DIMS)))
    voxel = 0.005
    bricks = SC.box_bricks(lo, SC.FAR_DIMS)
    vol = sparse_of(planes, lo, voxel=voxel)
    v, f = assert_mesh_equals_mirror(vol, planes, lo, bricks, voxel=voxel)
    info = mesh_topology(torch.from_numpy(f).to(_dev()), len(v))
    assert info["closed"] and info["oriented"] and info["euler"] == 2 and info["boundary_edges"] == 0
    lat = (v.astype(np.float64) - np.asarray(K.ORIGIN)) / voxel
    dist = np.abs(np.linalg.norm(lat - np.asarray(SC.FAR_CENTRE), axis=1) - SC.FAR_R)
    assert dist.max() < 1.0, dist.max()


# ---- H: pipeline -----------------------------------------------------------------------------------------------------
def test_fuse_map_reconstruct_and_save_sparse(built, tmp_path):
    from scenes import wide_scene
    from monogs_amd import sparse_tsdf as ST
    from monogs_amd import tsdf as T
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.gaussian_renderer import render
    from monogs_amd.ply_io import read_mesh_ply
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, Pipe, ViewCamera
    from monogs_amd.slam_surrogate import reconstruct_mesh
    dev = _dev()
    sc = wide_scene()
    cam = sc.cam
    gm = GaussianParams(*(t.to(dev) for t in (sc.means3D, sc.log_scales, sc.rot, sc.opacity_logit, sc.features_dc)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    tau = torch.tensor([0.1, -0.05, 0.08, 0.03, -0.02, 0.01])
    cams = [ViewCamera(k, torch.zeros(3, cam.H, cam.W), SE3_exp(k * tau), cam.projmatrix_raw, fovx, fovy, cam.H, cam.W, dev)
            for k in range(3)]
    bg = torch.zeros(3, device=dev)
    vs, cap = 0.125, 4000
    sparse = dict(max_bricks=cap, origin=(0.03, -0.02, 0.01))
    vol = T.fuse_map(gm, cams, bg, vs, sparse=sparse)
    assert isinstance(vol, ST.SparseTSDFVolume) and vol.origin == sparse["origin"] and vol.max_bricks == cap
    # the mirrors, fed the same rendered planes
    bricks = np.zeros((0, 3), np.int32)
    ref = (torch.ones(cap, 512), torch.zeros(cap, 512), torch.zeros(3, cap, 512))
    for v in cams:
        with torch.no_grad():
            pkg = render(v, gm, Pipe, bg)
        a = (vol.origin, vs, vol.trunc, pkg["depth"].cpu(), v.T.cpu(), v.fx, v.fy, v.cx, v.cy)
        kw = dict(opacity=pkg["opacity"].cpu(), min_opacity=0.95, normalize=True)
        bricks, dropped, out = ST.allocate_bricks_torch(bricks, cap, *a, **kw)
        assert dropped == 0 and out == 0
        ST.integrate_bricks_torch(bricks, *ref, *a, image=pkg["render"].cpu(), max_weight=vol.max_weight, **kw)
    n = vol.num_bricks
    assert 0 < n == len(bricks) < cap and np.array_equal(vol.bricks().cpu().numpy(), bricks)
    for got, want, name in zip((vol.tsdf, vol.weight, vol.color), ref, ("tsdf", "weight", "color")):
        assert torch.equal(bits(got), bits(want)), name
    verts, faces, colors = vol.extract_mesh()
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    rv, rf, rc = ST.extract_mesh_bricks_numpy(bricks, *(t.numpy() for t in ref), vol.origin, vs, 1.0)
    assert same_bits(verts, rv) and same_bits(colors, rc) and np.array_equal(faces.cpu().numpy(), rf)
    # a run's result
    result = {"cameras": {k: v for k, v in enumerate(cams)}, "kf_ids": [0, 1, 2], "gaussians": gm}
    v2, f2, c2 = reconstruct_mesh(result, vs, sparse=sparse)
    assert torch.equal(bits(v2), bits(verts)) and torch.equal(f2, faces) and torch.equal(bits(c2), bits(colors))
    post = dict(clean=dict(keep_largest=1), smooth=dict(iterations=2), simplify=dict(factor=2))
    v3, f3, c3 = reconstruct_mesh(result, vs, sparse=sparse, **post)
    w3, g3, d3 = vol.extract_mesh(**post)
    assert 0 < f3.shape[0] < faces.shape[0]
    assert torch.equal(bits(v3), bits(w3)) and torch.equal(f3, g3) and torch.equal(bits(c3), bits(d3))
    sensor = {}
    for k, v in enumerate(cams):
        with torch.no_grad():
            pkg = render(v, gm, Pipe, bg)
        sensor[k] = torch.where(pkg["opacity"] >= 0.95, pkg["depth"] / pkg["opacity"], torch.zeros_like(pkg["depth"]))[0]
    v4, f4, c4 = reconstruct_mesh(result, vs, sensor_depth=sensor, sparse=sparse)
    assert torch.equal(bits(v4), bits(verts)) and torch.equal(f4, faces) and float(c4.abs().max()) == 0.0
    # default origin, default capacity
    v5, f5, _ = reconstruct_mesh(result, vs, sparse=True)
    assert v5.shape[0] > 0 and f5.shape[0] > 0
    # the file, next to the point cloud
    path = save_mesh(vol, str(tmp_path))
    assert path == str(tmp_path / "point_cloud" / "final" / "mesh.ply")
    pv, pf, _ = read_mesh_ply(path)
    assert torch.equal(bits(pv), bits(verts)) and torch.equal(pf, faces.cpu())
    path2 = save_mesh(gm, str(tmp_path / "b"), cameras=cams, voxel_size=vs, sparse=sparse)
    assert open(path2, "rb").read() == open(path, "rb").read()


@pytest.mark.parametrize("sensor_depth", [False, True])
def test_run_sequence_fuses_keyframes_into_a_callers_volume(built, sensor_depth):
    from monogs_amd import slam_surrogate as SS
    from monogs_amd.sparse_tsdf import SparseTSDFVolume
    dev = _dev()
    Hh, Ww, n = 120, 160, 3
    frames, cam, _ = SS.load_sequence(n, Ww, Hh, dev, world_gaussians=3000)
    if sensor_depth and any(f.depth is None for f in frames):
        pytest.fail("the synthetic sequence has no depth")
    kw = dict(sensor_depth=sensor_depth, kf_interval=1, init_iters=20, mapping_iters=5, first_order_iters=5,
              second_order_iters=0)
    plain = SS.run_sequence(frames, cam, dev, **kw)
    vol = SparseTSDFVolume((0.0, 0.0, 0.0), 0.1, 6000, device=dev)
    fused = SS.run_sequence(frames, cam, dev, mesh_volume=vol, mesh_every=2, **kw)
    torch.cuda.synchronize()
    assert "mesh_keyframes" not in plain and fused["mesh_keyframes"] == [0, 2] and fused["kf_ids"] == plain["kf_ids"]
    for k in range(n):
        assert torch.equal(bits(fused["cameras"][k].T), bits(plain["cameras"][k].T)), k       # the same trajectory
    st = vol.stats()
    print("run_sequence volume:", st)
    assert st["bricks"] > 0 and float(vol.weight[:st["bricks"]].max()) >= 1.0
    assert st["dropped"] == 0 and st["out_of_range"] == 0
    # (a map of 20 + 2 * 5 iterations need not hold a closed surface yet: the extraction only has to run on it)
    verts, faces, colors = vol.extract_mesh()
    print("run_sequence mesh:", tuple(verts.shape), tuple(faces.shape))
    assert verts.shape == colors.shape and (faces.shape[0] == 0 or int(faces.max()) < verts.shape[0])
