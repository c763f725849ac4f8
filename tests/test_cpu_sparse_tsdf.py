"""The sparse TSDF volume without a GPU: the mirrors that define its contract (monogs_amd/sparse_tsdf.py) against the dense
mirrors they restate, the allocation rules, the C-ABI boundary of the new entry points, and the defaults of the callers
up the stack (with sparse=None they make the calls they made before)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import sparse_tsdf_cases as SC
import tsdf_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1: integration --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_image", [False, True])
def test_brick_integration_equals_the_dense_mirror_on_the_allocated_bricks(with_image):
    from monogs_amd.tsdf import integrate_torch
    origin = SC.ORIGIN_POSITIVE
    steps = SC.mirror_run(SC.MAX_BRICKS, True, with_image, origin=origin)
    bricks, dropped, out, t, w, c = steps[-1]
    assert dropped == 0 and out == 0 and len(bricks) > 20 and bricks.min() >= 0
    nx, ny, nz = (int(8 * (v + 1)) for v in bricks.max(0))
    dense = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    depth, kw, image = SC.view_inputs(True, with_image)
    for T, vw, _ in SC.views():
        integrate_torch(*dense, origin, SC.VS, 4.0 * SC.VS, depth, T, SC.FX, SC.FY, SC.CX, SC.CY, image=image,
                        view_weight=vw, max_weight=SC.MAX_WEIGHT, **kw)
    want = SC.brick_rows([p.numpy() for p in dense], (0, 0, 0), bricks)
    B = len(bricks)
    for got, ref, name in zip((t, w, c), want, ("tsdf", "weight", "color")):
        got = got[..., :B, :].numpy()
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), name
    assert float(w.max()) == SC.MAX_WEIGHT and float(t[:B].min()) < 0.0
    # the pool past the list is untouched
    assert bool((t[B:] == 1).all()) and bool((w[B:] == 0).all()) and bool((c[:, B:] == 0).all())
    assert (float(c.max()) > 0.0) == with_image


# ---- 2: extraction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [(), (13,), (0, 5, 26)])
def test_brick_extraction_equals_the_dense_mirror_of_the_masked_planes(drop):
    from monogs_amd.sparse_tsdf import bricks_to_box, extract_mesh_bricks_numpy
    from monogs_amd.tsdf import extract_mesh_numpy
    dims = (22, 19, 17)
    planes = K.sphere_volume(dims)
    bricks = np.delete(SC.box_bricks((0, 0, 0), dims), list(drop), axis=0)
    rows = SC.brick_rows(planes, (0, 0, 0), bricks)
    verts, faces, colors = extract_mesh_bricks_numpy(bricks, *rows, K.ORIGIN, K.VOXEL, 1.0)
    lo, t, w, c, grid = bricks_to_box(bricks, *rows)
    assert tuple(lo) == (0, 0, 0) and int((grid < 0).sum()) == len(drop)
    rv, rf, rc = extract_mesh_numpy(t, w, c, K.ORIGIN, K.VOXEL, 1.0)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and len(verts) > 0
    assert np.array_equal(SC.vertex_set(verts, colors), SC.vertex_set(rv, rc))
    assert np.array_equal(SC.face_position_set(verts, faces), SC.face_position_set(rv, rf))
    if not drop:
        # nothing masked: the mesh of the dense planes themselves (the box only adds points without weight)
        dv, df, dc = extract_mesh_numpy(*planes, K.ORIGIN, K.VOXEL, 1.0)
        assert np.array_equal(SC.vertex_set(verts, colors), SC.vertex_set(dv, dc))
        assert np.array_equal(SC.face_position_set(verts, faces), SC.face_position_set(dv, df))
        K.assert_closed_sphere(verts, faces)
    else:
        directed, undirected = K.edge_counts(faces, len(verts))
        assert set(undirected.tolist()) == {1, 2} and set(directed.tolist()) == {1}


def test_brick_extraction_order_and_empty_cases():
    from monogs_amd.sparse_tsdf import extract_mesh_bricks_numpy
    planes = SC.corner_sphere()
    bricks = SC.box_bricks(SC.CORNER_LO, SC.CORNER_DIMS)
    assert bricks.min() < 0 < bricks.max() and len(bricks) == 8
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    a = extract_mesh_bricks_numpy(bricks, *SC.brick_rows(planes, SC.CORNER_LO, bricks), K.ORIGIN, K.VOXEL)
    b = extract_mesh_bricks_numpy(bricks[perm], *SC.brick_rows(planes, SC.CORNER_LO, bricks[perm]), K.ORIGIN, K.VOXEL)
    # the brick order changes the order of the mesh, not the mesh
    assert np.array_equal(SC.vertex_set(a[0], a[2]), SC.vertex_set(b[0], b[2]))
    assert np.array_equal(SC.face_position_set(a[0], a[1]), SC.face_position_set(b[0], b[1]))
    assert not np.array_equal(a[0], b[0])
    lat = (a[0].astype(np.float64) - np.asarray(K.ORIGIN)) / K.VOXEL - np.asarray(SC.CORNER_LO)
    K.assert_closed_sphere(lat, a[1], origin=(0, 0, 0), voxel=1.0, c=SC.CORNER_C, r=SC.CORNER_R)
    # ascending key order: the owners' bricks never go back (a vertex lies at most one point past its owner's brick)
    owner = np.floor((lat - 1e-3) / 8).astype(np.int64)
    ids = {tuple(b - np.asarray(SC.CORNER_LO) // 8): n for n, b in enumerate(bricks)}
    low = np.array([min(ids[tuple(np.clip(o - d, 0, 1))] for d in np.ndindex(2, 2, 2)) for o in owner])
    assert (np.maximum.accumulate(low) <= np.array([ids[tuple(np.clip(o, 0, 1))] for o in owner])).all()
    # a single brick with every neighbour absent: an open patch; one sign: nothing
    first = SC.brick_rows(planes, SC.CORNER_LO, bricks[:1])
    one = extract_mesh_bricks_numpy(bricks[:1], *first, K.ORIGIN, K.VOXEL)
    assert len(one[0]) > 0 and len(one[1]) > 0 and 1 in K.edge_counts(one[1], len(one[0]))[1]
    t, w, c = first
    e = extract_mesh_bricks_numpy(bricks[:1], np.abs(t) + np.float32(0.25), w, c, K.ORIGIN, K.VOXEL)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0, 3)
    e = extract_mesh_bricks_numpy(np.zeros((0, 3), np.int32), t[:0], w[:0], c[:, :0], K.ORIGIN, K.VOXEL)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)


# ---- 3: allocation ---------------------------------------------------------------------------------------------------
def test_allocation_order_duplicates_range_and_capacity():
    from monogs_amd import sparse_tsdf as ST
    assert ST.samples_of(0.2, 0.05) == 3 and ST.samples_of(0.3, 0.05) == 4 and ST.samples_of(0.01, 0.05) == 2
    depth, kw, _ = SC.view_inputs(True, False)
    T0, T1, T2 = (v[0] for v in SC.views()[:3])
    args = (SC.ORIGIN, SC.VS, 4.0 * SC.VS, depth)
    cam = (SC.FX, SC.FY, SC.CX, SC.CY)
    none = np.zeros((0, 3), np.int32)
    b0, dropped, out = ST.allocate_bricks_torch(none, 1000, *args, T0, *cam, **kw)
    assert b0.dtype == np.int32 and dropped == 0 and out == 0 and 20 < len(b0) < 300
    assert len(np.unique(ST.brick_keys(b0))) == len(b0)
    assert (b0.min(0) < 0).all() and (b0.max(0) >= 0).all()                  # both signs on every axis
    # order of the first candidate: pixel-major, so the list starts with what the first valid pixel asks for
    d = depth / kw["opacity"]
    p0 = int(torch.nonzero(((d > 0) & (d <= 2.5) & ~(kw["opacity"] < 0.95)).view(-1))[0])
    first_pixel_only = torch.zeros_like(depth)
    first_pixel_only.view(-1)[p0] = depth.view(-1)[p0]
    b_first, _, _ = ST.allocate_bricks_torch(none, 1000, *args[:3], first_pixel_only, T0, *cam, **kw)
    assert 1 <= len(b_first) <= 24 and np.array_equal(b0[:len(b_first)], b_first)
    # the same view again adds nothing; an overlapping one only new bricks, behind the old ones
    again, _, _ = ST.allocate_bricks_torch(b0, 1000, *args, T0, *cam, **kw)
    assert np.array_equal(again, b0)
    b1, _, _ = ST.allocate_bricks_torch(b0, 1000, *args, T1, *cam, **kw)
    assert len(b1) > len(b0) and np.array_equal(b1[:len(b0)], b0) and len(np.unique(ST.brick_keys(b1))) == len(b1)
    # a camera that faces away into empty space (no depth anywhere) adds none
    b2, _, _ = ST.allocate_bricks_torch(b1, 1000, *args[:3], torch.zeros(SC.H, SC.W), T2, *cam, **SC.VIEW_KW)
    assert np.array_equal(b2, b1)
    # capacity: the kept bricks are the first ones, the rest is counted
    cap = len(b0) - 7
    bc, dropped, _ = ST.allocate_bricks_torch(none, cap, *args, T0, *cam, **kw)
    assert dropped == 7 and np.array_equal(bc, b0[:cap])
    bc2, dropped2, _ = ST.allocate_bricks_torch(bc, cap, *args, T0, *cam, **kw)
    assert dropped2 == 7 and np.array_equal(bc2, bc)                        # asked for again, dropped again
    # the coordinate range: a lattice so fine that the surface, 11 away from the origin, lies past 2^20 bricks
    tiny = 1.0e-6
    assert 11.0 / (8 * tiny) > 2 ** 20
    br, dropped, out = ST.allocate_bricks_torch(none, 1000, (0.0, 0.0, -10.0), tiny, 4 * tiny, depth, T0, *cam, **kw)
    valid = int(((depth / kw["opacity"] > 0) & (depth / kw["opacity"] <= 2.5) & ~(kw["opacity"] < 0.95)).sum())
    assert len(br) == 0 and dropped == 0 and out == valid * 3 * 8
    # what the integration skips allocates nothing
    for bad in (torch.zeros(SC.H, SC.W), torch.full((SC.H, SC.W), float("nan")), torch.full((SC.H, SC.W), 3.0)):
        bb, _, out = ST.allocate_bricks_torch(none, 10, *args[:3], bad, T0, *cam, depth_max=2.5)
        assert len(bb) == 0 and out == 0
    bb, _, _ = ST.allocate_bricks_torch(none, 10, *args[:3], torch.full((SC.H, SC.W), 1.5), T0, *cam,
                                        opacity=torch.full((SC.H, SC.W), 0.5))
    assert len(bb) == 0


def test_allocation_covers_every_point_the_integration_updates_inside_the_band():
    """The point of the sampling rule: a lattice point the dense integration gives |tsdf| < 1 lies in an allocated brick."""
    from monogs_amd import sparse_tsdf as ST
    from monogs_amd.tsdf import integrate_torch
    origin = SC.ORIGIN_POSITIVE
    depth, kw, _ = SC.view_inputs(True, False)
    T0 = SC.views()[0][0]
    bricks, _, _ = ST.allocate_bricks_torch(np.zeros((0, 3), np.int32), 1000, origin, SC.VS, 4 * SC.VS, depth, T0,
                                            SC.FX, SC.FY, SC.CX, SC.CY, **kw)
    nx, ny, nz = (int(8 * (v + 1)) for v in bricks.max(0))
    assert bricks.min() >= 0
    dense = (torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(3, nz, ny, nx))
    integrate_torch(*dense, origin, SC.VS, 4 * SC.VS, depth, T0, SC.FX, SC.FY, SC.CX, SC.CY, **kw)
    k, j, i = np.nonzero((dense[1].numpy() > 0) & (np.abs(dense[0].numpy()) < 1))
    assert len(i) > 1000
    need = np.unique(ST.brick_keys(np.stack([i // 8, j // 8, k // 8], 1)))
    assert np.isin(need, ST.brick_keys(bricks)).all()


# ---- 4: tables -------------------------------------------------------------------------------------------------------
def test_tet_table_is_the_one_in_the_kernel_source():
    from monogs_amd import tsdf as T
    src = open(os.path.join(ROOT, "monogs_amd", "csrc", "sparse_tsdf.hip")).read()
    block = src[src.index("TET_TABLE_BEGIN"):src.index("TET_TABLE_END")]
    ntri = [int(v) for v in re.search(r"c_tet_ntri\[16\] = \{([^}]*)\}", block).group(1).split(",")]
    body = block[block.index("c_tet_tri[16][6]"):]
    rows = [[int(v) for v in m.split(",")] for m in re.findall(r"\{([0-9, ]+)\}", body)]
    table = T._tet_table()
    assert len(rows) == 16 and ntri == [len(t) for t in table]
    for case, tris in enumerate(table):
        flat = [e for tri in tris for e in tri]
        assert rows[case][:len(flat)] == flat, case
    # the other constant tables are the dense file's, word for word
    dense = open(os.path.join(ROOT, "monogs_amd", "csrc", "tsdf.hip")).read()
    for name in ("c_slot_of[8]", "c_slot_code[7]", "c_tet[6][4]", "c_tet_flip[6]", "c_tet_edge[6][2]"):
        grab = lambda s: re.sub(r"\s+", " ", s[s.index(name):s.index(";", s.index(name))])
        assert grab(src) == grab(dense), name


# ---- 5: C ABI --------------------------------------------------------------------------------------------------------
NAMES = ("mgs_sparse_tsdf_volume_size", "mgs_sparse_tsdf_view_args_size", "mgs_sparse_tsdf_mesh_args_size",
         "mgs_sparse_tsdf_table_size", "mgs_sparse_tsdf_allocate_scratch_bytes", "mgs_sparse_tsdf_allocate",
         "mgs_sparse_tsdf_integrate", "mgs_sparse_tsdf_register", "mgs_sparse_tsdf_mesh_scratch_bytes",
         "mgs_sparse_tsdf_mesh_count", "mgs_sparse_tsdf_mesh_emit")


def test_exports_struct_sizes_and_limits(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n), n
    assert L.mgs_sparse_tsdf_volume_size() == C.sizeof(_cabi.SparseTsdfVolume) == 6 * 4 + 7 * 8
    assert L.mgs_sparse_tsdf_view_args_size() == C.sizeof(_cabi.SparseTsdfViewArgs) == 80 + 16 * 4 + 5 * 8
    assert L.mgs_sparse_tsdf_mesh_args_size() == C.sizeof(_cabi.SparseTsdfMeshArgs) == 80 + 2 * 4 + 5 * 8 + 2 * 4
    header = open(os.path.join(ROOT, "include", "monogs_raster.h"), encoding="utf-8").read()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
    cap = _cabi.SPARSE_TSDF_MAX_BRICKS
    assert cap == 599186 and 7 * 512 * cap < 2 ** 31 <= 7 * 512 * (cap + 1)
    assert L.mgs_sparse_tsdf_table_size(0) == 0 and L.mgs_sparse_tsdf_table_size(cap + 1) == 0
    assert [L.mgs_sparse_tsdf_table_size(n) for n in (1, 2, 3, 512, 513, cap)] == [2, 4, 8, 1024, 2048, 2 ** 21]
    # scratch arithmetic: planes padded to 256 bytes, in the order of the file
    pad = lambda b: (b + 255) // 256 * 256
    n = 70 * 45 * 8 * 3
    table = 1 << (2 * n - 1).bit_length()
    assert L.mgs_sparse_tsdf_allocate_scratch_bytes(70, 45, 3) == (pad(8 * n) + pad(4 * table) + pad(2 * n)
                                                                   + pad(8 * ((n + 255) // 256)) + 256)
    assert L.mgs_sparse_tsdf_allocate_scratch_bytes(0, 45, 3) == 0 and L.mgs_sparse_tsdf_allocate_scratch_bytes(70, 45, 0) == 0
    assert L.mgs_sparse_tsdf_allocate_scratch_bytes(20000, 20000, 3) == 0         # 8 * 3 * 4e8 candidates >= 2^31
    assert L.mgs_sparse_tsdf_mesh_scratch_bytes(0) == 0 and L.mgs_sparse_tsdf_mesh_scratch_bytes(cap + 1) == 0
    assert L.mgs_sparse_tsdf_mesh_scratch_bytes(5) == pad(4 * 27 * 5) + 3 * pad(2 * 512 * 5) + pad(8 * 10)


def _volume(v, cap=4):
    v.max_bricks, v.voxel_size = cap, 0.05
    v.tsdf = v.weight = v.color = v.brick_coords = v.map_keys = v.map_vals = v.state = 4096


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    for fn in (L.mgs_sparse_tsdf_allocate, L.mgs_sparse_tsdf_integrate, L.mgs_sparse_tsdf_mesh_count,
               L.mgs_sparse_tsdf_mesh_emit):
        assert fn(None, None) == -1
    assert L.mgs_sparse_tsdf_register(None, 0, 1, None) == -1

    def view():
        a = _cabi.SparseTsdfViewArgs()
        _volume(a.vol)
        a.width, a.height, a.samples = 16, 16, 3
        a.trunc, a.fx, a.fy, a.view_weight, a.max_weight = 0.2, 10.0, 10.0, 1.0, 64.0
        a.T = a.depth = a.scratch = 4096
        return a

    def broken(**kw):
        a = view()
        for k, v in kw.items():
            obj, _, name = k.rpartition("__")
            setattr(a.vol if obj == "vol" else a, name, v)
        return a

    for both in (dict(vol__max_bricks=0), dict(vol__voxel_size=0.0), dict(vol__tsdf=None), dict(vol__weight=None),
                 dict(vol__brick_coords=None), dict(vol__map_keys=None), dict(vol__map_vals=None), dict(vol__state=None),
                 dict(width=0), dict(height=-1), dict(trunc=0.0), dict(fx=0.0), dict(fy=float("nan")), dict(T=None),
                 dict(depth=None)):
        a = broken(**both)
        assert L.mgs_sparse_tsdf_allocate(C.byref(a), None) == -1, both
        assert L.mgs_sparse_tsdf_integrate(C.byref(a), None) == -1, both
    for only in (dict(samples=0), dict(scratch=None)):
        assert L.mgs_sparse_tsdf_allocate(C.byref(broken(**only)), None) == -1, only
    for only in (dict(view_weight=0.0), dict(max_weight=0.0), dict(image=4096, vol__color=None)):
        assert L.mgs_sparse_tsdf_integrate(C.byref(broken(**only)), None) == -1, only
    big = broken(vol__max_bricks=_cabi.SPARSE_TSDF_MAX_BRICKS + 1)
    assert L.mgs_sparse_tsdf_allocate(C.byref(big), None) == -3 and L.mgs_sparse_tsdf_integrate(C.byref(big), None) == -3
    assert L.mgs_sparse_tsdf_allocate(C.byref(broken(width=20000, height=20000)), None) == -3
    v = _cabi.SparseTsdfVolume()
    _volume(v)
    for first, count in ((-1, 1), (0, 0), (0, 5), (4, 1), (5, 0)):
        assert L.mgs_sparse_tsdf_register(C.byref(v), first, count, None) == -1, (first, count)

    def mesh(**kw):
        m = _cabi.SparseTsdfMeshArgs()
        _volume(m.vol)
        m.num_bricks, m.min_weight = 2, 1.0
        m.scratch = m.counts = 4096
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    for bad in (dict(num_bricks=0), dict(num_bricks=5), dict(scratch=None)):
        assert L.mgs_sparse_tsdf_mesh_count(C.byref(mesh(**bad)), None) == -1, bad
        assert L.mgs_sparse_tsdf_mesh_emit(C.byref(mesh(**bad)), None) == -1, bad
    assert L.mgs_sparse_tsdf_mesh_count(C.byref(mesh(counts=None)), None) == -1
    assert L.mgs_sparse_tsdf_mesh_emit(C.byref(mesh(num_verts=-1)), None) == -1
    assert L.mgs_sparse_tsdf_mesh_emit(C.byref(mesh(num_verts=3, num_faces=1)), None) == -1      # counts without outputs
    assert L.mgs_sparse_tsdf_mesh_emit(C.byref(mesh(num_verts=2 ** 31 - 1)), None) == -3
    assert L.mgs_sparse_tsdf_mesh_emit(C.byref(mesh()), None) == 0                               # nothing to write: no launch
    m = mesh()
    m.vol.tsdf = None
    assert L.mgs_sparse_tsdf_mesh_count(C.byref(m), None) == -1 and L.mgs_sparse_tsdf_mesh_emit(C.byref(m), None) == -1


# ---- 6: defaults -----------------------------------------------------------------------------------------------------
def test_the_volume_raises_off_the_gpu_like_the_dense_one():
    from monogs_amd.sparse_tsdf import MAX_BRICKS, SparseTSDFVolume, check_max_bricks
    assert check_max_bricks(MAX_BRICKS) == MAX_BRICKS
    with pytest.raises(ValueError):
        check_max_bricks(MAX_BRICKS + 1)
    with pytest.raises(ValueError):
        SparseTSDFVolume((0, 0, 0), 0.01, MAX_BRICKS + 1, device="cpu")
    with pytest.raises(ValueError):
        SparseTSDFVolume((0, 0, 0), 0.01, 0, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        SparseTSDFVolume((0, 0, 0), 0.01, 16, device="cpu")


class _Spy:
    """Stands in for tsdf.TSDFVolume and records every call made to it."""
    log = []

    def __init__(self, *a, **kw):
        _Spy.log.append(("__init__", a, kw))

    @classmethod
    def for_map(cls, *a, **kw):
        _Spy.log.append(("for_map", a, kw))
        return cls.__new__(cls)

    def integrate_view(self, *a, **kw):
        _Spy.log.append(("integrate_view", a, kw))

    def integrate(self, *a, **kw):
        _Spy.log.append(("integrate", a, kw))

    def extract_mesh(self, *a, **kw):
        _Spy.log.append(("extract_mesh", a, kw))
        return torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32), torch.zeros(3, 3)


class _Cam:
    T, fx, fy, cx, cy = "T", 1.0, 2.0, 3.0, 4.0
    original_image = None


class _Map:
    get_xyz = torch.zeros(4, 3)


def test_with_sparse_none_the_callers_make_the_calls_they_made(monkeypatch, tmp_path):
    import monogs_amd.sparse_tsdf  # noqa: F401  (imported before TSDFVolume is replaced)
    from monogs_amd import tsdf
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.slam_surrogate import reconstruct_mesh
    monkeypatch.setattr(tsdf, "TSDFVolume", _Spy)
    gm, cams, bg = _Map(), [_Cam(), _Cam()], "bg"

    def calls():
        out, _Spy.log = _Spy.log, []
        return out

    view = lambda c, mode="mean": ("integrate_view", (gm, c, bg), dict(min_opacity=0.95, depth_max=math.inf, depth_mode=mode))
    # fuse_map
    vol = tsdf.fuse_map(gm, cams, bg, 0.05)
    assert isinstance(vol, _Spy)
    assert calls() == [("for_map", (gm, 0.05, 0.1), dict(trunc=None, max_weight=64.0)), view(cams[0]), view(cams[1])]
    tsdf.fuse_map(gm, cams[:1], bg, 0.05, margin=0.3, trunc=0.2, max_weight=8.0, depth_mode="median", sparse=None)
    assert calls() == [("for_map", (gm, 0.05, 0.3), dict(trunc=0.2, max_weight=8.0)), view(cams[0], "median")]
    tsdf.fuse_map(gm, cams[:1], bg, 0.05, volume=vol, sparse=False)
    assert calls() == [view(cams[0])]
    # reconstruct_mesh: its four extract_mesh spellings and the sensor-depth branch
    result = {"gaussians": gm, "kf_ids": [0, 1], "cameras": {0: cams[0], 1: cams[1]}}
    for kw, want in ((dict(), ((1.0,), {})), (dict(clean=dict(keep_largest=1)), ((1.0,), dict(clean=dict(keep_largest=1)))),
                     (dict(simplify=dict(factor=2)), ((1.0,), dict(clean=None, simplify=dict(factor=2)))),
                     (dict(smooth=dict(iterations=2)), ((1.0,), dict(clean=None, simplify=None, smooth=dict(iterations=2))))):
        reconstruct_mesh(result, 0.05, **kw)
        log = calls()
        assert log[0] == ("for_map", (gm, 0.05, 0.1), dict(trunc=None, max_weight=64.0))
        assert [c[0] for c in log[1:3]] == ["integrate_view"] * 2 and log[1][1][0] is gm
        assert torch.equal(log[1][1][2], torch.zeros(3)) and log[1][2] == view(cams[0])[2]
        assert log[3] == ("extract_mesh",) + want and len(log) == 4
    reconstruct_mesh(result, 0.05, sensor_depth={0: "d0", 1: "d1"}, margin=0.2, depth_max=3.0, sparse=None)
    assert calls() == [("for_map", (gm, 0.05, 0.2), dict(trunc=None, max_weight=64.0)),
                       ("integrate", ("d0", "T", 1.0, 2.0, 3.0, 4.0), dict(image=None, depth_max=3.0)),
                       ("integrate", ("d1", "T", 1.0, 2.0, 3.0, 4.0), dict(image=None, depth_max=3.0)),
                       ("extract_mesh", (1.0,), {})]
    # save_mesh
    path = save_mesh(gm, str(tmp_path), cameras=cams[:1], background=bg, voxel_size=0.05, margin=0.2)
    assert path.endswith("mesh.ply") and os.path.exists(path)
    assert calls() == [("for_map", (gm, 0.05, 0.2), dict(trunc=None, max_weight=64.0)), view(cams[0]),
                       ("extract_mesh", (1.0,), {})]
    save_mesh(_Spy.__new__(_Spy), str(tmp_path), clean=dict(min_faces=1), sparse=None)
    assert calls() == [("extract_mesh", (1.0,), dict(clean=dict(min_faces=1)))]


def test_run_sequence_takes_a_mesh_volume_and_defaults_to_none():
    import inspect
    from monogs_amd.slam_surrogate import reconstruct_mesh, run_sequence
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.tsdf import fuse_map
    p = inspect.signature(run_sequence).parameters
    assert p["mesh_volume"].default is None and p["mesh_every"].default == 1
    for fn in (fuse_map, reconstruct_mesh, save_mesh):
        assert inspect.signature(fn).parameters["sparse"].default is None


# ---- 7: the dense-equality scene ---------------------------------------------------------------------------------------
def test_six_view_sphere_masked_by_its_bricks_is_the_dense_mesh():
    """The condition GPU test E rests on, with mirrors only: in this scene (sphere of 10 voxels seen from 1.5 m, trunc
    4 voxels) the dense volume's mesh lies wholly in allocated bricks, so masking the dense planes by the brick list
    changes nothing, and the brick mirror gives that mesh."""
    from monogs_amd.sparse_tsdf import extract_mesh_bricks_numpy
    from monogs_amd.tsdf import extract_mesh_numpy
    dense, bricks, rows = SC.six_views_mirror()
    nx, ny, nz = SC.SIX_DIMS
    assert bricks.min() >= 0 and (bricks.max(0) < np.array([nx, ny, nz]) // 8).all()
    assert len(bricks) * 512 < nx * ny * nz // 4
    dv, df, dc = extract_mesh_numpy(*(p.numpy() for p in dense), SC.SIX_ORIGIN, SC.SIX_VS, 1.0)
    mask = np.zeros((nz // 8, ny // 8, nx // 8), bool)
    mask[bricks[:, 2], bricks[:, 1], bricks[:, 0]] = True
    mask = mask.repeat(8, 0).repeat(8, 1).repeat(8, 2)
    t, w, c = (p.numpy().copy() for p in dense)
    t[~mask], w[~mask], c[:, ~mask] = 1.0, 0.0, 0.0
    mv, mf, mc = extract_mesh_numpy(t, w, c, SC.SIX_ORIGIN, SC.SIX_VS, 1.0)
    assert len(dv) > 1000 and np.array_equal(SC.vertex_set(mv, mc), SC.vertex_set(dv, dc))
    assert np.array_equal(SC.face_position_set(mv, mf), SC.face_position_set(dv, df))
    # the brick planes are the dense planes on the bricks, and their mesh is that mesh
    want = SC.brick_rows([p.numpy() for p in dense], (0, 0, 0), bricks)
    B = len(bricks)
    for got, ref in zip(rows, want):
        assert np.array_equal(got[..., :B, :].numpy().view(np.int32), ref.view(np.int32))
    sv, sf, sc_ = extract_mesh_bricks_numpy(bricks, *(r.numpy() for r in rows), SC.SIX_ORIGIN, SC.SIX_VS, 1.0)
    assert np.array_equal(SC.vertex_set(sv, sc_), SC.vertex_set(dv, dc))
    assert np.array_equal(SC.face_position_set(sv, sf), SC.face_position_set(dv, df))
    dist = np.abs(np.linalg.norm(sv.astype(np.float64) - np.asarray(SC.SIX_CENTRE), axis=1) - SC.SIX_RADIUS)
    print("six views: bricks", B, "verts", len(sv), "faces", len(sf), "max |r - R| / voxel", dist.max() / SC.SIX_VS)
    # a sign change needs a view that saw the point inside its band: no vertex is farther than trunc from the sphere
    assert dist.max() < 4 * SC.SIX_VS
