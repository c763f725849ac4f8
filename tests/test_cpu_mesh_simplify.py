"""Mesh simplification without a GPU: the NumPy mirror that defines the contract (monogs_amd/mesh_simplify.py) on the
24^3 test sphere and against an independent plain-Python statement, the restated hash functions, and the refusals of
the C-ABI entry points and of the Python drivers.

Measured here (mirror, the big sphere of mesh_clean_cases, 2292 vertices / 4580 faces, origin (0,0,0)):
    cell 1: 768 / 1532, cell 2: 190 / 376, cell 3: 88 / 172, cell 4: 54 / 104, all closed with chi = 2;
    largest radial error 0.047 voxel at cell 1 and 0.090 at cell 2 (0.056 for the input)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_simplify_cases as K

SPHERE_VF = {1: (768, 1532), 2: (190, 376), 3: (88, 172), 4: (54, 104)}


def _check_invariants(v, f, out, kw):
    """What holds for every output of the contract."""
    from monogs_amd import mesh_simplify as MS
    ov, of, oc, info = out
    V2, F2 = ov.shape[0], of.shape[0]
    assert tuple(info) == MS.INFO_KEYS
    assert (info["verts_in"], info["faces_in"], info["verts_out"], info["faces_out"]) == (len(v), len(f), V2, F2)
    assert info["collapsed_faces"] + info["duplicate_faces"] + F2 == len(f)
    assert ov.dtype == np.float32 and of.dtype == np.int32 and of.shape == (F2, 3)
    if F2:
        assert of.min() >= 0 and of.max() < V2
        assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 0] != of[:, 2]).all()
        assert len(np.unique(np.sort(of, axis=1), axis=0)) == F2                 # no two faces share an index set
    assert np.array_equal(np.unique(of), np.arange(V2))                          # every vertex is named by a face
    assert V2 <= info["num_clusters"] <= len(v)


@pytest.mark.parametrize("factor", [1, 2, 3, 4])
def test_sphere_counts_closedness_and_cluster_radius(factor):
    from monogs_amd.mesh_simplify import simplify_mesh_numpy
    v, f, c = MC.floater_mesh(big_only=True)
    assert (v.shape[0], f.shape[0]) == MC.BIG_ONLY_VF
    kw = dict(cell=float(factor) * MC.FLOATER_VOXEL, origin=MC.FLOATER_ORIGIN)
    out = simplify_mesh_numpy(v, f, c, **kw)
    ov, of, oc, info = out
    _check_invariants(v, f, out, kw)
    assert (ov.shape[0], of.shape[0]) == SPHERE_VF[factor]
    edges, n = K.edge_counts(of)
    assert (n == 2).all()                                                        # every edge lies in exactly two faces
    assert ov.shape[0] - len(edges) + of.shape[0] == 2                           # chi = 2
    # every output vertex lies within sqrt(3) cell of every input vertex of its cluster; a colour mean inside [0, 1]
    cells = np.floor(v / np.float32(kw["cell"])).astype(np.int64)               # the origin is 0: t = v / cell
    _, first, inv = np.unique(cells, axis=0, return_index=True, return_inverse=True)
    assert info["num_clusters"] == len(first) == ov.shape[0]                     # a closed sphere: every cluster is named
    row = np.argsort(np.argsort(first))[inv.reshape(-1)]                         # clusters are emitted in ascending label
    dist = np.linalg.norm(ov[row].astype(np.float64) - v.astype(np.float64), axis=1)
    assert dist.max() <= np.sqrt(3.0) * kw["cell"]
    assert oc.shape == ov.shape and oc.min() >= 0.0 and oc.max() <= 1.0


@pytest.mark.parametrize("name", sorted(K.SMALL_CASES))
def test_mirror_agrees_with_the_plain_statement(name):
    from monogs_amd.mesh_simplify import _min_origin, simplify_mesh_numpy
    v, c, f, kw = K.SMALL_CASES[name]()
    out = simplify_mesh_numpy(v, f, c, **kw)
    _check_invariants(v, f, out, kw)
    origin = kw["origin"] if kw["origin"] is not None else (v.min(axis=0) if len(v) else np.zeros(3, np.float32))
    if kw["origin"] is None and len(v):
        assert np.array_equal(_min_origin(v), v.min(axis=0))
    pv, pf, pc, pinfo = K.plain_simplify(v, c, f, kw["cell"], origin)
    assert out[3] == pinfo
    assert np.array_equal(out[0].view(np.int32), pv.view(np.int32)) and np.array_equal(out[1], pf)
    assert (c is None and out[2] is None) or np.array_equal(out[2].view(np.int32), pc.view(np.int32))
    if name == "hand":
        assert out[3] == K.HAND_INFO
        assert out[1].tolist() == [[0, 1, 2], [3, 4, 5], [6, 2, 1], [5, 6, 0]]     # order and winding of the kept faces
        assert out[0][3].tolist() == [-0.25, 0.5, 0.5]                           # the mean of -0.5 and (fraction 1) -0.0
    if name in ("one_cell", "empty_v0", "empty_f0"):
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3)
    if name == "crowd":
        assert out[3]["verts_out"] == 3 and out[3]["faces_out"] == 1 and out[3]["duplicate_faces"] == 1


def test_mirror_on_the_large_strip():
    from monogs_amd.mesh_simplify import simplify_mesh_numpy
    v, c, f, kw = K.two_scan_trips()
    assert len(v) > 262144 + 256 and len(f) > 262144 + 256
    out = simplify_mesh_numpy(v, f, c, **kw)
    _check_invariants(v, f, out, kw)
    assert out[3]["faces_out"] == len(f) // 2 and out[3]["duplicate_faces"] == len(f) // 2
    assert out[3]["verts_out"] == len(v) // 2 == out[3]["num_clusters"]


def test_mirror_refuses_bad_input():
    from monogs_amd.mesh_simplify import simplify_keywords, simplify_mesh_numpy
    v, c, f, kw = K.hand()
    for cell in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError, match="cell"):
            simplify_mesh_numpy(v, f, c, cell=cell)
    with pytest.raises(ValueError, match="origin"):
        simplify_mesh_numpy(v, f, c, cell=1.0, origin=(0.0, float("nan"), 0.0))
    bad = v.copy()
    bad[3, 1] = np.nan
    bad[6, 0] = np.inf
    with pytest.raises(ValueError, match="2 of 13 vertices"):
        simplify_mesh_numpy(bad, f, c, **kw)
    with pytest.raises(ValueError, match="13 of 13 vertices"):
        simplify_mesh_numpy(v, f, c, cell=1e-9, origin=(-100.0, 0.0, 0.0))
    g = f.copy()
    g[2, 1], g[7, 0] = 13, -1
    with pytest.raises(ValueError, match=r"2 of 12 faces hold an index outside \[0, 13\)"):
        simplify_mesh_numpy(v, g, c, **kw)
    with pytest.raises(ValueError, match="not both"):
        simplify_keywords(dict(cell=1.0, factor=2), 0.5, (0, 0, 0))
    with pytest.raises(ValueError, match="cell or factor"):
        simplify_keywords(dict(), 0.5, (0, 0, 0))
    assert simplify_keywords(dict(factor=3), 0.5, (1, 2, 3)) == dict(cell=1.5, origin=(1.0, 2.0, 3.0))
    assert simplify_keywords(dict(cell=0.25, origin=(4, 5, 6)), 0.5, (1, 2, 3)) == dict(cell=0.25, origin=(4, 5, 6))


def test_home_slots_restate_the_tables():
    from monogs_amd import mesh_simplify as MS
    assert [MS.table_size(n) for n in (0, 1, 2, 3, 40, 64, 65, 262144)] == [1, 2, 4, 8, 128, 128, 256, 524288]
    assert MS.cell_key(-2 ** 20, -2 ** 20, -2 ** 20) == 0 and MS.cell_key(2 ** 20 - 1, 2 ** 20 - 1, 2 ** 20 - 1) == 2 ** 63 - 1
    for wrap in (False, True):
        _, cells, size, home = K.vertex_collisions(wrap)
        assert len(set(cells)) == 40 and {MS._home_slot(MS.cell_key(*cc), size) for cc in cells} == {home}
        _, triples, fsize, fhome = K.face_collisions(wrap)
        assert len(set(triples)) == 40 and {MS._home_slot_faces(t, fsize) for t in triples} == {fhome}
        assert (home == size - 1) == wrap and (fhome == fsize - 1) == wrap
    assert MS._home_slot_faces((3, 1, 2), 1 << 20) == MS._home_slot_faces((1, 2, 3), 1 << 20)
    slots = {MS._home_slot(MS.cell_key(x, 0, 0), 1 << 10) for x in range(512)}
    assert len(slots) > 256                                                      # neighbours along an axis are spread out


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_exports_and_struct_size(built):
    from monogs_amd import _cabi
    for n in ("mgs_mesh_simplify_args_size", "mgs_mesh_simplify_scratch_bytes", "mgs_mesh_simplify_count",
              "mgs_mesh_simplify_emit"):
        assert n in _cabi.EXPORTS, n
    L = _cabi.lib()
    assert L.mgs_mesh_simplify_args_size() == C.sizeof(_cabi.MeshSimplifyArgs) == 4 * 4 + 4 * 4 + 8 * 8 + 2 * 4
    assert L.mgs_abi_version() == _cabi.ABI_VERSION


def _fake_args(_cabi, fake=4096):
    a = _cabi.MeshSimplifyArgs()
    a.num_verts, a.num_faces, a.cell = 8, 4, 1.0
    a.verts = a.faces = a.scratch = a.counts = fake                      # never dereferenced on the host
    return a


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    fns = (L.mgs_mesh_simplify_count, L.mgs_mesh_simplify_emit)
    for fn in fns:
        assert fn(None, None) == -1
    for field in ("scratch", "faces", "verts"):
        a = _fake_args(_cabi)
        setattr(a, field, None)
        for fn in fns:
            assert fn(C.byref(a), None) == -1, field
    a = _fake_args(_cabi)
    a.counts = None
    assert L.mgs_mesh_simplify_count(C.byref(a), None) == -1
    for field in ("num_verts", "num_faces"):
        a = _fake_args(_cabi)
        setattr(a, field, -1)
        for fn in fns:
            assert fn(C.byref(a), None) == -1, field
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        a = _fake_args(_cabi)
        a.cell = cell
        for fn in fns:
            assert fn(C.byref(a), None) == -1, cell
    a = _fake_args(_cabi)
    a.origin[1] = float("nan")
    for fn in fns:
        assert fn(C.byref(a), None) == -1
    a.origin_from_verts = 1                                               # the given origin is then not looked at
    a.out_num_verts = a.out_num_faces = 0
    assert L.mgs_mesh_simplify_emit(C.byref(a), None) == 0                # nothing to write: no launch
    # emit: counts without outputs, counts beyond the input
    a = _fake_args(_cabi)
    a.out_num_verts, a.out_num_faces = 3, 1
    assert L.mgs_mesh_simplify_emit(C.byref(a), None) == -1
    a.out_verts = a.out_faces = 4096
    a.colors = 4096                                                       # colours without a place to put them
    assert L.mgs_mesh_simplify_emit(C.byref(a), None) == -1
    a.out_colors = 4096
    a.out_num_verts = 9
    assert L.mgs_mesh_simplify_emit(C.byref(a), None) == -1
    a.out_num_verts, a.out_num_faces = 0, 5
    assert L.mgs_mesh_simplify_emit(C.byref(a), None) == -1
    a.out_num_verts, a.out_num_faces = -1, 0
    assert L.mgs_mesh_simplify_emit(C.byref(a), None) == -1
    # sizes beyond 32-bit element indices
    big = (2 ** 31 - 1) // 3
    for nv, nf in ((big + 1, 4), (8, big + 1)):
        a = _fake_args(_cabi)
        a.num_verts, a.num_faces = nv, nf
        for fn in fns:
            assert fn(C.byref(a), None) == -3
        assert L.mgs_mesh_simplify_scratch_bytes(nv, nf) == 0
    assert L.mgs_mesh_simplify_scratch_bytes(-1, 4) == 0 and L.mgs_mesh_simplify_scratch_bytes(4, -1) == 0
    # the planes: box, keys, labels, counts, two sum planes, two flag planes, block totals, two tables
    pad = lambda b: (b + 255) // 256 * 256
    assert L.mgs_mesh_simplify_scratch_bytes(0, 0) == 256 + 2 * 256
    V, F = 4099, 700
    want = (256 + pad(8 * V) + 3 * pad(4 * V) + 2 * pad(24 * V) + pad(4 * F) + pad(16 * ((V + 255) // 256))
            + pad(4 * 16384) + pad(4 * 2048))
    assert L.mgs_mesh_simplify_scratch_bytes(V, F) == want
    assert L.mgs_mesh_simplify_scratch_bytes(big, big) > (8 + 12 + 48 + 8 + 4 + 8) * big


def test_drivers_raise_off_the_gpu_and_default_to_no_simplification():
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_simplify import simplify_mesh
    from monogs_amd.slam_surrogate import reconstruct_mesh
    from monogs_amd.tsdf import TSDFVolume
    v, c, f, kw = K.hand()
    with pytest.raises(RuntimeError, match="GPU only"):
        simplify_mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c), **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        simplify_mesh(v, f, cell=1.0)
    with pytest.raises(ValueError, match="cell"):
        simplify_mesh(torch.from_numpy(v), torch.from_numpy(f), cell=-1.0)
    with pytest.raises(TypeError):
        simplify_mesh(torch.from_numpy(v), torch.from_numpy(f))               # cell has no default
    for fn in (save_mesh, reconstruct_mesh, TSDFVolume.extract_mesh):
        assert inspect.signature(fn).parameters["simplify"].default is None, fn
