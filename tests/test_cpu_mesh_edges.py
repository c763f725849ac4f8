"""The contracts of monogs_amd/mesh_topology.py and monogs_amd/mesh_smooth.py on their NumPy mirrors (no GPU): known
meshes, an independent plain-Python statement, smoothing as numbers, the refusals of the mirrors and of the C entry
points, the restated home slot, and the ABI.

Sizes: mesh_edges_cases.py lists the block, scan-trip and hash-table boundaries and the case that crosses each."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_edges_cases as EC
import mesh_simplify_cases as K
from monogs_amd import mesh_smooth as SM
from monogs_amd import mesh_topology as MT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_the_sphere_is_closed_and_oriented():
    v, f = EC.sphere()
    assert (len(v), len(f)) == MC.BIG_ONLY_VF
    edges, edge_faces, degree, flags, info = MT.mesh_edges_numpy(f, len(v))
    assert info["edges"] == 6870 == len(edges) and (edge_faces == 2).all() and info["inconsistent_edges"] == 0
    assert info["euler"] == 2 and info["closed"] and info["oriented"]
    assert tuple(info) == MT.INFO_KEYS
    assert info["boundary_edges"] + info["manifold_edges"] + info["nonmanifold_edges"] == info["edges"]
    assert (flags == 1).all() and degree.sum() == 2 * 6870
    uniq, n = K.edge_counts(f)                                      # the helper the simplifier's tests use
    assert {tuple(e) for e in edges.tolist()} == {tuple(e) for e in uniq.tolist()} and (n == 2).all()
    assert edges.dtype == edge_faces.dtype == degree.dtype == flags.dtype == np.int32


def test_the_floater_mesh_has_five_components():
    v, f = EC.floaters()
    assert (len(v), len(f)) == MC.FLOATER_VF
    info = MT.mesh_topology_numpy(f, len(v), components=True)
    assert info["edges"] == 7836 and info["euler"] == 10 and info["components"] == 5 and info["oriented"]
    assert tuple(info) == MT.INFO_KEYS + ("components",)
    assert "components" not in MT.mesh_topology_numpy(f, len(v))


def test_one_reversed_face():
    v, f = EC.reversed_face()
    info = MT.mesh_topology_numpy(f, len(v))
    assert info["inconsistent_edges"] == 3 and info["closed"] and not info["oriented"]


def test_the_upper_half_is_open_and_its_rim_is_pinned():
    v, f = EC.upper_half()
    assert len(f) == 2268
    _, _, degree, flags, info = MT.mesh_edges_numpy(f, len(v))
    assert info["boundary_edges"] == 110 and info["manifold_edges"] == 3347 and not info["closed"]
    out, sinfo = SM.smooth_mesh_numpy(v, f, boundary="pin")
    still = (degree == 0) | (flags & 2 != 0)
    assert still.sum() == 110 + (len(v) - info["referenced_verts"])
    assert np.array_equal(bits(out)[still], bits(v)[still]) and (bits(out)[~still] != bits(v)[~still]).any(axis=1).all()
    assert sinfo["pinned_verts"] == 110 and sinfo["steps"] == 20 and sinfo["iterations"] == 10
    free, finfo = SM.smooth_mesh_numpy(v, f, boundary="free")
    rim = flags & 2 != 0
    assert (bits(free)[rim] != bits(v)[rim]).any(axis=1).all() and finfo["pinned_verts"] == 0
    assert np.array_equal(bits(free)[degree == 0], bits(v)[degree == 0])
    assert tuple(sinfo) == SM.INFO_KEYS


def test_star_and_three_faces_on_one_edge():
    v, f = EC.star()
    _, edge_faces, degree, _, info = MT.mesh_edges_numpy(f, len(v))
    assert info["edges"] == 9000 == info["boundary_edges"] and degree.max() == 6000 == degree[7]
    v, f = EC.three_on_an_edge()
    edges, edge_faces, _, flags, info = MT.mesh_edges_numpy(f, len(v))
    assert info["nonmanifold_edges"] == 1 and edges[0].tolist() == [0, 1] and edge_faces[0] == 3
    assert info["boundary_edges"] == 6 and (flags == 3).all()


@pytest.mark.parametrize("name", ["hand", "random_3", "random_7", "random_50", "random_300", "three_on_an_edge",
                                  "edge_home", "edge_wrap", "empty_v0", "empty_f0", "one_face"])
def test_mirrors_equal_the_plain_statement_bit_for_bit(name):
    v, f = EC.SMALL_CASES[name]()
    want = EC.plain_edges(f, len(v))
    got = MT.mesh_edges_numpy(f, len(v))
    for a, b in zip(got[:4], want[:4]):
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)
    assert got[4] == want[4]
    if name == "hand":
        assert got[4] == EC.HAND_INFO
    for kw in (dict(iterations=3, lam=0.5, mu=-0.53, boundary="pin"), dict(iterations=2, lam=0.25, mu=None, boundary="free"),
               dict(iterations=1, lam=1.0, mu=-1.0, boundary="free")):
        out, info = SM.smooth_mesh_numpy(v, f, **kw)
        assert out.dtype == np.float32 and out.shape == v.shape
        assert np.array_equal(bits(out), bits(EC.plain_smooth(v, f, **kw))), kw
        assert {k: info[k] for k in MT.INFO_KEYS} == want[4]


def test_long_rows():
    """The rows at which the device changes from a lane to a workgroup: the mirror on them against the plain statement."""
    v, f = EC.long_rows()
    _, _, degree, flags, info = MT.mesh_edges_numpy(f, len(v))
    assert {h: int(degree[h]) for h in EC.LONG_ROW_HUBS} == EC.LONG_ROW_HUBS and degree[3:300].max() == 0
    assert flags[301] == 1 and (flags[[0, 1, 2, 300]] == 3).all()     # only the closed fan's hub is off the boundary
    for kw in (dict(iterations=2, lam=0.5, mu=-0.53, boundary="free"), dict(iterations=1, lam=0.5, mu=None, boundary="pin")):
        out, sinfo = SM.smooth_mesh_numpy(v, f, **kw)
        assert np.array_equal(bits(out), bits(EC.plain_smooth(v, f, **kw)))
        moved = np.flatnonzero((bits(out) != bits(v)).any(axis=1))
        if kw["boundary"] == "pin":
            assert moved.tolist() == [301] and sinfo["pinned_verts"] == info["referenced_verts"] - 1
        else:
            assert set(EC.LONG_ROW_HUBS) <= set(moved.tolist())


def test_smoothing_as_numbers():
    noisy, f = EC.noisy_sphere()
    mean0, std0 = EC.radii(noisy)
    assert abs(mean0 - 6.3928) < 1e-3 and abs(std0 - 0.1507) < 1e-3
    taubin, _ = SM.smooth_mesh_numpy(noisy, f, iterations=10, lam=0.5, mu=-0.53)
    mean1, std1 = EC.radii(taubin)
    print("noisy", mean0, std0, "taubin", mean1, std1)
    assert std1 < 0.5 * std0 and abs(mean1 - mean0) < 0.01
    laplace, _ = SM.smooth_mesh_numpy(noisy, f, iterations=10, mu=None)
    mean2, _ = EC.radii(laplace)
    print("laplacian", mean2)
    assert mean0 - mean2 > 0.1                                       # the shrinkage Taubin exists to avoid
    same, info = SM.smooth_mesh_numpy(noisy, f, iterations=0)
    assert np.array_equal(bits(same), bits(noisy)) and info["steps"] == 0


def test_exponent_and_scale_do_not_change_the_bits_by_a_power_of_two():
    """E follows the input's largest coordinate, so scaling the mesh by 2^k scales the output by 2^k exactly."""
    v, f = EC.hand()
    out = SM.smooth_mesh_numpy(v, f, iterations=2, boundary="free")[0]
    for k in (-40, 7, 60):
        scaled = SM.smooth_mesh_numpy(np.ldexp(v, k), f, iterations=2, boundary="free")[0]
        assert np.array_equal(bits(scaled), bits(np.ldexp(out, k)))
    zeros = np.zeros((3, 3), np.float32)                             # E = -127
    assert np.array_equal(bits(SM.smooth_mesh_numpy(zeros, [[0, 1, 2]], boundary="free")[0]), bits(zeros))


def test_mirrors_refuse():
    v, f = EC.hand()
    g = f.copy()
    g[2, 1], g[7, 0] = 19, -1
    with pytest.raises(ValueError, match=r"mesh_edges: 2 of 13 faces hold an index outside \[0, 19\)"):
        MT.mesh_edges_numpy(g, 19)
    with pytest.raises(ValueError, match=r"mesh_topology: 2 of 13 faces"):
        MT.mesh_topology_numpy(g, 19)
    with pytest.raises(ValueError, match=r"smooth_mesh: 2 of 13 faces"):
        SM.smooth_mesh_numpy(v, g)
    with pytest.raises(ValueError, match="num_verts"):
        MT.mesh_edges_numpy(f, -1)
    bad = v.copy()
    bad[3, 1], bad[6, 0] = np.nan, np.inf
    with pytest.raises(ValueError, match="2 of 19 vertices are not finite"):
        SM.smooth_mesh_numpy(bad, f)
    for kw in (dict(lam=0.0), dict(lam=1.5), dict(lam=float("nan")), dict(mu=0.0), dict(mu=-1.5), dict(mu=0.3),
               dict(iterations=-1), dict(iterations=1001), dict(iterations=2.5), dict(boundary="clamp")):
        with pytest.raises(ValueError, match="smooth_mesh: " + next(iter(kw))):
            SM.smooth_mesh_numpy(v, f, **kw)
    SM.smooth_mesh_numpy(v, f, iterations=1000, lam=1.0, mu=-1.0)          # the ends that belong to the ranges


def test_home_slot_restated():
    """mix64 is MurmurHash3's finaliser; the key of the edge {0, 1} is 1, and fmix64(1) = 0xB456BCFC34C2CB2C."""
    assert MT.edge_key(1, 0) == 1 == MT.edge_key(0, 1) and MT.edge_key(5, 3) == (3 << 32) | 5
    assert MT._home_slot_edges(0, 1, 1 << 32) == 0x34C2CB2C
    assert MT._home_slot_edges(1, 0, 4096) == 0xB2C and MT._home_slot_edges(0, 1, 1) == 0
    for wrap in (False, True):
        (v, f), edges, size, home = EC.edge_collisions(wrap)
        assert size == 512 and home == (511 if wrap else 11) and len(set(edges)) == 40
        assert {MT._home_slot_edges(a, b, size) for a, b in edges} == {home}
        _, edge_faces, _, _, info = MT.mesh_edges_numpy(f, len(v))
        assert info["edges"] == 40 + 2 * 48 and info["manifold_edges"] == 8 and info["inconsistent_edges"] == 0


def _fake_edges(_cabi):
    a = _cabi.MeshEdgesArgs()
    a.num_verts, a.num_faces = 8, 4
    a.faces = a.scratch = a.record = a.vertex_degree = a.vertex_flags = 4096    # never dereferenced on the host
    return a


def _fake_smooth(_cabi):
    a = _cabi.MeshSmoothArgs()
    a.num_verts, a.num_faces, a.iterations, a.taubin, a.lam, a.mu = 8, 4, 10, 1, 0.5, -0.53
    a.verts = a.faces = a.scratch = a.record = a.out_verts = 4096
    return a


def test_abi(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    names = {"mgs_mesh_edges_args_size", "mgs_mesh_edges_scratch_bytes", "mgs_mesh_edges_count", "mgs_mesh_edges_emit",
             "mgs_mesh_smooth_args_size", "mgs_mesh_smooth_scratch_bytes", "mgs_mesh_smooth"}
    assert names <= set(_cabi.EXPORTS) and all(hasattr(L, n) for n in names)
    assert L.mgs_mesh_edges_args_size() == C.sizeof(_cabi.MeshEdgesArgs) == 2 * 4 + 7 * 8 + 2 * 4
    assert L.mgs_mesh_smooth_args_size() == C.sizeof(_cabi.MeshSmoothArgs) == 8 * 4 + 5 * 8
    assert _cabi.ABI_VERSION == 10 and L.mgs_abi_version() == 10
    assert L.mgs_struct_size(len(_cabi.struct_mirrors())) == -1          # the list ends where it ended
    header = open(os.path.join(os.path.dirname(_cabi.__file__), "..", "include", "monogs_raster.h"), encoding="utf-8").read()
    for n in names:
        assert f" {n}(" in header
    assert "#define MGS_MESH_EDGES_RECORD_INTS 16" in header and _cabi.MESH_EDGES_RECORD_INTS == 16
    assert "#define MGS_MESH_SMOOTH_MAX_ITERATIONS 1000" in header and SM.MAX_ITERATIONS == 1000


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    edge_fns = (L.mgs_mesh_edges_count, L.mgs_mesh_edges_emit)
    for fn in edge_fns + (L.mgs_mesh_smooth,):
        assert fn(None, None) == -1
    for fake, fns, fields in ((_fake_edges, edge_fns, ("scratch", "faces", "record")),
                              (_fake_smooth, (L.mgs_mesh_smooth,), ("scratch", "faces", "record", "verts", "out_verts"))):
        for field in fields:
            a = fake(_cabi)
            setattr(a, field, None)
            for fn in fns:
                assert fn(C.byref(a), None) == -1, field
        for field in ("num_verts", "num_faces"):
            a = fake(_cabi)
            setattr(a, field, -1)
            for fn in fns:
                assert fn(C.byref(a), None) == -1, field
        # 3 F >= 2^31, 3 V >= 2^31, and 3 F > 2^30 (the table)
        big = (2 ** 31 - 1) // 3
        for nv, nf in ((big + 1, 4), (8, big + 1), (8, 2 ** 30 // 3 + 1)):
            a = fake(_cabi)
            a.num_verts, a.num_faces = nv, nf
            for fn in fns:
                assert fn(C.byref(a), None) == -3, (nv, nf)
    for field in ("vertex_degree", "vertex_flags"):
        a = _fake_edges(_cabi)
        setattr(a, field, None)
        assert L.mgs_mesh_edges_count(C.byref(a), None) == -1
    a = _fake_edges(_cabi)
    a.out_num_edges = 0
    assert L.mgs_mesh_edges_emit(C.byref(a), None) == 0                  # nothing to write: no launch
    a.out_num_edges = 5                                                  # a count without outputs
    assert L.mgs_mesh_edges_emit(C.byref(a), None) == -1
    a.edges = a.edge_faces = 4096
    a.out_num_edges = 13                                                 # beyond the 12 half-edges
    assert L.mgs_mesh_edges_emit(C.byref(a), None) == -1
    a.out_num_edges = -1
    assert L.mgs_mesh_edges_emit(C.byref(a), None) == -1
    for field, values in (("lam", (0.0, -0.5, 1.5, float("nan"))), ("mu", (0.0, 0.5, -1.5, float("nan"))),
                          ("iterations", (-1, 1001))):
        for x in values:
            a = _fake_smooth(_cabi)
            setattr(a, field, x)
            assert L.mgs_mesh_smooth(C.byref(a), None) == -1, (field, x)
    for fn in (L.mgs_mesh_edges_scratch_bytes, L.mgs_mesh_smooth_scratch_bytes):
        assert fn(-1, 4) == 0 and fn(4, -1) == 0 and fn((2 ** 31 - 1) // 3 + 1, 4) == 0 and fn(4, 2 ** 30 // 3 + 1) == 0
    # the planes: three per half-edge, the block totals, the table; smoothing adds four per vertex, the rows, two position
    # planes and the exponent word
    pad = lambda b: (b + 255) // 256 * 256
    assert L.mgs_mesh_edges_scratch_bytes(0, 0) == 256 and L.mgs_mesh_smooth_scratch_bytes(0, 0) == 2 * 256
    V, F = 4099, 700
    edges = 3 * pad(4 * 3 * F) + pad(16 * ((V + 255) // 256)) + pad(4 * 8192)
    assert L.mgs_mesh_edges_scratch_bytes(V, F) == edges
    assert L.mgs_mesh_smooth_scratch_bytes(V, F) == edges + 4 * pad(4 * V) + pad(4 * 6 * F) + 2 * pad(12 * V) + 256


def test_drivers_raise_off_the_gpu_and_default_to_the_old_path():
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.slam_surrogate import reconstruct_mesh
    from monogs_amd.tsdf import TSDFVolume
    v, f = EC.hand()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    for call in (lambda: MT.mesh_edges(tf, 19), lambda: MT.mesh_topology(tf, 19), lambda: SM.smooth_mesh(tv, tf),
                 lambda: MT.mesh_edges(f, 19)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for kw in (dict(lam=0.0), dict(mu=0.25), dict(iterations=1001), dict(boundary="clamp")):        # before any launch
        with pytest.raises(ValueError, match="smooth_mesh: " + next(iter(kw))):
            SM.smooth_mesh(tv, tf, **kw)
    for fn in (save_mesh, reconstruct_mesh, TSDFVolume.extract_mesh):
        assert inspect.signature(fn).parameters["smooth"].default is None, fn
    assert inspect.signature(save_mesh).parameters["topology"].default is False
