"""Mesh clean-up without a GPU: the NumPy mirror that defines the contract (monogs_amd/mesh_clean.py) against two
independent statements of the components - scipy.sparse.csgraph.connected_components and a plain union-find -, the
extraction of the largest sphere alone as an oracle that knows nothing of the mirror, the tie rule against an explicit
sort, and the C-ABI boundary of the new entry points."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import mesh_clean_cases as K


@pytest.mark.parametrize("name", K.SMALL_CASES + K.LARGE_CASES)
def test_mirror_labels_equal_scipys_partition_with_the_smallest_index_rule(name):
    pytest.importorskip("scipy")
    from monogs_amd.mesh_clean import connected_components_numpy
    v, _, f = K.case(name)
    V = len(v)
    labels = connected_components_numpy(V, f)
    assert labels.dtype == np.int32 and labels.shape == (V,)
    n, part = K.scipy_components(V, f)
    K.assert_labels_are(labels, V, part)
    assert len(np.unique(labels)) == n


@pytest.mark.parametrize("name", K.SMALL_CASES)
def test_mirror_labels_equal_a_plain_union_find(name):
    from monogs_amd.mesh_clean import connected_components_numpy
    v, _, f = K.case(name)
    assert np.array_equal(connected_components_numpy(len(v), f), K.union_find_labels(len(v), f))


def test_floaters_are_what_the_issue_counted():
    pytest.importorskip("scipy")
    from monogs_amd.mesh_clean import clean_mesh_numpy
    v, c, f = K.case("floaters")
    assert (len(v), len(f)) == K.FLOATER_VF
    n, part = K.scipy_components(len(v), f)
    assert n == 5
    assert tuple(sorted(np.bincount(part[f[:, 0]]).tolist(), reverse=True)) == K.FLOATER_CLUSTERS
    _, _, _, info = clean_mesh_numpy(v, f, c)
    assert info == dict(num_clusters=5, kept_clusters=5, verts_in=2622, faces_in=5224, verts_out=2622, faces_out=5224)


def test_min_faces_cuts_between_the_floaters():
    """min_faces = 145 is one past the tied pair: the 144 / 144 / 48 clusters go, 4580 and 308 stay; 309 is one past
    the second sphere and leaves the big one alone, as keep_largest = 1 does."""
    from monogs_amd.mesh_clean import clean_mesh_numpy
    v, c, f = K.case("floaters")
    for m, clusters, faces in ((48, 5, 5224), (49, 4, 5176), (144, 4, 5176), (145, 2, 4888), (308, 2, 4888),
                               (309, 1, 4580), (4580, 1, 4580), (4581, 0, 0)):
        info = clean_mesh_numpy(v, f, c, min_faces=m)[3]
        assert (info["kept_clusters"], info["faces_out"]) == (clusters, faces), m


@pytest.mark.parametrize("kw", [dict(keep_largest=1), dict(min_faces=309), dict(keep_largest=2, min_faces=309)])
def test_cleaned_floaters_equal_the_extraction_of_the_big_sphere_alone(kw):
    from monogs_amd.mesh_clean import clean_mesh_numpy
    v, c, f = K.case("floaters")
    bv, bf, bc = K.floater_mesh(big_only=True)
    assert (len(bv), len(bf)) == K.BIG_ONLY_VF
    ov, of, oc, info = clean_mesh_numpy(v, f, c, **kw)
    assert ov.dtype == np.float32 and of.dtype == np.int32 and oc.dtype == np.float32
    assert np.array_equal(ov.view(np.int32), bv.view(np.int32))
    assert np.array_equal(oc.view(np.int32), bc.view(np.int32))
    assert np.array_equal(of, bf)
    assert info["kept_clusters"] == 1 and info["num_clusters"] == 5
    assert (info["verts_out"], info["faces_out"]) == K.BIG_ONLY_VF


def test_keep_three_keeps_the_lower_labelled_of_the_tied_floaters():
    from monogs_amd.mesh_clean import clean_mesh_numpy, connected_components_numpy
    v, c, f = K.case("floaters")
    labels = connected_components_numpy(len(v), f)
    count = np.bincount(labels[f[:, 0]], minlength=len(v))
    tied = np.flatnonzero(count == 144)
    assert tied.size == 2
    ov, of, _, info = clean_mesh_numpy(v, f, c, keep_largest=3)
    assert info["kept_clusters"] == 3 and info["faces_out"] == 4580 + 308 + 144
    big, mid = int(np.flatnonzero(count == 4580)[0]), int(np.flatnonzero(count == 308)[0])
    vkeep = np.isin(labels, [big, mid, int(tied[0])])                  # tied ascends: the lower label stays
    assert np.array_equal(ov.view(np.int32), v[vkeep].view(np.int32))
    assert np.array_equal(of, (np.cumsum(vkeep) - 1)[f[vkeep[f[:, 0]]]])


@pytest.mark.parametrize("min_faces", K.TIES_MIN)
@pytest.mark.parametrize("keep", (None,) + K.TIES_KEEP)
def test_tie_rule_against_an_explicit_sort(keep, min_faces):
    from monogs_amd.mesh_clean import clean_mesh_numpy
    v, c, f = K.case("ties")
    V = len(v)
    labels = K.union_find_labels(V, f)
    sizes = {}
    for lab in labels[f[:, 0]].tolist():
        sizes[lab] = sizes.get(lab, 0) + 1
    assert sorted(sizes.values()) == [1] * 40 + [5] * 6 + [9] * 3
    ranked = sorted(sizes, key=lambda lab: (-sizes[lab], lab))
    kept = [lab for r, lab in enumerate(ranked) if sizes[lab] >= max(min_faces, 1) and (keep is None or r < keep)]
    vkeep = np.isin(labels, kept)
    fkeep = vkeep[f[:, 0]]
    new = np.cumsum(vkeep) - 1
    ov, of, oc, info = clean_mesh_numpy(v, f, c, keep_largest=keep, min_faces=min_faces)
    assert np.array_equal(ov, v[vkeep]) and np.array_equal(oc, c[vkeep]) and np.array_equal(of, new[f[fkeep]])
    assert info == dict(num_clusters=49, kept_clusters=len(kept), verts_in=V, faces_in=len(f),
                        verts_out=int(vkeep.sum()), faces_out=int(fkeep.sum()))


def test_mirror_on_degenerate_duplicate_unreferenced_and_empty_input():
    from monogs_amd.mesh_clean import clean_mesh_numpy, connected_components_numpy
    v, c, f = K.case("odd")
    labels = connected_components_numpy(20, f)
    assert labels.tolist() == [0, 0, 0, 3, 4, 4, 4, 7, 8, 9, 10, 11, 10, 10, 10, 15, 15, 17, 18, 19]
    ov, of, oc, info = clean_mesh_numpy(v, f, c)
    assert info["num_clusters"] == 5 and info["kept_clusters"] == 5 and info["verts_out"] == 13 and info["faces_out"] == 11
    assert of.tolist()[:5] == [[0, 0, 1], [1, 2, 2], [3, 4, 5], [3, 4, 5], [5, 4, 3]]      # duplicates stay, renumbered
    _, of2, _, info2 = clean_mesh_numpy(v, f, c, keep_largest=2)                            # 3 / 3 / 2 / 2 / 1 faces
    assert info2["kept_clusters"] == 2 and of2.tolist() == [[0, 0, 1], [1, 2, 2], [3, 4, 5], [3, 4, 5], [5, 4, 3], [2, 1, 0]]
    for V in (0, 7):
        ev, ec, ef = K.empty(V)
        ov, of, oc, info = clean_mesh_numpy(ev, ef, ec, keep_largest=1)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and oc.shape == (0, 3) and of.dtype == np.int32
        assert info == dict(num_clusters=0, kept_clusters=0, verts_in=V, faces_in=0, verts_out=0, faces_out=0)
        assert connected_components_numpy(V, ef).tolist() == list(range(V))
    assert clean_mesh_numpy(v, f, None)[2] is None
    # a bad index connects nothing and raises
    bad = np.concatenate([f, np.array([[0, 19, 20], [3, -1, 7]], np.int32)])
    assert np.array_equal(connected_components_numpy(20, bad), labels)
    with pytest.raises(ValueError, match="2 of 13 faces"):
        clean_mesh_numpy(v, bad, c)
    with pytest.raises(ValueError):
        clean_mesh_numpy(v, f, c, keep_largest=-1)
    with pytest.raises(ValueError):
        clean_mesh_numpy(v, f, c, min_faces=-1)


def test_exports_struct_size_and_abi_version(built):
    import monogs_amd
    from monogs_amd import _cabi, mesh_clean
    names = ("mgs_mesh_clean_args_size", "mgs_mesh_clean_scratch_bytes", "mgs_mesh_clean_count", "mgs_mesh_clean_emit",
             "mgs_mesh_components")
    for n in names:
        assert n in _cabi.EXPORTS, n
    L = _cabi.lib()
    assert L.mgs_mesh_clean_args_size() == C.sizeof(_cabi.MeshCleanArgs) == 4 * 4 + 9 * 8 + 2 * 4
    assert _cabi.ABI_VERSION == 10 and L.mgs_abi_version() == 10
    assert L.mgs_struct_size(len(_cabi.struct_mirrors())) == -1          # the list ends where it ended
    for n in ("clean_mesh", "connected_components", "clean_mesh_numpy", "connected_components_numpy"):
        assert getattr(monogs_amd, n) is getattr(mesh_clean, n)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(built):
    from monogs_amd import _cabi
    L = _cabi.lib()
    fake = 4096                                                           # never dereferenced on the host
    for fn in (L.mgs_mesh_clean_count, L.mgs_mesh_clean_emit, L.mgs_mesh_components):
        assert fn(None, None) == -1
    a = _cabi.MeshCleanArgs()
    a.num_verts, a.num_faces, a.keep_largest = 8, 4, -1
    for fn in (L.mgs_mesh_clean_count, L.mgs_mesh_clean_emit, L.mgs_mesh_components):
        assert fn(C.byref(a), None) == -1                                 # no scratch
    a.scratch = fake
    assert L.mgs_mesh_clean_count(C.byref(a), None) == -1                 # no faces
    assert L.mgs_mesh_components(C.byref(a), None) == -1
    a.faces = fake
    assert L.mgs_mesh_clean_count(C.byref(a), None) == -1                 # no counts
    assert L.mgs_mesh_components(C.byref(a), None) == -1                  # no labels
    a.counts = a.labels = fake
    a.keep_largest = -2
    assert L.mgs_mesh_clean_count(C.byref(a), None) == -1
    a.keep_largest, a.min_faces = 1, -1
    assert L.mgs_mesh_clean_count(C.byref(a), None) == -1
    a.min_faces = 0
    a.num_verts = -1
    for fn in (L.mgs_mesh_clean_count, L.mgs_mesh_clean_emit, L.mgs_mesh_components):
        assert fn(C.byref(a), None) == -1
    a.num_verts = 8
    # emit: counts without outputs, counts beyond the input, nothing to write
    a.out_num_verts, a.out_num_faces = 3, 1
    assert L.mgs_mesh_clean_emit(C.byref(a), None) == -1
    a.verts = a.out_verts = a.out_faces = fake
    a.colors = fake                                                       # colours without a place to put them
    assert L.mgs_mesh_clean_emit(C.byref(a), None) == -1
    a.out_colors = fake
    a.out_num_verts = 9
    assert L.mgs_mesh_clean_emit(C.byref(a), None) == -1
    a.out_num_verts, a.out_num_faces = -1, 0
    assert L.mgs_mesh_clean_emit(C.byref(a), None) == -1
    a.out_num_verts = 0
    assert L.mgs_mesh_clean_emit(C.byref(a), None) == 0                   # nothing to write: no launch
    # sizes beyond 32-bit element indices
    big = (2 ** 31 - 1) // 3
    assert 3 * big < 2 ** 31 <= 3 * (big + 1) and _cabi.MESH_CLEAN_MAX_ITEMS == big
    for nv, nf in ((big + 1, 4), (8, big + 1)):
        a.num_verts, a.num_faces = nv, nf
        for fn in (L.mgs_mesh_clean_count, L.mgs_mesh_clean_emit, L.mgs_mesh_components):
            assert fn(C.byref(a), None) == -3
        assert L.mgs_mesh_clean_scratch_bytes(nv, nf) == 0
    assert L.mgs_mesh_clean_scratch_bytes(-1, 4) == 0 and L.mgs_mesh_clean_scratch_bytes(4, -1) == 0
    assert L.mgs_mesh_clean_scratch_bytes(big, big) > 6 * 4 * big
    # V = 0 and F = 0 are legal sizes
    pad = lambda b: (b + 255) // 256 * 256
    fixed = pad(4 * (2048 + 2048 + 1024)) + 256
    assert L.mgs_mesh_clean_scratch_bytes(0, 0) == fixed
    V, F = 4099, 700
    assert L.mgs_mesh_clean_scratch_bytes(V, F) == fixed + 5 * pad(4 * V) + pad(4 * F) + 2 * pad(16 * ((V + 255) // 256))


def test_device_entry_points_raise_off_the_gpu():
    from monogs_amd.mesh_clean import clean_mesh, connected_components
    v, c, f = K.case("odd")
    with pytest.raises(RuntimeError, match="GPU only"):
        clean_mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c), keep_largest=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        clean_mesh(v, f)
    with pytest.raises(RuntimeError, match="GPU only"):
        connected_components(len(v), torch.from_numpy(f))
    with pytest.raises(ValueError):
        clean_mesh(torch.from_numpy(v), torch.from_numpy(f), keep_largest=-3)


def test_mesh_paths_default_to_no_clean_up():
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.slam_surrogate import reconstruct_mesh
    from monogs_amd.tsdf import TSDFVolume
    for fn in (save_mesh, reconstruct_mesh, TSDFVolume.extract_mesh):
        p = inspect.signature(fn).parameters["clean"]
        assert p.default is None, fn
    assert inspect.signature(TSDFVolume.extract_mesh).parameters["min_weight"].default == 1.0
