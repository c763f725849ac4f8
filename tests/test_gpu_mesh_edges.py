"""The edge set, the topology report and smoothing on the device against their NumPy mirrors (monogs_amd/mesh_topology.py,
monogs_amd/mesh_smooth.py): every array and info bit for bit, two calls the same bytes, the refusals after the one host
read, the users' keywords, and the scores of a smoothed noisy sphere.

Sizes: mesh_edges_cases.py lists the block, scan-trip and hash-table boundaries and the case that crosses each."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_edges_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The scratch buffers the drivers keep between calls, and the allocator's cached blocks, go back to the device when
    this module is done: later modules meet the memory they met before this one existed."""
    yield
    from monogs_amd import _device
    for kind in ("edges", "smooth", "clean", "simplify"):
        _device._scratch.pop(kind, None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def floater_volume(big_only=False):
    from monogs_amd.tsdf import TSDFVolume
    vol = TSDFVolume(MC.FLOATER_ORIGIN, MC.FLOATER_VOXEL, MC.FLOATER_DIMS, device=_dev())
    for dst, src in zip((vol.tsdf, vol.weight, vol.color), MC.floater_planes(big_only)):
        dst.copy_(torch.from_numpy(src))
    return vol


def assert_edges_equal_mirror(f, V, twice=True):
    """mesh_edges on the device equals mesh_edges_numpy: the four arrays and info; returns the mirror's output."""
    from monogs_amd.mesh_topology import mesh_edges, mesh_edges_numpy, mesh_topology
    want = mesh_edges_numpy(f, V)
    df = to_dev(f)
    got = mesh_edges(df, V)
    assert got[4] == want[4]
    for a, b in zip(got[:4], want[:4]):
        assert a.dtype == torch.int32 and tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b)
    assert mesh_topology(df, V) == want[4]
    if twice:                                                          # two calls, the same bytes
        again = mesh_edges(df, V)
        assert again[4] == got[4] and all(torch.equal(a, b) for a, b in zip(again[:4], got[:4]))
    return want


def assert_smooth_equals_mirror(v, f, twice=True, **kw):
    """smooth_mesh on the device equals smooth_mesh_numpy: the position bits and info; returns the mirror's output."""
    from monogs_amd.mesh_smooth import smooth_mesh, smooth_mesh_numpy
    want = smooth_mesh_numpy(v, f, **kw)
    dv, df = to_dev(v), to_dev(f)
    got = smooth_mesh(dv, df, **kw)
    assert got[1] == want[1]
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == want[0].shape
    assert np.array_equal(bits(got[0]), want[0].view(np.int32))
    assert np.array_equal(bits(dv), v.view(np.int32))                  # the input is untouched
    if twice:
        again = smooth_mesh(dv, df, **kw)
        assert again[1] == got[1] and torch.equal(again[0], got[0])
    return want


@pytest.mark.parametrize("boundary", ["pin", "free"])
@pytest.mark.parametrize("mu", [-0.53, None], ids=["taubin", "laplacian"])
@pytest.mark.parametrize("iterations", [1, 10])
def test_floater_extraction_equals_the_mirror_bit_for_bit(built, iterations, mu, boundary):
    v, f = EC.floaters()
    want = assert_smooth_equals_mirror(v, f, iterations=iterations, mu=mu, boundary=boundary)
    assert want[1]["euler"] == 10 and want[1]["steps"] == iterations * (1 if mu is None else 2)
    assert (want[0].view(np.int32) != v.view(np.int32)).any(axis=1).all()          # closed: every vertex moves


def test_floater_edges_and_components(built):
    from monogs_amd.mesh_topology import mesh_topology, mesh_topology_numpy
    v, f = EC.floaters()
    want = assert_edges_equal_mirror(f, len(v))
    assert want[4]["edges"] == 7836 and want[4]["oriented"]
    got = mesh_topology(to_dev(f), len(v), components=True)
    assert got == mesh_topology_numpy(f, len(v), components=True) and got["components"] == 5 and got["euler"] == 10


@pytest.mark.parametrize("name", sorted(EC.SMALL_CASES))
def test_small_cases_equal_the_mirror_bit_for_bit(built, name):
    from monogs_amd import mesh_topology as MT
    from monogs_amd.mesh_simplify import table_size
    v, f = EC.SMALL_CASES[name]()
    if name.startswith("edge_"):                                       # the collisions, through the restated hash, first
        _, edges, size, home = EC.edge_collisions(name == "edge_wrap")
        assert size == table_size(3 * len(f)) and home == (size - 1 if name == "edge_wrap" else 11)
        assert {MT._home_slot_edges(a, b, size) for a, b in edges} == {home} and len(set(edges)) == 40
        assert set(edges) <= {tuple(sorted(e)) for face in f.tolist() for e in zip(face, face[1:] + face[:1])}
    want = assert_edges_equal_mirror(f, len(v))
    if name == "hand":
        assert want[4] == EC.HAND_INFO
    if name == "star":
        assert want[2].max() == 6000 and want[4]["edges"] == 9000
    if name == "empty_f0":
        assert want[4]["edges"] == 0 and not want[2].any() and not want[3].any() and want[4]["closed"]
    if name == "upper_half":
        assert want[4]["boundary_edges"] == 110
    if name == "long_rows":                                            # rows on both sides of the lane / workgroup change
        assert {h: int(want[2][h]) for h in EC.LONG_ROW_HUBS} == EC.LONG_ROW_HUBS
        pinned = assert_smooth_equals_mirror(v, f, iterations=2, boundary="pin")
        assert np.flatnonzero((pinned[0].view(np.int32) != v.view(np.int32)).any(axis=1)).tolist() == [301]
        assert_smooth_equals_mirror(v, f, iterations=10, boundary="free")
    for kw in (dict(iterations=3), dict(iterations=2, lam=0.25, mu=None, boundary="free")):
        assert_smooth_equals_mirror(v, f, **kw)
    same = assert_smooth_equals_mirror(v, f, iterations=0, twice=False)
    assert np.array_equal(same[0].view(np.int32), v.view(np.int32))


def test_second_scan_trip(built):
    v, f = EC.two_scan_trips()
    assert len(f) > 262144 + 256 and len(v) > 262144 + 256             # more than 1024 block totals of both kinds
    want = assert_edges_equal_mirror(f, len(v), twice=False)
    assert (want[0][-1] > 262144 + 256).all() and want[4]["edges"] > 262144 + 256     # edges and rows past block 1024
    assert_smooth_equals_mirror(v, f, twice=False, iterations=2, boundary="free")


def test_refusals_after_the_read(built):
    from monogs_amd.mesh_smooth import smooth_mesh
    from monogs_amd.mesh_topology import mesh_edges, mesh_topology
    v, f = EC.hand()
    g = f.copy()
    g[2, 1], g[7, 0] = 19, -1
    for fn, what in ((mesh_edges, "mesh_edges"), (mesh_topology, "mesh_topology")):
        with pytest.raises(ValueError, match=what + r": 2 of 13 faces hold an index outside \[0, 19\)"):
            fn(to_dev(g), 19)
    with pytest.raises(ValueError, match=r"smooth_mesh: 2 of 13 faces hold an index outside \[0, 19\)"):
        smooth_mesh(to_dev(v), to_dev(g))
    bad = v.copy()
    bad[3, 1], bad[6, 0], bad[6, 2] = np.nan, np.inf, -np.inf
    with pytest.raises(ValueError, match="smooth_mesh: 2 of 19 vertices are not finite"):
        smooth_mesh(to_dev(bad), to_dev(f))
    assert mesh_edges(to_dev(f), 19)[4] == EC.HAND_INFO                # and the next calls are whole
    assert_smooth_equals_mirror(v, f, twice=False, boundary="free")


def test_extract_mesh_keyword(built):
    from monogs_amd.mesh_simplify import simplify_mesh
    from monogs_amd.mesh_smooth import smooth_mesh
    vol = floater_volume()
    v, f, c = vol.extract_mesh()
    want, _ = smooth_mesh(v, f, iterations=5, mu=None)
    got = vol.extract_mesh(smooth=dict(iterations=5, mu=None))
    assert torch.equal(got[0], want) and torch.equal(got[1], f) and torch.equal(got[2], c)
    # after the clean-up and before the simplification
    cv, cf, cc = vol.extract_mesh(clean=dict(keep_largest=1))
    sv, _ = smooth_mesh(cv, cf)
    want = simplify_mesh(sv, cf, cc, cell=2.0 * vol.voxel_size, origin=vol.origin)
    got = vol.extract_mesh(clean=dict(keep_largest=1), simplify=dict(factor=2), smooth=dict())
    for a, b in zip(got, want[:3]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="lam"):
        vol.extract_mesh(smooth=dict(lam=2.0))
    # the default: what a call without the keyword gives, byte for byte
    for a, b in zip(vol.extract_mesh(smooth=None), (v, f, c)):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


def test_save_mesh_keywords(built, tmp_path):
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_topology import mesh_topology_numpy
    from monogs_amd.ply_io import read_mesh_ply
    vol = floater_volume()
    plain = save_mesh(vol, str(tmp_path / "plain"))
    explicit = save_mesh(vol, str(tmp_path / "explicit"), smooth=None, topology=False)
    assert os.listdir(os.path.dirname(explicit)) == ["mesh.ply"]
    assert open(plain, "rb").read() == open(explicit, "rb").read()
    path = save_mesh(vol, str(tmp_path / "report"), topology=True)
    assert open(plain, "rb").read() == open(path, "rb").read()
    v, f = EC.floaters()
    with open(os.path.join(os.path.dirname(path), "mesh_topology.json"), encoding="utf-8") as fh:
        report = json.load(fh)
    assert report == mesh_topology_numpy(f, len(v), components=True) and report["components"] == 5
    smooth = dict(iterations=3)
    path = save_mesh(vol, str(tmp_path / "smooth"), clean=dict(keep_largest=1), smooth=smooth, topology=True)
    pv, pf = read_mesh_ply(path)[:2]
    sv, sf, _ = vol.extract_mesh(clean=dict(keep_largest=1), smooth=smooth)
    assert np.array_equal(bits(pv), bits(sv)) and torch.equal(pf, sf.cpu()) and sf.shape[0] == 4580
    with open(os.path.join(os.path.dirname(path), "mesh_topology.json"), encoding="utf-8") as fh:
        report = json.load(fh)
    assert report == mesh_topology_numpy(sf.cpu().numpy(), sv.shape[0], components=True) and report["euler"] == 2


def test_smoothed_sphere_scores(built):
    """The mirror's prototype: precision 0.365 for the noisy sphere against the clean one at 0.1 voxel, 0.571 after 10
    Taubin iterations."""
    from monogs_amd.mesh_eval import evaluate_mesh
    from monogs_amd.mesh_smooth import smooth_mesh
    clean, f = EC.sphere()
    noisy, _ = EC.noisy_sphere()
    dc, dn, df = to_dev(clean), to_dev(noisy), to_dev(f)
    kw = dict(n_samples=20000, threshold=0.1 * MC.FLOATER_VOXEL, seed=0)
    before = evaluate_mesh((dn, df), (dc, df), **kw)["precision"]
    smoothed, _ = smooth_mesh(dn, df, iterations=10, lam=0.5, mu=-0.53)
    after = evaluate_mesh((smoothed, df), (dc, df), **kw)["precision"]
    print("precision noisy", before, "smoothed", after)
    assert after - before > 0.1
