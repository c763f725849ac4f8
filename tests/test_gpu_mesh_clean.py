"""Mesh clean-up on the device against its NumPy mirror (monogs_amd/mesh_clean.py): labels, counts record, vertices,
colours and faces bit for bit - the contract is order-free, so nothing is tolerated -, the floaters of a TSDF volume
against the extraction of the big sphere alone, and the path from a map to a cleaned PLY file.

Sizes: mesh_clean_cases.py lists the block, scan-trip and select-level boundaries and the case that crosses each."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_clean_cases as K

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def host_case(name):
    return K.case(name)


@functools.lru_cache(maxsize=None)
def device_case(name):
    v, c, f = host_case(name)
    dev = _dev()
    return (torch.from_numpy(v).to(dev), None if c is None else torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev))


@functools.lru_cache(maxsize=None)
def mirror(name, keep, min_faces):
    from monogs_amd.mesh_clean import clean_mesh_numpy
    v, c, f = host_case(name)
    return clean_mesh_numpy(v, f, c, keep_largest=keep, min_faces=min_faces)


def assert_equals_mirror(got, want):
    gv, gf, gc, ginfo = got
    wv, wf, wc, winfo = want
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32
    assert ginfo == winfo
    assert tuple(gv.shape) == wv.shape and tuple(gf.shape) == wf.shape
    assert np.array_equal(bits(gv), wv.view(np.int32))
    assert np.array_equal(gf.cpu().numpy(), wf)
    if wc is None:
        assert gc is None
    else:
        assert gc.dtype == torch.float32 and np.array_equal(bits(gc), wc.view(np.int32))


@pytest.mark.parametrize("name", K.SMALL_CASES + K.LARGE_CASES)
def test_labels_equal_the_mirror(built, name):
    from monogs_amd.mesh_clean import connected_components, connected_components_numpy
    v, _, f = host_case(name)
    dv, _, df = device_case(name)
    labels = connected_components(len(v), df)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (len(v),)
    want = connected_components_numpy(len(v), f)
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(connected_components(len(v), df).cpu().numpy(), want)        # and again


@pytest.mark.parametrize("param", K.PARAMS, ids=K.param_id)
def test_clean_mesh_equals_the_mirror_bit_for_bit(built, param):
    from monogs_amd.mesh_clean import clean_mesh
    name, keep, min_faces = param
    dv, dc, df = device_case(name)
    want = mirror(name, keep, min_faces)
    got = clean_mesh(dv, df, dc, keep_largest=keep, min_faces=min_faces)
    assert_equals_mirror(got, want)
    if len(want[1]):
        assert int(got[1].min()) >= 0 and int(got[1].max()) < got[0].shape[0]
    again = clean_mesh(dv, df, dc, keep_largest=keep, min_faces=min_faces)            # two calls, the same bytes
    assert np.array_equal(bits(again[0]), bits(got[0])) and torch.equal(again[1], got[1]) and again[3] == got[3]
    if dc is not None:
        assert np.array_equal(bits(again[2]), bits(got[2]))
        none = clean_mesh(dv, df, None, keep_largest=keep, min_faces=min_faces)        # colors=None passes through
        assert none[2] is None and torch.equal(none[1], got[1])


def floater_volume(big_only=False):
    from monogs_amd.tsdf import TSDFVolume
    vol = TSDFVolume(K.FLOATER_ORIGIN, K.FLOATER_VOXEL, K.FLOATER_DIMS, device=_dev())
    for dst, src in zip((vol.tsdf, vol.weight, vol.color), K.floater_planes(big_only)):
        dst.copy_(torch.from_numpy(src))
    return vol


def mesh_bits(mesh):
    return [bits(mesh[0]), mesh[1].cpu().numpy(), bits(mesh[2])]


def same_mesh(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(mesh_bits(a), mesh_bits(b)))


def test_floaters_of_a_volume_against_the_big_sphere_alone(built):
    from monogs_amd.mesh_clean import clean_mesh_numpy
    vol, big = floater_volume(), floater_volume(big_only=True)
    before = mesh_bits(vol.extract_mesh())                       # clean=None before the module's code has run here
    assert (len(before[0]), len(before[1])) == K.FLOATER_VF
    want = big.extract_mesh()
    assert (want[0].shape[0], want[1].shape[0]) == K.BIG_ONLY_VF
    assert float(want[2].max()) > 0.0                            # the colour plane is live
    assert same_mesh(vol.extract_mesh(clean=dict(keep_largest=1)), want)
    assert same_mesh(vol.extract_mesh(clean=dict(min_faces=309)), want)
    # one past the tied pair: the 144 / 144 / 48 clusters go, the second sphere stays
    v145, f145, c145 = vol.extract_mesh(clean=dict(min_faces=145))
    assert f145.shape[0] == 4580 + 308
    v3, f3, c3 = vol.extract_mesh(clean=dict(keep_largest=3))
    hv, hf, hc = (t.cpu().numpy() for t in vol.extract_mesh())
    rv, rf, rc, info = clean_mesh_numpy(hv, hf, hc, keep_largest=3)
    assert info["kept_clusters"] == 3 and info["faces_out"] == 4580 + 308 + 144
    assert np.array_equal(bits(v3), rv.view(np.int32)) and np.array_equal(f3.cpu().numpy(), rf)
    assert np.array_equal(bits(c3), rc.view(np.int32))
    # the lower-labelled of the tied pair stayed
    from monogs_amd.mesh_clean import connected_components
    labels = connected_components(len(hv), torch.from_numpy(hf).to(_dev())).cpu().numpy()
    count = np.bincount(labels[hf[:, 0]], minlength=len(hv))
    tied = np.flatnonzero(count == 144)
    kept = np.isin(labels, [np.flatnonzero(count == 4580)[0], np.flatnonzero(count == 308)[0], tied[0]])
    assert tied.size == 2 and np.array_equal(bits(v3), hv[kept].view(np.int32))
    # clean=None afterwards: the bytes it gave before
    after = mesh_bits(vol.extract_mesh())
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_bad_indices_raise_and_leave_no_state(built):
    from monogs_amd.mesh_clean import clean_mesh, connected_components, connected_components_numpy
    dv, dc, df = device_case("odd")
    V = dv.shape[0]
    bad = torch.cat([df, torch.tensor([[0, 19, V], [3, -1, 7]], dtype=torch.int32, device=df.device)])
    with pytest.raises(ValueError, match="2 of 13 faces"):
        clean_mesh(dv, bad, dc, keep_largest=1)
    with pytest.raises(ValueError):
        clean_mesh(dv, bad[:12], dc)
    # labels: a bad face connects nothing
    assert np.array_equal(connected_components(V, bad).cpu().numpy(), connected_components_numpy(V, host_case("odd")[2]))
    # the same workspace, a valid call afterwards
    assert_equals_mirror(clean_mesh(dv, df, dc, keep_largest=2), mirror("odd", 2, 0))
    assert_equals_mirror(clean_mesh(dv, bad[:11], dc), mirror("odd", None, 0))


def test_reconstruct_and_save_a_cleaned_mesh(built, tmp_path):
    """The small scene of test_gpu_tsdf.py::test_fuse_map_reconstruct_and_save."""
    from scenes import wide_scene
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_clean import clean_mesh_numpy, connected_components_numpy
    from monogs_amd.ply_io import quantise_colors, read_mesh_ply
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, ViewCamera
    from monogs_amd.slam_surrogate import reconstruct_mesh
    dev = _dev()
    sc = wide_scene()
    cam = sc.cam
    gm = GaussianParams(*(t.to(dev) for t in (sc.means3D, sc.log_scales, sc.rot, sc.opacity_logit, sc.features_dc)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    tau = torch.tensor([0.1, -0.05, 0.08, 0.03, -0.02, 0.01])
    cams = [ViewCamera(k, torch.zeros(3, cam.H, cam.W), SE3_exp(k * tau), cam.projmatrix_raw, fovx, fovy, cam.H, cam.W, dev)
            for k in range(3)]
    vs = 0.125
    result = {"cameras": {k: v for k, v in enumerate(cams)}, "kf_ids": [0, 1, 2], "gaussians": gm}
    raw = reconstruct_mesh(result, vs)
    V, F = raw[0].shape[0], raw[1].shape[0]
    assert V > 0 and F > 0
    clean = dict(keep_largest=1)
    cv, cf, cc = reconstruct_mesh(result, vs, clean=clean)
    want = clean_mesh_numpy(*(t.cpu().numpy() for t in (raw[0], raw[1], raw[2])), keep_largest=1)
    assert np.array_equal(bits(cv), want[0].view(np.int32)) and np.array_equal(cf.cpu().numpy(), want[1])
    assert np.array_equal(bits(cc), want[2].view(np.int32))
    path = save_mesh(gm, str(tmp_path / "clean"), cameras=cams, voxel_size=vs, clean=clean)
    pv, pf, pc = read_mesh_ply(path)
    assert 0 < pv.shape[0] <= V and 0 < pf.shape[0] <= F
    assert int(pf.min()) >= 0 and int(pf.max()) < pv.shape[0]
    labels = connected_components_numpy(pv.shape[0], pf.numpy())
    assert (labels == 0).all()                                   # one component, no unreferenced vertex
    assert np.array_equal(bits(pv), bits(cv)) and torch.equal(pf, cf.cpu())
    assert np.array_equal(pc.numpy(), quantise_colors(cc))
    # the un-cleaned calls still return what they returned
    assert same_mesh(reconstruct_mesh(result, vs), raw)
    path2 = save_mesh(gm, str(tmp_path / "raw"), cameras=cams, voxel_size=vs)
    rv, rf, rc = read_mesh_ply(path2)
    assert np.array_equal(bits(rv), bits(raw[0])) and torch.equal(rf, raw[1].cpu())
    assert np.array_equal(rc.numpy(), quantise_colors(raw[2]))
