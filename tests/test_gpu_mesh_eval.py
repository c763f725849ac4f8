"""Mesh evaluation on the device against its mirrors (monogs_amd/mesh_eval.py): sampled points and face indices, nearest
distances and indices bit for bit - both contracts are order-free, so nothing is tolerated -, the statistics record
(integers and maxima exactly, the fp64 sums to the order of adding), and the scores where they have to move: floaters
against the clean-up, mean against median fusion.

Sizes: mesh_eval_cases.py lists the block, scan-trip and grid-cap boundaries and the case that crosses each."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_clean_cases as MC
import mesh_eval_cases as K

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy()


@functools.lru_cache(maxsize=None)
def device_mesh(name):
    v, f = K.sampler_mesh(name)
    return torch.from_numpy(v).to(_dev()), torch.from_numpy(f).to(_dev())


# ---- sample_surface ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["philox", "randoms"])
@pytest.mark.parametrize("param", K.SAMPLER_PARAMS, ids=lambda p: f"{p[0]}-n{p[1]}")
def test_sample_surface_equals_the_mirror_bit_for_bit(built, param, path):
    from monogs_amd.mesh_eval import sample_surface, sample_surface_numpy
    name, n, seed = param
    v, f = K.sampler_mesh(name)
    dv, df = device_mesh(name)
    words = K.replay_words(n, seed) if path == "randoms" else None
    wp, wf, wrec = sample_surface_numpy(v, f, n, seed, randoms=words, with_record=True)
    dwords = None if words is None else torch.from_numpy(words).to(_dev())
    gp, gf, grec = sample_surface(dv, df, n, seed, randoms=dwords, with_record=True)
    assert gp.dtype == torch.float32 and gf.dtype == torch.int32 and tuple(gp.shape) == (n, 3) and tuple(gf.shape) == (n,)
    assert grec.cpu().tolist() == wrec.tolist()
    assert np.array_equal(gf.cpu().numpy(), wf)
    assert np.array_equal(bits(gp), wp.view(np.int32))
    if name == "two_trips":                                      # samples on both sides of the scan's trip boundary
        assert int((gf < 262144).sum()) > 1000 and int((gf >= 262144).sum()) > 1000
    if name in ("zero_area", "no_faces") and n:
        assert bool(torch.isnan(gp).all()) and bool((gf == -1).all()) and grec.cpu().tolist()[0] == 1
    ap, af = sample_surface(dv, df, n, seed, randoms=dwords)    # two calls, the same bytes
    assert np.array_equal(bits(ap), bits(gp)) and torch.equal(af, gf)


def test_sample_surface_words_and_share(built):
    from monogs_amd.mesh_eval import sample_surface, sample_words_numpy
    dev = _dev()
    v, f = (torch.from_numpy(t).to(dev) for t in K.two_triangles_3_to_1())
    n = 65536
    p, fi = sample_surface(v, f, n, seed=0)
    share = float((fi == 0).float().mean())
    print(f"share of the large face on the device: {share:.5f}")
    assert abs(share - 0.75) <= 5.0 * math.sqrt(0.75 * 0.25 / n)
    # the generator's words replayed through `randoms`, held as int32
    words = torch.from_numpy(sample_words_numpy(n, 0).astype(np.int64).astype(np.int32)).to(dev)
    p2, fi2 = sample_surface(v, f, n, seed=123, randoms=words)
    assert np.array_equal(bits(p), bits(p2)) and torch.equal(fi, fi2)
    with pytest.raises(ValueError):
        sample_surface(v, f, 10, randoms=words[:9])
    with pytest.raises(ValueError):
        sample_surface(v, f, -1)


# ---- nearest_distance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.NEAREST_CASES))
def test_nearest_distance_equals_the_brute_force_bit_for_bit(built, name):
    from monogs_amd.mesh_eval import nearest_distance, nearest_distance_torch
    dev = _dev()
    q, r, cell = K.nearest_case(name)
    dq, dr = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
    want_d2, want_i = nearest_distance_torch(dq, dr)             # the contract, run on the device
    got_d2, got_i = nearest_distance(dq, dr, cell_size=cell)
    assert got_d2.dtype == torch.float32 and got_i.dtype == torch.int32
    assert tuple(got_d2.shape) == tuple(got_i.shape) == (len(q),)
    assert np.array_equal(got_i.cpu().numpy(), want_i.cpu().numpy())
    assert np.array_equal(bits(got_d2), bits(want_d2))
    host_d2, host_i = nearest_distance_torch(torch.from_numpy(q), torch.from_numpy(r))          # and on the host
    assert np.array_equal(bits(host_d2), bits(want_d2)) and torch.equal(host_i, want_i.cpu())
    if name == "lattice_ties":
        assert bool((got_d2 == 0.75).all())
    if name in ("no_ref", "all_non_finite"):
        assert bool(torch.isinf(got_d2).all()) and bool((got_i == -1).all())
    again = nearest_distance(dq, dr, cell_size=cell)             # two calls, the same bytes
    assert np.array_equal(bits(again[0]), bits(got_d2)) and torch.equal(again[1], got_i)


@pytest.mark.parametrize("cell", [None, 0.01, 0.05, 0.5, 3.0, 1e9])
def test_nearest_distance_does_not_depend_on_the_cell_size(built, cell):
    from monogs_amd.mesh_eval import nearest_distance, nearest_distance_torch
    dev = _dev()
    q, r, _ = K.nearest_case("surface")
    dq, dr = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
    want = nearest_distance_torch(dq, dr)
    for a, b in ((dq, dr), (dr, dq)):
        want = nearest_distance_torch(a, b)
        got = nearest_distance(a, b, cell_size=cell)
        assert np.array_equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        nearest_distance(dq, dr, cell_size=0.0)
    with pytest.raises(ValueError):
        nearest_distance(dq, dr, cell_size=float("nan"))


# ---- statistics and evaluate_mesh ----------------------------------------------------------------------------------------
def _assert_record(got, want_dirs, flags=(0, 0, 0, 0)):
    got = [float(x) for x in got]
    for d, st in enumerate(want_dirs):
        n, below, mx, sm = got[4 * d:4 * d + 4]
        assert (n, below) == (st["n"], st["below"])
        assert np.float32(mx) == np.float32(st["max"]) and mx == float(np.float32(mx))
        assert abs(sm - st["sum"]) <= max(st["n"], 1) * 2.0 ** -53 * st["sum"], (sm, st["sum"])
    assert tuple(got[8:12]) == tuple(float(x) for x in flags)


@pytest.mark.parametrize("name", ["surface", "non_finite", "outside", "no_ref", "strided"])
def test_distance_stats_equal_the_mirror(built, name):
    from monogs_amd.mesh_eval import distance_stats, distance_stats_numpy, nearest_distance_torch
    dev = _dev()
    if name == "strided":                                        # more items than the 256 x 256 threads of a launch
        rng = np.random.default_rng(80)
        a, b = (rng.uniform(0.0, 0.04, n).astype(np.float32) for n in (70001, 65537))
        a[::1000], b[5], b[-1] = np.inf, np.nan, 9.0
        a, b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    else:
        q, r, _ = K.nearest_case(name)
        dq, dr = torch.from_numpy(q).to(dev), torch.from_numpy(r).to(dev)
        a, b = nearest_distance_torch(dq, dr)[0], nearest_distance_torch(dr, dq)[0]
    thr = 0.05 if name == "surface" else 0.1
    rec = distance_stats(a, b, thr)
    assert rec.dtype == torch.float64 and tuple(rec.shape) == (12,)
    want = [distance_stats_numpy(t.cpu().numpy(), thr) for t in (a, b)]
    _assert_record(rec.cpu().numpy(), want)
    if name == "surface":
        assert 0 < want[0]["below"] < want[0]["n"]
    again = distance_stats(a, b, thr)                            # two calls, the same bytes
    assert np.array_equal(rec.cpu().numpy().view(np.int64), again.cpu().numpy().view(np.int64))
    with pytest.raises(ValueError):
        distance_stats(a, b, -1.0)


def floater_volume(big_only=False):
    from monogs_amd.tsdf import TSDFVolume
    vol = TSDFVolume(MC.FLOATER_ORIGIN, MC.FLOATER_VOXEL, MC.FLOATER_DIMS, device=_dev())
    for dst, src in zip((vol.tsdf, vol.weight, vol.color), MC.floater_planes(big_only)):
        dst.copy_(torch.from_numpy(src))
    return vol


def test_evaluate_mesh_floaters_against_the_big_sphere(built):
    from monogs_amd.mesh_eval import METRIC_KEYS, evaluate_mesh, evaluate_mesh_numpy
    gv, gf, _ = floater_volume(big_only=True).extract_mesh()
    vol = floater_volume()
    thr = 0.5 * MC.FLOATER_VOXEL
    scores = {}
    for key, clean in (("raw", None), ("clean", dict(keep_largest=1))):
        v, f, _ = vol.extract_mesh() if clean is None else vol.extract_mesh(clean=clean)
        scores[key] = evaluate_mesh((v, f), (gv, gf), n_samples=20000, threshold=thr, seed=0)
        assert tuple(scores[key]) == METRIC_KEYS and scores[key]["n_pred"] == scores[key]["n_gt"] == 20000
        # the device against the mirror on the same meshes, at a size the host's brute force affords
        got, rec = evaluate_mesh((v, f), (gv, gf), n_samples=4099, threshold=thr, seed=3, with_record=True)
        want, wrec = evaluate_mesh_numpy((v.cpu().numpy(), f.cpu().numpy()), (gv.cpu().numpy(), gf.cpu().numpy()),
                                         n_samples=4099, threshold=thr, seed=3, with_record=True)
        for d in range(2):
            assert tuple(rec[4 * d:4 * d + 3]) == tuple(wrec[4 * d:4 * d + 3])           # counts and maximum: exact
            assert abs(rec[4 * d + 3] - wrec[4 * d + 3]) <= 4099 * 2.0 ** -53 * wrec[4 * d + 3]
        assert tuple(rec[8:]) == tuple(wrec[8:]) == (0.0, 0.0, 0.0, 0.0)
        for k in ("precision", "recall", "completion_ratio", "f_score", "hausdorff", "n_pred", "n_gt", "bad_faces"):
            assert got[k] == want[k], k
        for k in ("accuracy", "completion", "chamfer"):
            assert abs(got[k] - want[k]) <= 1e-12 * want[k], k
    raw, clean = scores["raw"], scores["clean"]
    print(f"floaters: precision {raw['precision']:.4f} recall {raw['recall']:.4f}; cleaned: precision "
          f"{clean['precision']:.4f} recall {clean['recall']:.4f} hausdorff {clean['hausdorff']:.3f}")
    assert raw["recall"] == 1.0 and raw["precision"] < 0.9
    assert clean["precision"] == 1.0 and clean["recall"] == 1.0 and clean["f_score"] == 1.0
    again = evaluate_mesh(vol.extract_mesh()[:2], (gv, gf), n_samples=20000, threshold=thr, seed=0)
    assert again == raw                                          # two calls, the same numbers


def test_evaluate_mesh_flags_points_and_transform(built):
    from monogs_amd.mesh_eval import evaluate_mesh, evaluate_mesh_numpy
    dev = _dev()
    sq = tuple(torch.from_numpy(t).to(dev) for t in K.square(0.0, 3))
    with pytest.raises(ValueError, match="2 faces"):
        evaluate_mesh(device_mesh("bad_index"), sq, n_samples=64)
    with pytest.raises(ValueError, match="pred mesh"):
        evaluate_mesh(device_mesh("zero_area"), sq, n_samples=64)
    with pytest.raises(ValueError, match="gt mesh"):
        evaluate_mesh(sq, device_mesh("no_faces"), n_samples=64)
    # a point tensor as ground truth, and a transform: the two parallel squares of the host test
    D, pitch = 0.25, 1.0 / 32.0
    far = math.sqrt(D * D + 0.5 * pitch * pitch)
    lattice = K.square_lattice(D, pitch)
    gt = torch.from_numpy(lattice).to(dev)
    out = evaluate_mesh(sq, gt, n_samples=4096, threshold=D * 0.999)
    assert out["n_gt"] == 33 * 33 and D <= out["accuracy"] <= far * (1 + 1e-6) and out["completion"] >= D
    assert out["precision"] == 0.0 and out["recall"] == 0.0 and out["f_score"] == 0.0
    assert evaluate_mesh(sq, gt, n_samples=4096, threshold=far * 1.001)["precision"] == 1.0
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tr = (1.5, R, (0.3, -0.2, D))
    got = evaluate_mesh(sq, gt, n_samples=2048, threshold=pitch, transform=tr)
    want = evaluate_mesh_numpy(K.square(0.0, 3), lattice, n_samples=2048, threshold=pitch, transform=tr)
    for k in want:
        assert got[k] == want[k] or abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3], M[:3, 3] = 1.5 * torch.from_numpy(R), torch.tensor([0.3, -0.2, D], dtype=torch.float64)
    assert evaluate_mesh(sq, gt, n_samples=2048, threshold=pitch, transform=M) == got


def test_median_fusion_scores_a_higher_precision_than_mean_fusion(built):
    """The vertices between the two layers (test_gpu_surface.py::test_two_layer_mesh_on_the_device) as a metric, at
    threshold = the truncation distance."""
    import surface_cases as SC
    from monogs_amd.slam_loops import ViewCamera
    from monogs_amd import tsdf as T
    from monogs_amd.mesh_eval import evaluate_mesh
    dev = _dev()
    sc = SC.scene("two_layer")
    c = sc.cam
    cam = ViewCamera(0, torch.zeros(3, c.H, c.W), torch.eye(4), c.projmatrix_raw, 2 * math.atan(c.tanfovx),
                     2 * math.atan(c.tanfovy), c.H, c.W, dev, intrinsics=(c.fx, c.fy, c.cx, c.cy))
    gm, bg = SC.model(sc, dev), sc.bg.to(dev)
    vs = SC.LAYER_VOLUME["voxel_size"]
    gt = tuple(torch.from_numpy(t).to(dev) for t in K.two_layer_truth(sc.cam))
    precision = {}
    for mode in ("mean", "median"):
        vol = T.TSDFVolume(SC.LAYER_VOLUME["origin"], vs, SC.LAYER_VOLUME["dims"], device=dev)
        T.fuse_map(gm, [cam], bg, vs, volume=vol, depth_mode=mode)
        verts, faces, _ = vol.extract_mesh()
        precision[mode] = evaluate_mesh((verts, faces), gt, n_samples=20000, threshold=vol.trunc)["precision"]
    print(f"precision at the truncation distance {vol.trunc}: mean {precision['mean']:.4f}, median {precision['median']:.4f}")
    assert precision["median"] > precision["mean"]
    assert precision["median"] > 0.99 and precision["mean"] < 0.9


def test_save_mesh_and_run_evaluation(built, tmp_path):
    """The small scene of test_gpu_tsdf.py::test_fuse_map_reconstruct_and_save, with five cameras off one line."""
    from scenes import wide_scene
    from monogs_amd import slam_surrogate
    from monogs_amd.eval_native import save_mesh
    from monogs_amd.mesh_eval import METRIC_KEYS, apply_transform
    from monogs_amd.ply_io import read_mesh_ply
    from monogs_amd.pose import SE3_exp
    from monogs_amd.slam_loops import GaussianParams, ViewCamera
    dev = _dev()
    sc = wide_scene()
    cam = sc.cam
    gm = GaussianParams(*(t.to(dev) for t in (sc.means3D, sc.log_scales, sc.rot, sc.opacity_logit, sc.features_dc)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    taus = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.1, -0.05, 0.08, 0.03, -0.02, 0.01],
                         [-0.12, 0.07, 0.02, -0.02, 0.03, 0.0], [0.04, 0.11, -0.06, 0.01, 0.0, -0.03],
                         [-0.03, -0.09, 0.12, 0.0, 0.02, 0.02]])
    cams = [ViewCamera(k, torch.zeros(3, cam.H, cam.W), SE3_exp(tau), cam.projmatrix_raw, fovx, fovy, cam.H, cam.W, dev)
            for k, tau in enumerate(taus)]
    vs = 0.125
    result = {"cameras": {k: v for k, v in enumerate(cams)}, "kf_ids": [0, 1, 2, 3, 4], "gaussians": gm}
    raw = slam_surrogate.reconstruct_mesh(result, vs)
    eval_kw = dict(n_samples=100_000, threshold=vs)             # two samplings of one surface: gaps far below a voxel
    # save_mesh: the file as before, the scores beside it
    scores = save_mesh(gm, str(tmp_path / "scored"), cameras=cams, voxel_size=vs, gt=(raw[0], raw[1]), eval_kw=eval_kw)
    assert tuple(scores) == METRIC_KEYS and scores["f_score"] > 0.999 and scores["accuracy"] < 0.5 * vs
    folder = os.path.join(str(tmp_path / "scored"), "point_cloud", "final")
    with open(os.path.join(folder, "mesh_eval.json"), encoding="utf-8") as fh:
        assert json.load(fh) == scores
    path = save_mesh(gm, str(tmp_path / "plain"), cameras=cams, voxel_size=vs)
    assert path.endswith("mesh.ply") and sorted(os.listdir(os.path.dirname(path))) == ["mesh.ply"]
    with open(path, "rb") as a, open(os.path.join(folder, "mesh.ply"), "rb") as b:
        assert a.read() == b.read()                              # gt=None: byte for byte what it wrote before
    pv, pf, _ = read_mesh_ply(path)
    assert np.array_equal(bits(pv), bits(raw[0])) and torch.equal(pf, raw[1].cpu())
    # the run's scores: the ground truth lives in a frame that is a known Sim(3) of the run's
    c, t = 1.7, torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64)
    R = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    for v in cams:
        centre = torch.linalg.inv(v.T.double().cpu())[:3, 3]
        T_gt = torch.eye(4, dtype=torch.float64)
        T_gt[:3, 3] = -(c * R @ centre + t)
        v.T_gt = T_gt
    gt = (apply_transform(raw[0], (c, R, t)), raw[1])
    out = slam_surrogate.evaluate_mesh(result, gt, vs, monocular=True, n_samples=100_000, threshold=c * vs)
    assert out["f_score"] > 0.999 and out["accuracy"] < 0.5 * c * vs and out["completion"] < 0.5 * c * vs
    rigid = slam_surrogate.evaluate_mesh(result, gt, vs, monocular=False, n_samples=100_000, threshold=0.1 * vs)
    assert rigid["f_score"] < 0.5                                # without the scale the surfaces do not meet
