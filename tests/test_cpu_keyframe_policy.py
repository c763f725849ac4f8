"""The keyframe policy's torch mirrors (monogs_amd/keyframe_policy.py) against what the reference's own
FrontEnd.is_keyframe / add_to_window / get_median_depth returned (tests/golden/keyframe_policy_ref.npz, written by
tests/golden/make_keyframe_policy_golden.py): decisions, windows, removed frames and the median exactly, the ratios
exactly (fp32 division of the exact counts), dist and the eviction scores to 1e-6 relative."""
import os
import types

import numpy as np
import pytest
import torch

from monogs_amd import keyframe_policy as KP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_policy_ref.npz")


def load_cases():
    z = np.load(GOLDEN)
    return z, [str(n) for n in z["names"]]


def case_inputs(z, name, dev="cpu"):
    g = lambda k: z[f"{name}_{k}"]
    N = int(g("N"))
    window = [int(v) for v in g("window")]
    ids = [int(v) for v in g("ids")]
    cams = {i: types.SimpleNamespace(T=torch.from_numpy(T).to(dev)) for i, T in zip(ids, g("T"))}
    cur_vis = torch.from_numpy(np.unpackbits(g("cur_vis"))[:N].astype(bool)).to(dev)
    rows = np.unpackbits(g("rows"), axis=1)[:, :N]
    occ = {kf: torch.from_numpy(rows[k].copy()).to(dev) for k, kf in enumerate(window)}
    depth = torch.from_numpy(g("depth")).to(dev)
    opacity = torch.from_numpy(g("opacity")).to(dev)
    return dict(N=N, window=window, cur=int(g("cur")), initialized=bool(g("initialized")),
                single_thread=bool(g("single_thread")), monocular=bool(g("monocular")), cams=cams,
                cur_vis=cur_vis, occ=occ, depth=depth, opacity=opacity)


def config_of(z):
    return {"Training": {str(k): float(v) if k.startswith("kf_") and k != "kf_interval" else int(v)
                         for k, v in zip(z["training_keys"], z["training"])}}


def test_fixture_covers_the_required_cases():
    z, names = load_cases()
    creates = [bool(z[f"{n}_create_kf"]) for n in names]
    assert any(creates) and not all(creates)
    assert any(bool(z[f"{n}_reset"]) for n in names)
    assert any(int(z[f"{n}_removed"]) >= 0 for n in names)
    assert any((z[f"{n}_scores"] >= 0).any() for n in names)                       # eviction by score
    assert any(not bool(z[f"{n}_initialized"]) for n in names) and any(bool(z[f"{n}_initialized"]) for n in names)
    assert any(np.isnan(z[f"{n}_median"]) for n in names)                          # no valid pixel
    assert len(z["names"]) >= 10


@pytest.mark.parametrize("name", load_cases()[1])
def test_mirrors_reproduce_the_reference(name):
    z, _ = load_cases()
    c = case_inputs(z, name)
    cfg = config_of(z)
    med = KP.median_depth(c["depth"][None], c["opacity"][None])
    want_med = z[f"{name}_median"]
    assert np.array_equal(np.float32(med.item()).view(np.uint32), np.float32(want_med).view(np.uint32)) or \
        (np.isnan(med.item()) and np.isnan(want_med))
    trace = {}
    vis = c["cur_vis"].long()
    d = KP.loop_decision(cfg, c["cams"], med, c["initialized"], c["monocular"], c["single_thread"], c["cur"],
                         c["window"], vis, c["occ"], trace)
    assert d["create_kf"] == bool(z[f"{name}_create_kf"])
    assert d["window"] == [int(v) for v in z[f"{name}_new_window"]]
    assert (-1 if d["removed"] is None else d["removed"]) == int(z[f"{name}_removed"])
    assert d["reset"] == bool(z[f"{name}_reset"])
    # dist to 1e-6 relative (the same CPU ops: in practice equal)
    np.testing.assert_allclose(float(trace["dist"]), float(z[f"{name}_dist"]), rtol=1e-6)
    # ratios: fp32 divisions of the exact counts
    cur = c["cur_vis"].numpy()
    row0 = c["occ"][c["window"][0]].numpy() != 0
    inter, union = int((cur & row0).sum()), int((cur | row0).sum())
    want = np.float32(inter) / np.float32(union) if union else np.float32("nan")
    got = np.float32(trace["overlap"].item())
    assert got.view(np.uint32) == want.view(np.uint32) or (np.isnan(got) and np.isnan(want))
    for kf, r in trace.get("ss_ratio", {}).items():
        row = c["occ"][kf].numpy() != 0
        den = min(int(cur.sum()), int(row.sum()))
        want = np.float32(int((cur & row).sum())) / np.float32(den) if den else np.float32("nan")
        got = np.float32(r.item())
        assert got.view(np.uint32) == want.view(np.uint32) or (np.isnan(got) and np.isnan(want)), kf
    scores = z[f"{name}_scores"]
    if (scores >= 0).any():
        got = np.full(len(c["window"]), -1.0)
        for kf, s in trace["scores"].items():
            got[c["window"].index(kf)] = s
        np.testing.assert_allclose(got, scores, rtol=1e-6)
    else:
        assert "scores" not in trace


def test_policy_torch_path_tracks_the_initialized_flag():
    """KeyframePolicy(native=False): the frontend's flag is set once the window is full and stays set."""
    z, _ = load_cases()
    c = case_inputs(z, "uninit_below_keep")
    trk = types.SimpleNamespace(n_touched=c["cur_vis"].to(torch.int32) * 3, depth=c["depth"][None],
                                opacity=c["opacity"][None])
    P = KP.KeyframePolicy(config_of(z), monocular=True, native=False)
    assert not P.initialized
    d = P.decide(c["cur"], c["cams"], c["window"], trk, c["occ"])
    assert not P.initialized and d.create_kf == bool(z["uninit_below_keep_create_kf"])
    win8 = list(range(35, -1, -5))
    cams = {i: types.SimpleNamespace(T=torch.eye(4)) for i in win8 + [40]}
    occ = {kf: c["occ"][c["window"][0]] for kf in win8}
    P.decide(40, cams, win8, trk, occ)
    assert P.initialized
    P.decide(40, cams, win8[:3], trk, occ)
    assert P.initialized
    P.reset_state()
    assert not P.initialized
    assert KP.KeyframePolicy(monocular=False, native=False).initialized


def test_length_mismatch_names_the_keyframe():
    z, _ = load_cases()
    c = case_inputs(z, "uninit_below_keep")
    trk = types.SimpleNamespace(n_touched=c["cur_vis"].to(torch.int32), depth=c["depth"][None],
                                opacity=c["opacity"][None])
    occ = dict(c["occ"])
    occ[5] = occ[5][:-1]
    P = KP.KeyframePolicy(config_of(z), native=False)
    with pytest.raises(ValueError, match="keyframe 5"):
        P.decide(c["cur"], c["cams"], c["window"], trk, occ)


def test_config_defaults_are_the_tum_base_config():
    P = KP.KeyframePolicy({"Training": {"window_size": 5, "unrelated": 1}})
    tr = P.config["Training"]
    assert tr == {"kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3,
                  "window_size": 5, "kf_interval": 5}
    assert P.window_size == 5 and P.kf_interval == 5
