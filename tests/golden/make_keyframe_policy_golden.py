"""Golden vectors for the keyframe policy, produced by RUNNING the reference's own Python on the CPU (build container
only; the reference tree does not exist on the GPU box):

    python tests/golden/make_keyframe_policy_golden.py      ->  tests/golden/keyframe_policy_ref.npz

What is run (nothing of it is copied; only arrays - inputs and what the reference returned - are stored):
  * utils/slam_frontend.py: FrontEnd.is_keyframe (:1692-1720) and FrontEnd.add_to_window (:1722-1783), called unbound
    with a SimpleNamespace `self` holding config, cameras (.T), median_depth and initialized;
  * utils/slam_utils.py: get_median_depth (:286-297) of each case's depth / opacity;
  * the run loop's decision (:1914-1950) chains them here as the loop does: check_time, is_keyframe, the IoU rule
    while the window is not full, the single-thread AND, add_to_window, the monocular reset.
slam_frontend imports cv2, diff_gaussian_rasterization, open3d, plyfile, simple_knn, evo, torchmetrics, wandb and
lietorch at its top (not installed: empty modules stand in; nothing of them runs).  torch.norm and np.argmax are
wrapped inside the reference module to record dist and the eviction scores it computed.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path[:0] = [REF]
STUBS = ("cv2", "diff_gaussian_rasterization", "open3d", "plyfile", "simple_knn", "evo", "torchmetrics", "wandb",
         "lietorch")


class _Stub(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return type(n, (), {})


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        return importlib.machinery.ModuleSpec(name, self, is_package=True) if name.split(".")[0] in STUBS else None

    def create_module(self, spec):
        m = _Stub(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _StubFinder())
import utils.slam_frontend as F  # noqa: E402
import utils.slam_utils as SU  # noqa: E402

TRAINING = {"kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3,
            "window_size": 8, "kf_interval": 5}


class _Recorder:
    """Stands in for the torch / numpy modules inside slam_frontend: records norms and argmax inputs."""

    def __init__(self, mod, log):
        self._mod, self._log = mod, log

    def __getattr__(self, n):
        return getattr(self._mod, n)


def _wrap(log):
    tr = _Recorder(torch, log)
    tr.norm = lambda *a, **k: log.setdefault("norm", []).append(torch.norm(*a, **k)) or log["norm"][-1]
    npr = _Recorder(np, log)
    npr.argmax = lambda x, *a, **k: log.__setitem__("scores", list(x)) or np.argmax(x, *a, **k)
    return tr, npr


def se3(g, trans_scale):
    w = torch.randn(3, generator=g, dtype=torch.float64) * 0.3
    th = w.norm()
    K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + torch.sin(th) / th * K + (1 - torch.cos(th)) / th ** 2 * K @ K
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = R
    T[:3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 2 * trans_scale
    return T.float()


def depth_image(kind, g, H=12, W=16):
    d = 0.5 + 3.0 * torch.rand(H, W, generator=g)
    o = torch.rand(H, W, generator=g) * 0.2 + 0.85          # about half above 0.95
    if kind == "ties":
        d = torch.tensor([1.0, 1.5, 2.0, 2.5])[torch.randint(0, 4, (H, W), generator=g)]
    elif kind == "binade":                                   # [2, 4): the same exponent, low mantissa bits differ
        d = (torch.full((H, W), 2.0) + torch.randint(0, 24, (H, W), generator=g).float() * 2.0 ** -22)
    elif kind == "none":
        o = torch.rand(H, W, generator=g) * 0.95
    d[torch.rand(H, W, generator=g) < 0.1] = 0.0             # no depth
    d[0, 0] = float("nan")
    if kind != "none":
        o[0, 1] = 1.0
    n = int(((d > 0) & (o > 0.95)).sum())
    want = {"odd": 1, "even": 0}.get(kind)
    if want is not None and n % 2 != want:                   # flip one valid pixel off
        ys, xs = torch.nonzero((d > 0) & (o > 0.95), as_tuple=True)
        o[ys[0], xs[0]] = 0.5
    return d, o


def visibility(g, n, cur, overlap, density=0.6, empty=False):
    if empty:
        return torch.zeros(n, dtype=torch.bool)
    keep = torch.rand(n, generator=g) < overlap
    extra = torch.rand(n, generator=g) < density * (1 - overlap)
    return (cur & keep) | (~cur & extra)


# name: (N, window, cur, initialized, depth kind, overlaps (per window position), cur empty, translation scale,
#        single_thread, monocular)
CASES = {
    "uninit_below_reset": (300, [10, 5, 0], 15, False, "odd", [0.6, 0.2, 0.1], False, 0.6, True, True),
    "uninit_below_keep": (300, [10, 5, 0], 15, False, "even", [0.6, 0.8, 0.7], False, 0.6, True, True),
    "uninit_below_overlap": (300, [10, 5, 0], 15, False, "even", [0.97, 0.9, 0.9], False, 0.6, True, True),
    "uninit_check_time": (300, [10, 5, 0], 13, False, "odd", [0.5, 0.3, 0.3], False, 0.6, True, True),
    "full_evict": (250, [35, 30, 25, 20, 15, 10, 5, 0], 40, True, "odd", [0.7, 0.8, 0.75, 0.7, 0.8, 0.65, 0.7, 0.6],
                   False, 0.8, True, True),
    "full_cut_many": (250, [35, 30, 25, 20, 15, 10, 5, 0], 40, True, "ties",
                      [0.7, 0.05, 0.8, 0.02, 0.7, 0.05, 0.7, 0.8], False, 0.8, True, True),
    "full_dist_only": (250, [35, 30, 25, 20, 15, 10, 5, 0], 40, True, "binade",
                       [0.99, 0.8, 0.7, 0.7, 0.6, 0.6, 0.6, 0.6], False, 1.5, True, True),
    "full_empty_sets": (200, [35, 30, 25, 20, 15, 10, 5, 0], 40, True, "even", [0.5] * 8, True, 1.5, True, True),
    "full_no_depth": (200, [35, 30, 25, 20, 15, 10, 5, 0], 40, True, "none", [0.5] * 8, False, 1.5, True, True),
    "full_multi_thread": (250, [35, 30, 25, 20, 15, 10, 5, 0], 38, True, "odd", [0.5] * 8, False, 0.8, False, True),
    "init_rgbd_cut": (300, [20, 15, 10, 5], 25, False, "ties", [0.5, 0.3, 0.35, 0.2], False, 0.6, True, False),
    "over_full_cut_evict": (250, [45, 40, 35, 30, 25, 20, 15, 10, 5], 50, True, "odd",
                            [0.7, 0.7, 0.7, 0.7, 0.7, 0.7, 0.7, 0.7, 0.1], False, 0.8, True, True),
}


def run_case(name, spec, g):
    N, window, cur, initialized, kind, overlaps, cur_empty, tscale, single_thread, monocular = spec
    ids = [cur] + window
    cams = {i: types.SimpleNamespace(T=se3(g, tscale)) for i in ids}
    cur_vis = torch.rand(N, generator=g) < 0.6
    if cur_empty:
        cur_vis[:] = False
    rows = {kf: visibility(g, N, cur_vis, ov, empty=cur_empty and k % 2 == 0) for k, (kf, ov) in
            enumerate(zip(window, overlaps))}
    depth, opacity = depth_image(kind, g)
    med = SU.get_median_depth(depth[None], opacity[None])
    config = {"Training": dict(TRAINING)}
    self_ = types.SimpleNamespace(config=config, cameras=cams, median_depth=med, initialized=initialized)
    curr_visibility = cur_vis.long()
    occ = {kf: r.to(torch.uint8) for kf, r in rows.items()}
    log = {}
    F.torch, F.np = _wrap(log)
    try:
        # the run loop (:1914-1950)
        last_keyframe_idx = window[0]
        check_time = (cur - last_keyframe_idx) >= config["Training"]["kf_interval"]
        is_kf = F.FrontEnd.is_keyframe(self_, cur, last_keyframe_idx, curr_visibility, occ)
        dist = log["norm"][0]
        create_kf = is_kf
        if len(window) < config["Training"]["window_size"]:
            union = torch.logical_or(curr_visibility, occ[last_keyframe_idx]).count_nonzero()
            intersection = torch.logical_and(curr_visibility, occ[last_keyframe_idx]).count_nonzero()
            create_kf = check_time and intersection / union < config["Training"]["kf_overlap"]
        if single_thread:
            create_kf = check_time and create_kf
        create_kf = bool(create_kf)
        new_window, removed, reset = list(window), None, False
        if create_kf:
            new_window, removed = F.FrontEnd.add_to_window(self_, cur, curr_visibility, occ, list(window))
            reset = bool(monocular and not initialized and removed is not None)
    finally:
        F.torch, F.np = torch, np
    scores = np.full(len(window), -1.0)      # by window position; -1 where not a candidate
    if "scores" in log:   # the candidates: positions >= 2 of [cur] + window after the cutoff removal
        full = [cur] + list(window)
        cut_kf = next((kf for kf in full if kf not in new_window and kf != removed), None)
        for kf, sc in zip([kf for kf in full if kf != cut_kf][2:], log["scores"]):
            scores[window.index(kf)] = sc
    out = {"N": np.int32(N), "window": np.array(window, np.int32), "cur": np.int32(cur),
           "initialized": np.int32(initialized), "single_thread": np.int32(single_thread),
           "monocular": np.int32(monocular), "ids": np.array(ids, np.int32),
           "T": np.stack([cams[i].T.numpy() for i in ids]), "cur_vis": np.packbits(cur_vis.numpy()),
           "rows": np.packbits(np.stack([rows[kf].numpy() for kf in window]), axis=1),
           "depth": depth.numpy(), "opacity": opacity.numpy(),
           "median": med.numpy().astype(np.float32), "dist": dist.numpy().astype(np.float32),
           "is_kf": np.int32(bool(is_kf)), "create_kf": np.int32(create_kf),
           "new_window": np.array(new_window, np.int32), "removed": np.int32(-1 if removed is None else removed),
           "reset": np.int32(reset), "scores": scores}
    print(f"{name:22s} median {float(med):.6g} create {create_kf} removed {removed} reset {reset} "
          f"window {new_window} scores {'yes' if 'scores' in log else 'no'}")
    return out


def main():
    g = torch.Generator().manual_seed(20261016)
    out = {"names": np.array(list(CASES)), "training": np.array([TRAINING[k] for k in sorted(TRAINING)]),
           "training_keys": np.array(sorted(TRAINING))}
    for name, spec in CASES.items():
        for k, v in run_case(name, spec, g).items():
            out[f"{name}_{k}"] = v
    path = os.path.join(HERE, "keyframe_policy_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
