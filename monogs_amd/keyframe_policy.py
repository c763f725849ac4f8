"""Keyframe selection and window management: the reference frontend's policy
(/root/reference utils/slam_frontend.py: is_keyframe :1692-1720, add_to_window :1722-1783, the run
loop's decision :1914-1956; get_median_depth utils/slam_utils.py:286-297).

Two implementations of the same decision:
  * the torch mirrors below (`median_depth`, `is_keyframe`, `add_to_window`, `loop_decision`), written the
    reference's way - they run on CPU or GPU tensors and are the yardstick of the native path;
  * `KeyframePolicy(native=True)`: one `mgs_keyframe_decide` call (keyframe_policy.hip: three launches - a radix
    select of the median depth, the covisibility counts, the decision) and one device-to-host copy of the record.

The window is ordered newest first (window[0] is the last keyframe), as the reference's current_window.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Mapping, Optional

import numpy as np
import torch

from . import _cabi

# configs/mono/tum/base_config.yaml:33-42
DEFAULT_TRAINING = {"kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3,
                    "window_size": 8, "kf_interval": 5}
N_DONT_TOUCH = 2


def _T(cam):
    return cam.T if hasattr(cam, "T") else cam


# ---- torch mirrors of the reference ------------------------------------------------------------------------------
def median_depth(depth, opacity):
    """get_median_depth(depth, opacity): torch.median (the lower median) of depth where depth > 0 and opacity > 0.95;
    NaN when no pixel is valid."""
    depth = depth.detach().clone()
    valid = torch.logical_and(depth > 0, opacity.detach() > 0.95)
    return depth[valid].median()


def is_keyframe(config, cameras, median_depth, cur_frame_idx, last_keyframe_idx, cur_frame_visibility_filter,
                occ_aware_visibility, trace: Optional[dict] = None):
    """FrontEnd.is_keyframe with the frontend's state passed in (config, cameras[idx].T, median_depth).  `trace`
    (optional) receives dist and the union-based ratio."""
    kf_translation = config["Training"]["kf_translation"]
    kf_min_translation = config["Training"]["kf_min_translation"]
    kf_overlap = config["Training"]["kf_overlap"]
    pose_CW = _T(cameras[cur_frame_idx])
    last_kf_WC = torch.linalg.inv(_T(cameras[last_keyframe_idx]))
    dist = torch.norm((pose_CW @ last_kf_WC)[0:3, 3])
    dist_check = dist > kf_translation * median_depth
    dist_check2 = dist > kf_min_translation * median_depth
    union = torch.logical_or(cur_frame_visibility_filter, occ_aware_visibility[last_keyframe_idx]).count_nonzero()
    intersection = torch.logical_and(cur_frame_visibility_filter,
                                     occ_aware_visibility[last_keyframe_idx]).count_nonzero()
    point_ratio_2 = intersection / union
    if trace is not None:
        trace["dist"], trace["overlap"] = dist, point_ratio_2
    return (point_ratio_2 < kf_overlap and dist_check2) or dist_check


def add_to_window(config, cameras, initialized, cur_frame_idx, cur_frame_visibility_filter, occ_aware_visibility,
                  window, trace: Optional[dict] = None):
    """FrontEnd.add_to_window -> (new window, removed keyframe or None).  `trace` (optional) receives the
    Szymkiewicz-Simpson ratios {keyframe: ratio} and the eviction scores {keyframe: score}."""
    window = [cur_frame_idx] + list(window)
    to_remove = []
    removed_frame = None
    for i in range(N_DONT_TOUCH, len(window)):
        kf_idx = window[i]
        intersection = torch.logical_and(cur_frame_visibility_filter, occ_aware_visibility[kf_idx]).count_nonzero()
        denom = min(cur_frame_visibility_filter.count_nonzero(), occ_aware_visibility[kf_idx].count_nonzero())
        point_ratio_2 = intersection / denom
        if trace is not None:
            trace.setdefault("ss_ratio", {})[kf_idx] = point_ratio_2
        cut_off = config["Training"]["kf_cutoff"] if "kf_cutoff" in config["Training"] else 0.4
        if not initialized:
            cut_off = 0.4
        if point_ratio_2 <= cut_off:
            to_remove.append(kf_idx)
    if to_remove:
        window.remove(to_remove[-1])
        removed_frame = to_remove[-1]
    kf_0_WC = torch.linalg.inv(_T(cameras[cur_frame_idx]))
    if len(window) > config["Training"]["window_size"]:
        inv_dist = []
        for i in range(N_DONT_TOUCH, len(window)):
            inv_dists = []
            kf_i_CW = _T(cameras[window[i]])
            for j in range(N_DONT_TOUCH, len(window)):
                if i == j:
                    continue
                kf_j_WC = torch.linalg.inv(_T(cameras[window[j]]))
                T_CiCj = kf_i_CW @ kf_j_WC
                inv_dists.append(1.0 / (torch.norm(T_CiCj[0:3, 3]) + 1e-6).item())
            T_CiC0 = kf_i_CW @ kf_0_WC
            k = torch.sqrt(torch.norm(T_CiC0[0:3, 3])).item()
            inv_dist.append(k * sum(inv_dists))
        if trace is not None:
            trace["scores"] = dict(zip(window[N_DONT_TOUCH:], inv_dist))
        idx = np.argmax(inv_dist)
        removed_frame = window[N_DONT_TOUCH + idx]
        window.remove(removed_frame)
    return window, removed_frame


def loop_decision(config, cameras, median_depth, initialized, monocular, single_thread, cur_frame_idx, window,
                  curr_visibility, occ_aware_visibility, trace: Optional[dict] = None):
    """The run loop's keyframe decision (:1914-1950) for one tracked frame ->
    {"create_kf", "window", "removed", "reset"} (window unchanged unless a keyframe is created)."""
    tr = config["Training"]
    last_keyframe_idx = window[0]
    check_time = (cur_frame_idx - last_keyframe_idx) >= tr["kf_interval"]
    create_kf = is_keyframe(config, cameras, median_depth, cur_frame_idx, last_keyframe_idx, curr_visibility,
                            occ_aware_visibility, trace)
    if len(window) < tr["window_size"]:
        union = torch.logical_or(curr_visibility, occ_aware_visibility[last_keyframe_idx]).count_nonzero()
        intersection = torch.logical_and(curr_visibility, occ_aware_visibility[last_keyframe_idx]).count_nonzero()
        point_ratio = intersection / union
        create_kf = check_time and point_ratio < tr["kf_overlap"]
    if single_thread:
        create_kf = check_time and create_kf
    create_kf = bool(create_kf)
    new_window, removed, reset = list(window), None, False
    if create_kf:
        new_window, removed = add_to_window(config, cameras, initialized, cur_frame_idx, curr_visibility,
                                            occ_aware_visibility, window, trace)
        reset = bool(monocular and not initialized and removed is not None)
    return {"create_kf": create_kf, "window": new_window, "removed": removed, "reset": reset}


# ---- the policy object --------------------------------------------------------------------------------------------
@dataclass
class KeyframeDecision:
    """One frame's decision.  `window` is the window after the frame (unchanged unless create_kf); `removed` the
    keyframe add_to_window dropped (None if none); the numbers are those of the native record (the torch path fills
    median_depth only)."""
    create_kf: bool
    window: List[int]
    removed: Optional[int]
    reset: bool
    median_depth: float = float("nan")
    n_valid: int = -1
    dist: float = float("nan")
    overlap: float = float("nan")
    n_cur: int = -1
    ss_ratio: List[float] = field(default_factory=list)
    scores: List[float] = field(default_factory=list)
    n_row: List[int] = field(default_factory=list)
    n_inter: List[int] = field(default_factory=list)
    flags: int = 0


class KeyframePolicy:
    """The frontend's keyframe policy with its `initialized` flag (set once the window has been full; `not monocular`
    from the start and after a reset).  `config`: a reference-shaped dict; Training.{kf_translation,
    kf_min_translation, kf_overlap, kf_cutoff, window_size, kf_interval} default to configs/mono/tum/base_config.yaml.
    native=True: the decision is one mgs_keyframe_decide call and one device-to-host copy; else the torch mirrors."""

    def __init__(self, config: Optional[dict] = None, monocular: bool = True, single_thread: bool = True,
                 native: bool = True):
        tr = dict(DEFAULT_TRAINING)
        tr.update({k: v for k, v in ((config or {}).get("Training") or {}).items() if k in DEFAULT_TRAINING})
        self.config = {"Training": tr}
        self.monocular, self.single_thread, self.native = bool(monocular), bool(single_thread), bool(native)
        self.initialized = not self.monocular
        self._scratch = None
        self._result = None
        self._host = None

    @property
    def window_size(self) -> int:
        return int(self.config["Training"]["window_size"])

    @property
    def kf_interval(self) -> int:
        return int(self.config["Training"]["kf_interval"])

    def reset_state(self):
        """frontend.initialize (:236-238): the flag after a (re-)initialisation."""
        self.initialized = not self.monocular

    def decide(self, cur_idx: int, cameras: Mapping, window: List[int], tracker,
               occ_aware_visibility: Dict[int, torch.Tensor]) -> KeyframeDecision:
        """The decision for tracked frame `cur_idx`.  `cameras[i].T`: world-to-camera poses (the current frame's and
        the window's); `tracker`: its n_touched / depth / opacity rendered at the frame's final pose (NativeTracker
        after run()); `occ_aware_visibility[kf]`: uint8 [N] rows of the window's keyframes."""
        window = [int(k) for k in window]
        if not window:
            raise ValueError("the keyframe window is empty")
        self.initialized = self.initialized or len(window) == self.window_size     # :1880-1882
        n = tracker.n_touched.numel()
        for kf in window:
            row = occ_aware_visibility.get(kf)
            if row is None:
                raise ValueError(f"keyframe {kf} has no visibility row")
            if row.numel() != n:
                raise ValueError(f"keyframe {kf}: visibility row has {row.numel()} entries, the current frame "
                                 f"renders {n} Gaussians")
        if self.native:
            return self._decide_native(cur_idx, cameras, window, tracker, occ_aware_visibility, self.initialized)
        return self._decide_torch(cur_idx, cameras, window, tracker, occ_aware_visibility, self.initialized)

    def _decide_torch(self, cur_idx, cameras, window, tracker, occ, initialized) -> KeyframeDecision:
        med = median_depth(tracker.depth, tracker.opacity)
        vis = (tracker.n_touched > 0).long()
        d = loop_decision(self.config, cameras, med, initialized, self.monocular, self.single_thread, cur_idx,
                          window, vis, occ)
        return KeyframeDecision(d["create_kf"], d["window"], d["removed"], d["reset"], median_depth=float(med))

    def _buffers(self, dev, nbytes):
        if self._scratch is None or self._scratch.device != dev or self._scratch.numel() < nbytes:
            # zero-filled once: the kernels leave the histograms and the ticket as they found them
            self._scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        if self._result is None or self._result.device != dev:
            self._result = torch.zeros(C.sizeof(_cabi.KeyframeResult), dtype=torch.uint8, device=dev)
            self._host = torch.empty(C.sizeof(_cabi.KeyframeResult), dtype=torch.uint8, pin_memory=True)

    def native_args(self, cur_idx, cameras, window, tracker, occ, initialized):
        """The mgs_keyframe_args of one decision (and the tensors its pointers refer to)."""
        tr = self.config["Training"]
        dev = tracker.n_touched.device
        if dev.type != "cuda":
            raise RuntimeError("mgs_keyframe_decide runs on the GPU only (HIP kernels, gfx950)")
        W = len(window)
        if W > _cabi.KF_MAX_WINDOW:
            raise ValueError(f"window of {W} keyframes: the native policy takes at most {_cabi.KF_MAX_WINDOW}")
        n_touched = tracker.n_touched.reshape(-1).contiguous()
        depth = tracker.depth.reshape(-1).contiguous()
        opacity = tracker.opacity.reshape(-1).contiguous()
        if n_touched.dtype != torch.int32 or depth.dtype != torch.float32 or opacity.dtype != torch.float32:
            raise ValueError("n_touched must be int32, depth and opacity float32")
        poses = [_T(cameras[cur_idx])] + [_T(cameras[kf]) for kf in window]
        poses = [T.to(dev, torch.float32).contiguous() for T in poses]
        rows = [occ[kf].reshape(-1) for kf in window]
        rows = [r.view(torch.uint8) if r.dtype == torch.bool else r for r in rows]
        if any(r.dtype != torch.uint8 for r in rows):
            raise ValueError("visibility rows must be uint8")
        rows = [r.contiguous() for r in rows]
        N, HW = n_touched.numel(), depth.numel()
        nbytes = int(_cabi.lib().mgs_keyframe_scratch_bytes(N, HW, W))
        if nbytes == 0:
            raise ValueError(f"mgs_keyframe_scratch_bytes({N}, {HW}, {W}) refused the sizes")
        self._buffers(dev, nbytes)
        a = _cabi.KeyframeArgs()
        a.num_gaussians, a.num_pixels, a.window_len, a.window_size = N, HW, W, int(tr["window_size"])
        a.check_time = int(cur_idx - window[0] >= tr["kf_interval"])
        a.initialized, a.monocular, a.single_thread = int(initialized), int(self.monocular), int(self.single_thread)
        a.kf_translation, a.kf_min_translation = float(tr["kf_translation"]), float(tr["kf_min_translation"])
        a.kf_overlap, a.kf_cutoff = float(tr["kf_overlap"]), float(tr["kf_cutoff"])
        a.n_touched, a.depth, a.opacity = n_touched.data_ptr(), depth.data_ptr(), opacity.data_ptr()
        a.T_cur = poses[0].data_ptr()
        for i in range(W):
            a.T_window[i] = poses[1 + i].data_ptr()
            a.visibility[i] = rows[i].data_ptr()
            a.visibility_len[i] = rows[i].numel()
        a.scratch, a.result = self._scratch.data_ptr(), self._result.data_ptr()
        return a, (n_touched, depth, opacity, poses, rows)

    def read_record(self) -> _cabi.KeyframeResult:
        """The device record of the last call (one device-to-host copy; synchronises the current stream)."""
        self._host.copy_(self._result, non_blocking=True)
        torch.cuda.current_stream(self._result.device).synchronize()
        return _cabi.KeyframeResult.from_buffer_copy(self._host.numpy().tobytes())

    def _decide_native(self, cur_idx, cameras, window, tracker, occ, initialized) -> KeyframeDecision:
        a, keep = self.native_args(cur_idx, cameras, window, tracker, occ, initialized)
        stream = C.c_void_p(torch.cuda.current_stream(self._result.device).cuda_stream)
        _cabi.check(_cabi.lib().mgs_keyframe_decide(C.byref(a), stream), "mgs_keyframe_decide")
        r = self.read_record()
        del keep
        return self.from_record(r, cur_idx, window)

    @staticmethod
    def from_record(r, cur_idx, window) -> KeyframeDecision:
        W = len(window)
        new_window, removed = list(window), None
        if r.create_kf:
            gone = {r.removed_cutoff, r.removed_evict}
            new_window = [cur_idx] + [kf for i, kf in enumerate(window) if i not in gone]
            removed = window[r.removed] if r.removed >= 0 else None
        return KeyframeDecision(bool(r.create_kf), new_window, removed, bool(r.reset), median_depth=float(r.median_depth),
                                n_valid=int(r.n_valid), dist=float(r.dist), overlap=float(r.overlap), n_cur=int(r.n_cur),
                                ss_ratio=[float(x) for x in r.ss_ratio[:W]], scores=[float(x) for x in r.score[:W]],
                                n_row=[int(x) for x in r.n_row[:W]], n_inter=[int(x) for x in r.n_inter[:W]],
                                flags=int(r.flags))
