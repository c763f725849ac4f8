"""The keyframe decision per frame on the GPU box, native against the torch mirror:

    python profiles/keyframe_policy_profile.py

At 300 k Gaussians, 640x480 and a full window of 8 keyframes (so every rule runs: is_keyframe, add_to_window's
cutoff scan and the inverse-distance eviction), times
  * KeyframePolicy(native=True).decide: mgs_keyframe_decide (three launches) + the one device-to-host read of the
    record, wall clock per decision;
  * KeyframePolicy(native=False).decide: the reference-shaped torch mirror on the same device tensors, wall clock;
  * the three launches alone by device events (back to back, no read), and per kernel by the library's timer.
Prints one line and, last, one JSON line with everything."""
import ctypes as C
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import _cabi  # noqa: E402
from monogs_amd import keyframe_policy as KP  # noqa: E402
from monogs_amd.pose import SE3_exp  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "profiles"))
from rgbd_tracking_profile import device_time_us, kernels_us  # noqa: E402


def wall_us(fn, warm, timed):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(timed):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / timed * 1e6


def main():
    dev = torch.device("cuda:0")
    N, W, H, win = 300_000, 640, 480, 8
    g = torch.Generator(device=dev).manual_seed(0)
    n_touched = torch.randint(-2, 4, (N,), device=dev, generator=g, dtype=torch.int32)
    depth = 0.5 + 3.0 * torch.rand(1, H, W, device=dev, generator=g)
    opacity = torch.rand(1, H, W, device=dev, generator=g) * 0.2 + 0.85
    window = [40 - 5 * i for i in range(win)]
    occ = {kf: (torch.rand(N, device=dev, generator=g) < 0.5).to(torch.uint8) for kf in window}
    cams = {k: types.SimpleNamespace(T=SE3_exp(torch.tensor([0.05 * k, -0.01 * k, 0.02 * k, 0.004 * k, 0.0, 0.001 * k]))
                                     .to(dev).contiguous()) for k in window + [45]}
    trk = types.SimpleNamespace(n_touched=n_touched, depth=depth, opacity=opacity)
    nat = KP.KeyframePolicy(monocular=True)
    mir = KP.KeyframePolicy(monocular=True, native=False)
    dn, dm = nat.decide(45, cams, window, trk, occ), mir.decide(45, cams, window, trk, occ)
    assert (dn.create_kf, dn.window, dn.removed) == (dm.create_kf, dm.window, dm.removed), (dn, dm)
    out = {"gaussians": N, "W": W, "H": H, "window": win, "create_kf": dn.create_kf, "removed": dn.removed,
           "evicted_by_score": max(dn.scores) > 0}
    out["native_decide_wall_us"] = round(wall_us(lambda: nat.decide(45, cams, window, trk, occ), 20, 200), 1)
    out["torch_mirror_decide_wall_us"] = round(wall_us(lambda: mir.decide(45, cams, window, trk, occ), 5, 50), 1)
    a, keep = nat.native_args(45, cams, window, trk, occ, True)
    lib = _cabi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: lib.mgs_keyframe_decide(C.byref(a), stream)
    out["native_launches_device_us"] = round(device_time_us(call, 20, 500), 2)
    out["kernels_us"] = kernels_us(call, 100)
    out["speedup_wall"] = round(out["torch_mirror_decide_wall_us"] / out["native_decide_wall_us"], 1)
    print(f"{N} Gaussians @ {W}x{H}, window {win}: native decide {out['native_decide_wall_us']} us wall "
          f"({out['native_launches_device_us']} us of device time for the three launches), torch mirror "
          f"{out['torch_mirror_decide_wall_us']} us wall")
    print(json.dumps({"keyframe_policy_profile": out}))


if __name__ == "__main__":
    main()
