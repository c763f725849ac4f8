"""Stereo depth at the EuRoC size (752x480) on the GPU box:

    timeout -k 10 400 python profiles/stereo_depth_profile.py > profiles/stereo_depth_profile.txt

  (a) StereoMatcher.compute on a rectified uint8 grey pair resident on the device: wall clock per pair with a final
      synchronise, the median of 50 calls after 10 warm-ups with quartiles and extremes;
  (b) the same on a RAW pair through two rectification maps (a synthetic distorted stereo calibration, the maps built
      on the device once): the remap's cost is the difference;
  (c) per kernel, from the library's own event timing (mgs_profile_enable: an event pair around every launch, which
      serialises the launches - the kernels' own durations, not their share of the wall clock), 20 calls each way;
  (d) the NumPy mirror on the host CPU, once, labelled as such - a statement of the contract, not an optimised
      baseline - and whether the two agree bit for bit at this size;
  (e) the scratch size.
The pair: uniform noise seen through four fronto-parallel planes (tests/stereo_cases.planes_pair's recipe)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W = 480, 752


def samples_us(fn, warm, timed):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def summary(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median_us": round(statistics.median(xs), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1),
            "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def calibration():
    def cam(fx, cx, k1):
        raw = {"fx": fx, "fy": fx, "cx": cx, "cy": 248.0, "k1": k1, "k2": 0.07, "p1": 2e-4, "p2": 2e-5, "k3": 0.0}
        opt = {"fx": 435.2, "fy": 435.2, "cx": 367.4, "cy": 252.2}
        return {"raw": raw, "opt": opt, "R": {"data": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]}}
    return {"cam0": cam(458.6, 367.2, -0.283), "cam1": cam(457.3, 379.9, -0.284), "distorted": True}


def kernel_times(fn, calls=20):
    import torch
    from monogs_amd import _cabi
    fn()
    torch.cuda.synchronize()
    _cabi.profile_enable(True)
    _cabi.profile_read()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    rows = _cabi.profile_read()
    _cabi.profile_enable(False)
    return {k: round(ms * 1e3 / n, 1) for k, (ms, n) in rows.items() if k.startswith("sd_")}


def main():
    import numpy as np
    import torch
    from monogs_amd import _cabi
    from monogs_amd import stereo_depth as SD
    import stereo_cases as SC
    dev = torch.device("cuda:0")
    left, right, _ = SC.planes_pair(H, W, seed=4, split_x=400)
    gl, gr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    plain = SD.StereoMatcher(H, W, dev)
    remapped = SD.StereoMatcher(H, W, dev, calibration=calibration())
    out = {"H": H, "W": W, "scratch_bytes": int(_cabi.lib().mgs_stereo_scratch_bytes(H, W))}
    print(f"{W}x{H}, 64 disparities; scratch {out['scratch_bytes'] / 2**20:.1f} MiB")
    f_plain, f_remap = (lambda: plain.compute(gl, gr)), (lambda: remapped.compute(gl, gr))
    a1, b1 = samples_us(f_plain, 10, 25), samples_us(f_remap, 10, 25)
    a2, b2 = samples_us(f_plain, 0, 25), samples_us(f_remap, 0, 25)
    out["rectified_pair"], out["raw_pair_remapped"] = summary(a1 + a2), summary(b1 + b2)
    for name in ("rectified_pair", "raw_pair_remapped"):
        s = out[name]
        print(f"{name}: {s['median_us']} us per pair (quartiles {s['q1_us']} .. {s['q3_us']}, range {s['min_us']} .. "
              f"{s['max_us']})")
    out["kernels_us_rectified"], out["kernels_us_remapped"] = kernel_times(f_plain), kernel_times(f_remap)
    vol = H * (W - 64) * 64
    for name in ("kernels_us_rectified", "kernels_us_remapped"):
        print(f"{name} (event-timed, serialised): total {sum(out[name].values()):.1f} us")
        for k, us in sorted(out[name].items(), key=lambda kv: -kv[1]):
            print(f"    {k}: {us} us")
    print(f"the cost volume has {vol / 1e6:.1f} M entries: C {vol * 2 / 2**20:.1f} MiB, the five L volumes "
          f"{vol * 10 / 2**20:.1f} MiB")
    res = plain.compute(gl, gr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    disp16, depth = SD.stereo_sgbm_numpy(left, right)
    out["numpy_mirror_cpu_s"] = round(time.perf_counter() - t0, 2)
    out["bit_equal_to_mirror"] = bool(np.array_equal(res["disp16"].cpu().numpy(), disp16)
                                      and np.array_equal(res["depth"][0].cpu().numpy().view(np.int32),
                                                         depth.view(np.int32)))
    out["valid_share"] = round(float((disp16 >= 0).mean()), 4)
    print(f"NumPy mirror on the host CPU (not a GPU figure, not an optimised baseline): {out['numpy_mirror_cpu_s']} s; "
          f"native output bit-equal to it: {out['bit_equal_to_mirror']}; {100 * out['valid_share']:.1f} % of the pixels "
          "hold a disparity")
    print(json.dumps({"stereo_depth_profile": out}))


if __name__ == "__main__":
    main()
