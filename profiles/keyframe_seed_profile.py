"""Keyframe seeding on the GPU box, the torch path against the native call:

    timeout -k 10 600 python profiles/keyframe_seed_profile.py > profiles/keyframe_seed_profile.txt && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o seed -- \
        python profiles/keyframe_seed_profile.py --native-only

Monocular with rendered depth (mode 0), at 640x480 with down-sample 64 and 32 and at 1200x680 with 64:
  (a) the torch path: slam_surrogate.keyframe_depth + keyframe_init.create_pcd_from_image_and_depth, up to but not
      including the append; wall clock per call with a final synchronise;
  (b) KeyframeSeeder.seed: mgs_keyframe_seed including its one read of the record; same protocol.
Each figure is the median of 50 calls after 10 warm-ups, with the quartiles and extremes of the 50 (the spread).  The
host synchronisations of (a) are counted with torch's sync debug mode (one warning per synchronising operator); (b)
synchronises once, inside the library, which that mode does not see.  --native-only runs (b) alone, 20 calls per
shape, for a kernel trace.  Prints one line per shape and, last, one JSON line with everything."""
import json
import os
import statistics
import sys
import time
import types
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monogs_amd import keyframe_seed as KS  # noqa: E402
from monogs_amd.keyframe_init import create_pcd_from_image_and_depth  # noqa: E402
from monogs_amd.slam_surrogate import keyframe_depth  # noqa: E402

SHAPES = ((480, 640, 64), (480, 640, 32), (680, 1200, 64))


def samples_us(fn, warm=10, timed=50):
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


def count_syncs(fn):
    """Synchronising torch operators in one call of fn (None when the build has no sync debug mode)."""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(x.message).lower() for x in w)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def inputs(H, W, dev):
    g = torch.Generator(device=dev).manual_seed(H + W)
    image = 0.05 + 0.9 * torch.rand(3, H, W, device=dev, generator=g)
    image[:, :8, :] = 0.0
    depth = 1.0 + 3.0 * torch.rand(1, H, W, device=dev, generator=g)
    depth[torch.rand(1, H, W, device=dev, generator=g) < 0.05] = 0.0
    opacity = 0.9 + 0.1 * torch.rand(1, H, W, device=dev, generator=g)
    T = torch.eye(4, device=dev)
    T[:3, 3] = torch.tensor([0.1, -0.2, 0.3], device=dev)
    cam = types.SimpleNamespace(fx=0.82 * W, fy=0.82 * W, cx=0.5 * W, cy=0.5 * H, T=T, exposure_eps=1e-8,
                                exposure_a=torch.tensor([1.0], device=dev), exposure_b=torch.tensor([0.0], device=dev))
    return cam, image, depth, opacity


def main():
    native_only = "--native-only" in sys.argv[1:]
    dev = torch.device("cuda:0")
    out = []
    for H, W, ds in SHAPES:
        cam, image, depth, opacity = inputs(H, W, dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        seeder = KS.KeyframeSeeder(H, W, dev, {"Dataset": {"pcd_downsample": ds, "pcd_downsample_init": ds}})
        seeds = iter(range(1, 1 << 30))

        def torch_path():
            d = keyframe_depth(image, depth, opacity, None, gen)
            return create_pcd_from_image_and_depth(cam, image, d, downsample_factor=ds, generator=gen)

        def native():
            return seeder.seed(cam, image, depth, opacity, KS.MODE_RENDERED, False, next(seeds))

        if native_only:
            for _ in range(20):
                native()
            torch.cuda.synchronize()
            continue
        rec = native()[-1]
        row = {"H": H, "W": W, "downsample": ds, "points": int(rec.num_points), "n_depth": int(rec.n_depth),
               "points_torch_path": int(torch_path()[0].shape[0])}
        # alternate the two paths so that a drift of the host hits both
        a1, b1 = samples_us(torch_path, 10, 25), samples_us(native, 10, 25)
        a2, b2 = samples_us(torch_path, 0, 25), samples_us(native, 0, 25)
        row["torch_path"], row["native"] = summary(a1 + a2), summary(b1 + b2)
        row["torch_path_host_syncs"] = count_syncs(torch_path)
        row["native_host_syncs"] = 1
        row["native_torch_visible_syncs"] = count_syncs(native)
        a, b = row["torch_path"], row["native"]
        row["speedup_median"] = round(a["median_us"] / b["median_us"], 2)
        row["native_below_torch_by_more_than_its_spread"] = bool(a["median_us"] - b["median_us"] > a["q3_us"] - a["q1_us"]
                                                                 and b["q3_us"] < a["q1_us"])
        print(f"{W}x{H} down-sample {ds} ({row['points']} points): torch path {a['median_us']} us (quartiles "
              f"{a['q1_us']} .. {a['q3_us']}, range {a['min_us']} .. {a['max_us']}; {row['torch_path_host_syncs']} "
              f"synchronising operators), native {b['median_us']} us (quartiles {b['q1_us']} .. {b['q3_us']}, range "
              f"{b['min_us']} .. {b['max_us']}; one read), x{row['speedup_median']}")
        out.append(row)
    if not native_only:
        print(json.dumps({"keyframe_seed_profile": out}))


if __name__ == "__main__":
    main()
