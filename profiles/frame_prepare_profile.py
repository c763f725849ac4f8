"""Frame preparation on the GPU box, the torch mirror against the native call:

    timeout -k 10 300 python profiles/frame_prepare_profile.py > profiles/frame_prepare_profile.txt
    for c in 0 1 2 3 4; do for p in native mirror; do
      timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d <dir>/trace_${p}_$c -o run -- \
          python profiles/frame_prepare_profile.py --$p-only --config $c
    done; done
    python profiles/frame_prepare_profile.py --summarise <dir> >> profiles/frame_prepare_profile.txt
        (also writes <dir>/frame_prepare_kernel_stats.csv)

Five configurations, inputs resident on the device in the format named:
  0  640x480, global mode (Dataset.type tum, edge_threshold 1.1), uint8 [H,W,3] image
  1  640x480, global mode, float [3,H,W] image
  2  1200x680, patch mode (Dataset.type replica, edge_threshold 4), uint8 image and uint16 depth (depth_scale 6553.5)
  3  configuration 0 undistorted: fr1_desk's calibration (Dataset.Calibration, distorted: True), the map built on the
     device once, every call mgs_frame_prepare_remapped
  4  configuration 2 undistorted: the same coefficients, the intrinsics scaled to 1200x680
     (3 and 4 also time the un-remapped native call of the same build on the same input: the cost of the remap is the
     difference; their mirror is prepare_frame_torch(remap=...))
  (a) frame_prepare.prepare_frame_torch on the device: wall clock per call with a final synchronise;
  (b) FramePreparer.prepare: one mgs_frame_prepare call; same protocol.
Each figure is the median of 50 calls after 10 warm-ups, the two paths alternating in blocks of 25, with the quartiles
and extremes of the 50 (the spread).  Synchronising torch operators are counted with torch's sync debug mode.
--native-only / --mirror-only run 20 calls of one configuration and nothing else, for a kernel trace: the trace's
dispatch count over 20 is the launches per call; --summarise turns the traces into the per-kernel table.

The block that ends frame_prepare_profile.txt ("the un-remapped call against the parent commit's build ...") is not
printed by a mode of this script.  Its procedure: check the parent commit out into a directory of its own and build it
there; on ONE box run `python profiles/frame_prepare_profile.py` from the parent's directory and from this one
alternately, twice each; copy the `native` median and quartiles of configurations 0 / 1 / 2 from each output (and, from
this build's outputs, the rows of configurations 3 and 4) into that block by hand."""
import csv
import glob
import json
import os
import statistics
import sys
import time
import warnings

CALLS_TRACED = 20
CONFIGS = (
    {"name": "640x480 global uint8", "H": 480, "W": 640, "type": "tum", "edge_threshold": 1.1, "u8": True, "depth": False},
    {"name": "640x480 global float", "H": 480, "W": 640, "type": "tum", "edge_threshold": 1.1, "u8": False, "depth": False},
    {"name": "1200x680 patch uint8 + uint16 depth", "H": 680, "W": 1200, "type": "replica", "edge_threshold": 4.0,
     "u8": True, "depth": True},
    {"name": "640x480 global uint8, remapped (fr1_desk)", "H": 480, "W": 640, "type": "tum", "edge_threshold": 1.1,
     "u8": True, "depth": False, "remap": True},
    {"name": "1200x680 patch uint8 + uint16 depth, remapped (fr1_desk scaled)", "H": 680, "W": 1200, "type": "replica",
     "edge_threshold": 4.0, "u8": True, "depth": True, "remap": True},
)
FR1_DESK = {"fx": 517.3, "fy": 516.5, "cx": 318.6, "cy": 255.3, "k1": 0.2624, "k2": -0.9531, "p1": -0.0054,
            "p2": 0.0026, "k3": 1.1633, "width": 640, "height": 480, "distorted": True}
DEPTH_SCALE = 6553.5


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


def count_syncs(fn):
    """Synchronising torch operators in one call of fn (None when the build has no sync debug mode)."""
    import torch
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


def inputs(cfg, dev):
    """A frame with edges at every scale (blocks over noise) and a dark corner, in the configuration's formats."""
    import torch
    H, W = cfg["H"], cfg["W"]
    g = torch.Generator().manual_seed(H + W)
    coarse = torch.rand(3, H // 12 + 2, W // 12 + 2, generator=g)
    img = coarse.repeat_interleave(12, 1).repeat_interleave(12, 2)[:, :H, :W] * 0.7 + 0.15
    img = (img + 0.02 * torch.randn(3, H, W, generator=g)).clamp(0.05, 0.95)
    img[:, :H // 8, :W // 8] = 0.0
    u8 = img.mul(255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    image = u8.to(dev) if cfg["u8"] else (u8.permute(2, 0, 1).float() / 255.0).contiguous().to(dev)
    depth = None
    if cfg["depth"]:
        d = (torch.rand(H, W, generator=g) * 30000 + 3000).to(torch.int32).numpy().astype("uint16")
        depth = torch.from_numpy(d.view("int16")).view(torch.uint16).to(dev)
    return image, depth


def paths(cfg, dev):
    import torch
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from monogs_amd import frame_prepare as FP
    image, depth = inputs(cfg, dev)
    scale = DEPTH_SCALE if cfg["depth"] else None
    config = {"Training": {"edge_threshold": cfg["edge_threshold"]}, "Dataset": {"type": cfg["type"]}}
    plain = FP.FramePreparer(cfg["H"], cfg["W"], dev, config)
    P = plain
    if cfg.get("remap"):
        sx, sy = cfg["W"] / 640.0, cfg["H"] / 480.0
        cal = dict(FR1_DESK, fx=FR1_DESK["fx"] * sx, fy=FR1_DESK["fy"] * sy, cx=FR1_DESK["cx"] * sx,
                   cy=FR1_DESK["cy"] * sy, width=cfg["W"], height=cfg["H"])
        P = FP.FramePreparer(cfg["H"], cfg["W"], dev, config, calibration=cal)

    def mirror():
        return FP.prepare_frame_torch(image, depth, dataset_type=cfg["type"], edge_threshold=cfg["edge_threshold"],
                                      depth_scale=scale, remap=P.map_q5)

    def native():
        return P.prepare(image, depth, scale)

    def unremapped():
        return plain.prepare(image, depth, scale)

    return mirror, native, unremapped


def measure():
    import torch
    dev = torch.device("cuda:0")
    out = []
    for cfg in CONFIGS:
        mirror, native, unremapped = paths(cfg, dev)
        a, b = mirror(), native()
        torch.cuda.synchronize()
        row = {"config": cfg["name"], "H": cfg["H"], "W": cfg["W"],
               "mask_pixels_differing": int((a["grad_mask"] != b["grad_mask"]).sum()),
               "edge_mask_cover": round(float(b["grad_mask"].mean()), 4)}
        # alternate the two paths so that a drift of the host hits both
        a1, b1 = samples_us(mirror, 10, 25), samples_us(native, 10, 25)
        c1 = samples_us(unremapped, 10, 25) if cfg.get("remap") else None
        a2, b2 = samples_us(mirror, 0, 25), samples_us(native, 0, 25)
        row["torch_mirror"], row["native"] = summary(a1 + a2), summary(b1 + b2)
        if c1 is not None:
            row["image_bits_equal_mirror"] = bool(torch.equal(a["image"], b["image"]))
            row["native_unremapped"] = summary(c1 + samples_us(unremapped, 0, 25))
        row["torch_mirror_host_syncs"], row["native_host_syncs"] = count_syncs(mirror), count_syncs(native)
        a, b = row["torch_mirror"], row["native"]
        row["speedup_median"] = round(a["median_us"] / b["median_us"], 2)
        row["native_below_mirror_by_more_than_its_spread"] = bool(
            a["median_us"] - b["median_us"] > a["q3_us"] - a["q1_us"] and b["q3_us"] < a["q1_us"])
        print(f"{cfg['name']}: torch mirror {a['median_us']} us (quartiles {a['q1_us']} .. {a['q3_us']}, range "
              f"{a['min_us']} .. {a['max_us']}; {row['torch_mirror_host_syncs']} synchronising operators), native "
              f"{b['median_us']} us (quartiles {b['q1_us']} .. {b['q3_us']}, range {b['min_us']} .. {b['max_us']}; "
              f"{row['native_host_syncs']} synchronising operators), x{row['speedup_median']}; edge mask covers "
              f"{100 * row['edge_mask_cover']:.1f} %, {row['mask_pixels_differing']} mask pixels differ")
        if "native_unremapped" in row:
            c = row["native_unremapped"]
            row["remap_cost_us"] = round(b["median_us"] - c["median_us"], 1)
            print(f"    the un-remapped native call of this build on the same input: {c['median_us']} us (quartiles "
                  f"{c['q1_us']} .. {c['q3_us']}, range {c['min_us']} .. {c['max_us']}): the remap costs "
                  f"{row['remap_cost_us']} us; image bit-equal to the mirror's: {row['image_bits_equal_mirror']}")
        out.append(row)
    print(json.dumps({"frame_prepare_profile": out}))


def traced(which, index):
    import torch
    mirror, native, _ = paths(CONFIGS[index], torch.device("cuda:0"))
    fn = native if which == "native" else mirror
    for _ in range(CALLS_TRACED):
        fn()
    torch.cuda.synchronize()


def summarise(root):
    rows = []
    for index, cfg in enumerate(CONFIGS):
        for which in ("native", "mirror"):
            files = glob.glob(os.path.join(root, f"trace_{which}_{index}", "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                print(f"{cfg['name']} {which}: no kernel trace under {root}")
                continue
            with open(files[0], newline="") as f:
                ks = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
            launches = sum(k[1] for k in ks) / CALLS_TRACED
            total = sum(k[2] for k in ks) / CALLS_TRACED / 1e3
            print(f"{cfg['name']} {which}: {launches:g} kernel launches per call, {total:.1f} us of kernel time per call")
            for name, calls, ns in sorted(ks, key=lambda k: -k[2]):
                rows.append((cfg["name"], which, name, calls, round(ns / calls, 1)))
                if which == "native":
                    print(f"    {name[:100]}: {calls / CALLS_TRACED:g} per call, {ns / calls / 1e3:.1f} us each")
    with open(os.path.join(root, "frame_prepare_kernel_stats.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Config", "Path", "Name", "Calls", "AverageNs"])
        w.writerows(rows)


def main():
    args = sys.argv[1:]
    if "--summarise" in args:
        return summarise(args[args.index("--summarise") + 1])
    index = int(args[args.index("--config") + 1]) if "--config" in args else 0
    if "--native-only" in args:
        return traced("native", index)
    if "--mirror-only" in args:
        return traced("mirror", index)
    measure()


if __name__ == "__main__":
    main()
