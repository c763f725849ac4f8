"""Mesh normals on the GPU box:

    python profiles/mesh_normals_profile.py [output file]          # default: profiles/mesh_normals_profile.txt
    python profiles/mesh_normals_profile.py --old-paths [--root CHECKOUT]

face_normals, vertex_normals, evaluate_mesh(normals=True) and render_mesh_frame (640 x 480, four modes) on (a) the
extraction of the 256^3 / 300 000-Gaussian view of profiles/mesh_clean_profile.py, (b) that file's lattice of 8 x 8 x 8
spheres with about a million faces; face_normals and vertex_normals also on (c) tests/mesh_clean_cases.star, the fan
whose apex is in every face, at 3000 faces and at a million: every face adds into one accumulator.  Per case: the wall
time per call (warm, median of 11 calls, each ended by a synchronise), the kernels' own times per launch from the
library's events (mean of five warm calls), the NumPy mirror on the host and the check that the device equals it bit for
bit.  No threshold is set anywhere: the numbers are written down.  One human-readable line per measurement, then one
JSON line.

--old-paths times only what existed before the mesh normals - evaluate_mesh without `normals` and render_mesh_depth, on
(a) and (b) - and prints one JSON line; --root imports the package (and profiles/) from another checkout, e.g. the
parent commit built in place.  Run alternately on both commits in one session, that is the comparison the text file
reports against the run-to-run spread; that table and the reading below it were added to the text file by hand, under
the script's own lines."""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import mesh_clean_profile as CP  # noqa: E402
import tsdf_profile as TP  # noqa: E402
from monogs_amd import mesh_eval as ME, mesh_render as MR  # noqa: E402

N_SAMPLES = 200_000
W, H = 640, 480


def meshes(dev):
    """name -> (verts, faces, view) of the two profile meshes."""
    gm, view, pkg = TP.setup(dev, W, H, 300000)
    vol = TP.volume_for(gm, 256, dev)
    vol.integrate(pkg["depth"], view.T, view.fx, view.fy, view.cx, view.cy, image=pkg["render"], opacity=pkg["opacity"],
                  normalize=True, min_opacity=0.95)
    v, f, _ = vol.extract_mesh(1.0)
    out = {"view_256": (v, f, (view.T.detach().clone(), view.fx, view.fy, view.cx, view.cy, H, W))}
    del vol, gm, pkg
    v, f, _ = CP.sphere_lattice(dev).extract_mesh(1.0)
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([-128.0, -128.0, 150.0])                       # the camera at (128, 128, -150) looks along +z
    out["sphere_lattice_256"] = (v, f, (T, 500.0, 500.0, 319.5, 239.5, H, W))
    return out


def shifted_truth(verts, faces):
    """mesh_render_profile's ground truth: the mesh moved by a thousandth of its diagonal; and the threshold."""
    lo, hi = verts.min(dim=0).values, verts.max(dim=0).values
    diag = float((hi - lo).norm())
    shift = torch.tensor([0.62, -0.34, 0.46], device=verts.device) * (1e-3 * diag)
    return ((verts + shift).contiguous(), faces), 2e-3 * diag


def old_paths(cases):
    out = {}
    for name, (v, f, view) in cases.items():
        gt, thr = shifted_truth(v, f)
        T, fx, fy, cx, cy, h, w = view
        plain = lambda: ME.evaluate_mesh((v, f), gt, n_samples=N_SAMPLES, threshold=thr)
        render = lambda: MR.render_mesh_depth(v, f, T, fx, fy, cx, cy, h, w)
        out[name] = {"evaluate_mesh_wall_us": round(CP.median_us(plain, 2, 11), 1),
                     "render_mesh_depth_wall_us": round(CP.median_us(render, 2, 11), 1),
                     "render_kernels_us_per_launch": CP.kernels_us(render)}
    return out


def measure_normals(name, v, f, lines, out):
    from monogs_amd import mesh_normals as MN
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    rec = {"verts": int(v.shape[0]), "faces": int(f.shape[0])}
    for what, fn, mirror in (("face_normals", MN.face_normals, MN.face_normals_numpy),
                             ("vertex_normals", MN.vertex_normals, MN.vertex_normals_numpy)):
        run = lambda: fn(v, f)
        got, grec = run()
        wall, k = CP.median_us(run, 2, 11), CP.kernels_us(run)
        t0 = time.perf_counter()
        want, wrec = mirror(hv, hf)
        t_np = time.perf_counter() - t0
        same = bool(np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)) and grec.cpu().tolist() == wrec.tolist())
        rec[what] = {"wall_us": round(wall, 1), "kernels_us_per_launch": k, "record": wrec.tolist(),
                     "mirror_ms": round(t_np * 1e3, 1), "device_equals_mirror": same}
        lines.append(f"{name} {what}: {rec['verts']} vertices, {rec['faces']} faces, record {wrec.tolist()}; {wall:.0f} us per "
                     f"call (wall); kernels, us per launch: {k}; NumPy mirror {t_np * 1e3:.1f} ms; device equals mirror: {same}")
    out[name] = rec


def measure_users(name, v, f, view, lines, out):
    gt, thr = shifted_truth(v, f)
    kw = dict(n_samples=N_SAMPLES, threshold=thr)
    plain = lambda: ME.evaluate_mesh((v, f), gt, **kw)
    normal = lambda: ME.evaluate_mesh((v, f), gt, normals=True, **kw)
    scores = normal()
    w_plain, w_normal = CP.median_us(plain, 2, 11), CP.median_us(normal, 2, 11)
    k = {n: t for n, t in CP.kernels_us(normal).items() if n in ("face_normals", "normal_stats", "normal_finish")}
    rec = out[name]
    rec["evaluate_mesh"] = {"wall_us": round(w_plain, 1), "normals_wall_us": round(w_normal, 1),
                            "normals_adds_us": round(w_normal - w_plain, 1), "new_kernels_us_per_launch": k,
                            "scores": {n: scores[n] for n in ME.NORMAL_KEYS}}
    lines.append(f"{name} evaluate_mesh at {N_SAMPLES} samples: {w_plain:.0f} us per call without normals, {w_normal:.0f} us "
                 f"with normals=True (+{w_normal - w_plain:.0f} us: two face_normals, two normal_stats, one normal_finish, eight "
                 f"more doubles in the one host read); its new kernels, us per launch: {k}; "
                 f"{ {n: scores[n] for n in ME.NORMAL_KEYS} }")
    T, fx, fy, cx, cy, h, w = view
    depth = lambda: MR.render_mesh_depth(v, f, T, fx, fy, cx, cy, h, w)
    w_depth = CP.median_us(depth, 2, 11)
    colors = torch.rand(v.shape[0], 3, device=v.device)
    frames = {}
    for mode in MR.FRAME_MODES:
        run = lambda: MR.render_mesh_frame(v, f, view, mode, colors=colors if mode == "color" else None)
        frame = run()
        wall = CP.median_us(run, 2, 11)
        shade = CP.kernels_us(run).get("mesh_shade")
        frames[mode] = {"wall_us": round(wall, 1), "mesh_shade_us": shade, "covered_pixels": int((frame != 0).any(dim=2).sum())}
    rec["render_mesh_frame"] = {"render_mesh_depth_wall_us": round(w_depth, 1), "modes": frames}
    lines.append(f"{name} render_mesh_frame {w}x{h}: render_mesh_depth alone {w_depth:.0f} us per call (wall); per mode, "
                 f"wall us per call and the mesh_shade launch in us: {frames}")


def main():
    dev = torch.device("cuda:0")
    cases = meshes(dev)
    if "--old-paths" in sys.argv:
        print(json.dumps({"root": ROOT, "old_paths": old_paths(cases)}), flush=True)
        return
    import mesh_clean_cases as MCC
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "mesh_normals_profile.txt")
    lines, out = [], {}
    for name, (v, f, view) in cases.items():
        measure_normals(name, v, f, lines, out)
        measure_users(name, v, f, view, lines, out)
    for n in (3000, 1_000_000):
        sv, _, sf = MCC.star(n)
        measure_normals(f"star_{n}", torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev), lines, out)
    out["old_paths"] = old_paths(cases)
    lines.append(f"old paths in this process: {out['old_paths']}")
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out, default=str))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
