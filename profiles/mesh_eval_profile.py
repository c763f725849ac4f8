"""Mesh evaluation on the GPU box:

    python profiles/mesh_eval_profile.py [output file]          # default: profiles/mesh_eval_profile.txt

evaluate_mesh at n_samples = 200 000 per side on the two meshes of profiles/mesh_clean_profile.py - (a) the extraction
of the 256^3 / 300 000-Gaussian view, (b) the lattice of 8 x 8 x 8 spheres with about a million faces - each against a
copy of itself moved by a thousandth of its box diagonal.  Per mesh: the wall time per call (warm; median of repeated
calls, each ending in its one host read), the kernels' own times per launch from the library's events (mean of five warm
calls; a call samples twice and queries twice, so these names appear twice per call), nearest_distance alone at the
chosen cell size and at cell sizes giving 1/2, 8 and 32 cells per point in the box, the device brute force
nearest_distance_torch on the same points, and the host route on the same inputs: the NumPy sampler mirror plus
scipy.spatial.cKDTree (build and query, both directions).  No threshold is set anywhere: the numbers are written down.
One human-readable line per measurement, then one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import mesh_clean_profile as CP  # noqa: E402
import tsdf_profile as TP  # noqa: E402
from monogs_amd import mesh_eval as ME  # noqa: E402

N_SAMPLES = 200_000


def measure(name, verts, faces, lines, out):
    lo, hi = verts.min(dim=0).values, verts.max(dim=0).values
    diag = float((hi - lo).norm())
    shift = torch.tensor([0.62, -0.34, 0.46], device=verts.device) * (1e-3 * diag)
    gt = ((verts + shift).contiguous(), faces)
    thr = 2e-3 * diag
    run = lambda: ME.evaluate_mesh((verts, faces), gt, n_samples=N_SAMPLES, threshold=thr)
    scores = run()
    wall = CP.median_us(run, 2, 11)
    k = CP.kernels_us(run)
    pp, _ = ME.sample_surface(verts, faces, N_SAMPLES, 0)
    gp, _ = ME.sample_surface(*gt, N_SAMPLES, 1)
    sample_wall = CP.median_us(lambda: ME.sample_surface(verts, faces, N_SAMPLES, 0), 2, 11)
    ext = (gp.max(dim=0).values - gp.min(dim=0).values).double()
    volume = float(ext.prod())
    nn = {}
    for label, per_point in (("chosen", None), ("0.5/pt", 0.5), ("8/pt", 8.0), ("32/pt", 32.0)):
        cell = None if per_point is None else (volume / (per_point * N_SAMPLES)) ** (1.0 / 3.0)
        fn = lambda: ME.nearest_distance(pp, gp, cell_size=cell)
        nn[label] = {"cell_size": cell, "wall_us": round(CP.median_us(fn, 2, 11), 1),
                     "query_us": CP.kernels_us(fn).get("nn_query")}
    d2, idx = ME.nearest_distance(pp, gp)
    t0 = time.perf_counter()
    bd2, bidx = ME.nearest_distance_torch(pp, gp, chunk_elems=1 << 26)
    torch.cuda.synchronize()
    brute_ms = (time.perf_counter() - t0) * 1e3
    agrees = bool(torch.equal(d2.view(torch.int32), bd2.view(torch.int32)) and torch.equal(idx, bidx))
    # the host route
    from scipy.spatial import cKDTree
    hv, hf, gv = verts.cpu().numpy(), faces.cpu().numpy(), gt[0].cpu().numpy()
    t0 = time.perf_counter()
    hp, _ = ME.sample_surface_numpy(hv, hf, N_SAMPLES, 0)
    hg, _ = ME.sample_surface_numpy(gv, hf, N_SAMPLES, 1)
    t_sample = time.perf_counter() - t0
    t0 = time.perf_counter()
    d_pg = cKDTree(hg).query(hp)[0]
    d_gp = cKDTree(hp).query(hg)[0]
    t_tree = time.perf_counter() - t0
    same_points = bool(np.array_equal(hp.view(np.int32), pp.cpu().numpy().view(np.int32)))
    host = dict(accuracy=float(d_pg.mean()), completion=float(d_gp.mean()), precision=float((d_pg < np.float32(thr)).mean()),
                recall=float((d_gp < np.float32(thr)).mean()))
    rec = {"verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "threshold": thr, "scores": scores,
           "evaluate_mesh_wall_us": round(wall, 1), "kernels_us_per_launch": k, "sample_surface_wall_us": round(sample_wall, 1),
           "nearest_distance": nn, "device_brute_force_ms": round(brute_ms, 1), "grid_equals_brute_force": agrees,
           "host_sampler_ms": round(t_sample * 1e3, 1), "host_ckdtree_ms": round(t_tree * 1e3, 1), "host_scores": host,
           "host_points_equal_device_points": same_points}
    lines.append(
        f"{name}: {rec['verts']} vertices, {rec['faces']} faces, {N_SAMPLES} samples per side; evaluate_mesh {wall:.0f} us per "
        f"call (wall, with its one host read); kernels, us per launch: {k}; sample_surface alone {sample_wall:.0f} us per "
        f"call; nearest_distance (wall us / nn_query us) " +
        ", ".join(f"{lab}: {v['wall_us']:.0f} / {v['query_us']}" for lab, v in nn.items()) +
        f"; device brute force nearest_distance_torch {brute_ms:.0f} ms (grid equals it bit for bit: {agrees}); host: NumPy "
        f"sampler {t_sample * 1e3:.0f} ms (same points as the device: {same_points}), cKDTree build + query both ways "
        f"{t_tree * 1e3:.0f} ms; scores device {scores} host {host}")
    out[name] = rec


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "mesh_eval_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    vol = TP.volume_for(gm, n, dev)
    vol.integrate(pkg["depth"], view.T, view.fx, view.fy, view.cx, view.cy, image=pkg["render"], opacity=pkg["opacity"],
                  normalize=True, min_opacity=0.95)
    v, f, _ = vol.extract_mesh(1.0)
    measure("view_256", v, f, lines, out)
    del vol, gm, pkg
    v, f, _ = CP.sphere_lattice(dev).extract_mesh(1.0)
    measure("sphere_lattice_256", v, f, lines, out)
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
