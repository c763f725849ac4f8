"""The edge set, the topology report and smoothing on the GPU box:

    python profiles/mesh_smooth_profile.py [output file]               # default: profiles/mesh_smooth_profile.txt

mesh_edges and smooth_mesh (10 Taubin iterations) on the two meshes of profiles/mesh_clean_profile.py - (a) the
extraction of the 256^3 / 300 000-Gaussian view, (b) the lattice of 8 x 8 x 8 spheres with about a million faces - and on
(c) a worst case for one degree counter, one cursor and one row: a fan of a million faces on ONE vertex.  Per mesh: the
wall time per call (warm; the median of 21 calls, each ended by a synchronise - the call synchronises itself anyway, by
its one host read of the record), the kernels' own times per launch from the library's events (mean of five warm calls),
one gather step against its byte count V (24 + 16 mean degree), and the NumPy mirrors on the host on the same input
(arrays already on the host).  extract_mesh() without the new keywords is measured by profiles/mesh_simplify_profile.py
--extract-only, here and on the commit before.  No threshold is set anywhere: the numbers are written down.  One
human-readable line per measurement, then one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import mesh_clean_profile as CP  # noqa: E402
import tsdf_profile as TP  # noqa: E402
from monogs_amd import mesh_smooth as SM, mesh_topology as MT  # noqa: E402


def measure(name, verts, faces, lines, out, smooth_kw=None, warm=3, timed=21, kernel_calls=5, mirror_repeats=3):
    V = int(verts.shape[0])
    smooth_kw = smooth_kw or {}                                        # default: 10 iterations, lam 0.5, mu -0.53, pinned
    edges_run = lambda: MT.mesh_edges(faces, V)
    smooth_run = lambda: SM.smooth_mesh(verts, faces, **smooth_kw)
    e = edges_run()
    s = smooth_run()
    info = e[4]
    e_wall, s_wall = CP.median_us(edges_run, 3, 21), CP.median_us(smooth_run, warm, timed)
    t_wall = CP.median_us(lambda: MT.mesh_topology(faces, V), 3, 21)
    e_k, s_k = CP.kernels_us(edges_run), CP.kernels_us(smooth_run, kernel_calls)
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    t_e, ref_e = CP.host_us(lambda: MT.mesh_edges_numpy(hf, V), mirror_repeats)
    t_s, ref_s = CP.host_us(lambda: SM.smooth_mesh_numpy(hv, hf, **smooth_kw), mirror_repeats)
    agrees = bool(all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(ref_e[:4], e[:4])) and ref_e[4] == info
                  and np.array_equal(ref_s[0].view(np.int32), s[0].cpu().numpy().view(np.int32)) and ref_s[1] == s[1])
    moved = info["referenced_verts"] - s[1]["pinned_verts"]
    mean_degree = 2.0 * info["edges"] / max(1, info["referenced_verts"])
    step_bytes = V * (24 + mean_degree * 16)
    step_us = s_k.get("ms_step", 0.0)
    out[name] = {"info": info, "mesh_edges_wall_us": round(e_wall, 1), "mesh_topology_wall_us": round(t_wall, 1),
                 "smooth_mesh_wall_us": round(s_wall, 1), "mesh_edges_kernels_us_per_launch": e_k,
                 "smooth_mesh_kernels_us_per_launch": s_k, "mesh_edges_kernels_sum_us": round(sum(e_k.values()), 1),
                 "smooth_keywords": smooth_kw, "smooth_timed_calls": timed, "steps": s[1]["steps"], "moved_verts": moved, "mean_degree": round(mean_degree, 2),
                 "step_bytes": int(step_bytes), "step_gb_per_s": round(step_bytes / max(step_us, 1e-9) / 1e3, 1),
                 "mesh_edges_numpy_host_us": round(t_e, 1), "smooth_mesh_numpy_host_us": round(t_s, 1),
                 "mirrors_agree": agrees}
    lines.append(f"{name}: {V} vertices, {info['faces_in']} faces, {info['edges']} edges ({info['boundary_edges']} boundary, "
                 f"{info['nonmanifold_edges']} non-manifold, euler {info['euler']}, closed {info['closed']}); mesh_edges "
                 f"{e_wall:.0f} us per call and mesh_topology {t_wall:.0f} us (wall, with the host read), kernels "
                 f"{sum(e_k.values()):.1f} us in all (us per launch: {e_k}); smooth_mesh({smooth_kw or 'defaults: 10 Taubin iterations'}) = "
                 f"{s[1]['steps']} steps, {moved} vertices move, {s_wall:.0f} us per call (us per launch: {s_k}); one gather step {step_us} us for "
                 f"{step_bytes / 1e6:.1f} MB at a mean degree of {mean_degree:.2f}: {step_bytes / max(step_us, 1e-9) / 1e3:.0f} "
                 f"GB/s; mesh_edges_numpy on the host {t_e / 1e3:.1f} ms, smooth_mesh_numpy {t_s / 1e3:.1f} ms (agree bit for "
                 f"bit: {agrees})")


def fan(dev, n=1_000_000):
    """n faces (0, i, i + 1) around vertex 0: one row of n + 1 neighbours."""
    rim = torch.arange(1, n + 2, dtype=torch.int32)
    faces = torch.stack([torch.zeros(n, dtype=torch.int32), rim[:-1], rim[1:]], 1).contiguous().to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    return torch.rand(n + 2, 3, generator=g).to(dev), faces


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "mesh_smooth_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    vol = TP.volume_for(gm, n, dev)
    vol.integrate(pkg["depth"], view.T, view.fx, view.fy, view.cx, view.cy, image=pkg["render"], opacity=pkg["opacity"],
                  normalize=True, min_opacity=0.95)
    measure("view_256", *vol.extract_mesh(1.0)[:2], lines, out)
    del vol, gm, pkg
    vol = CP.sphere_lattice(dev)
    measure("sphere_lattice_256", *vol.extract_mesh(1.0)[:2], lines, out)
    del vol
    # pinned, every vertex of the fan lies on a boundary edge and nothing moves: free
    measure("fan_1m", *fan(dev), lines, out, smooth_kw=dict(boundary="free"), mirror_repeats=1)
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
