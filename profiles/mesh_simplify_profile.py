"""Mesh simplification on the GPU box:

    python profiles/mesh_simplify_profile.py [output file] [--extract-only]    # default: profiles/mesh_simplify_profile.txt

simplify_mesh at cells of two voxels on the two meshes of profiles/mesh_clean_profile.py - (a) the extraction of the
256^3 / 300 000-Gaussian view, (b) the lattice of 8 x 8 x 8 spheres with about a million faces - and on (c) a worst case
for the atomics: a million vertices in ONE cell, with a million faces among them that all collapse.  Per mesh: the wall
time per call (warm; the median of repeated calls, each ended by a synchronise - the call synchronises itself anyway, by
its one host read of the counts), the kernels' own times per launch from the library's events (mean of five warm calls),
and the NumPy mirror on the host on the same input (arrays already on the host).  Then extract_mesh() of the lattice
volume without the keyword, for the comparison with the commit before (run this file there: the measurement needs
nothing of the simplification).  No threshold is set anywhere: the numbers are written down.  One human-readable line
per measurement, then one JSON line."""
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

try:
    from monogs_amd import mesh_simplify as MS  # noqa: E402
except ImportError:                                 # the commit before: only extract_mesh() is measured
    MS = None
if "--extract-only" in sys.argv:                    # for alternating runs against the commit before
    MS = None


def measure(name, verts, faces, colors, kw, lines, out):
    run = lambda: MS.simplify_mesh(verts, faces, colors, **kw)
    ov, of, oc, info = run()
    wall = CP.median_us(run, 3, 21)
    k = CP.kernels_us(run)
    hv, hf, hc = verts.cpu().numpy(), faces.cpu().numpy(), colors.cpu().numpy()
    t_np, ref = CP.host_us(lambda: MS.simplify_mesh_numpy(hv, hf, hc, **kw))
    agrees = bool(np.array_equal(ref[0].view(np.int32), ov.cpu().numpy().view(np.int32))
                  and np.array_equal(ref[1], of.cpu().numpy())
                  and np.array_equal(ref[2].view(np.int32), oc.cpu().numpy().view(np.int32)) and ref[3] == info)
    top = max(k, key=k.get)
    out[name] = {"info": info, "keywords": {a: (list(b) if isinstance(b, tuple) else b) for a, b in kw.items()},
                 "simplify_mesh_wall_us": round(wall, 1), "kernels_us_per_launch": k,
                 "kernels_sum_us": round(sum(k.values()), 1), "longest_launch": top,
                 "numpy_mirror_host_us": round(t_np, 1), "mirror_agrees": agrees}
    lines.append(f"{name}: {info['verts_in']} vertices, {info['faces_in']} faces -> {info['verts_out']} / "
                 f"{info['faces_out']} ({info['num_clusters']} clusters, {info['collapsed_faces']} collapsed and "
                 f"{info['duplicate_faces']} duplicate faces); simplify_mesh {wall:.0f} us per call (wall, with its host "
                 f"read and output allocations), kernels {sum(k.values()):.1f} us in all, the longest {top} "
                 f"(us per launch: {k}); simplify_mesh_numpy on the host {t_np / 1e3:.1f} ms (agrees bit for bit: {agrees})")


def one_cell(dev, n=1_000_000):
    g = torch.Generator(device="cpu").manual_seed(0)
    verts = torch.rand(n, 3, generator=g).to(dev)
    faces = torch.randint(0, n, (n, 3), generator=g, dtype=torch.int32).to(dev)
    return verts, faces, torch.rand(n, 3, generator=g).to(dev)


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "mesh_simplify_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    vol = TP.volume_for(gm, n, dev)
    vol.integrate(pkg["depth"], view.T, view.fx, view.fy, view.cx, view.cy, image=pkg["render"], opacity=pkg["opacity"],
                  normalize=True, min_opacity=0.95)
    if MS is not None:
        measure("view_256", *vol.extract_mesh(1.0), dict(cell=2.0 * vol.voxel_size, origin=tuple(vol.origin)), lines, out)
    del vol, gm, pkg
    vol = CP.sphere_lattice(dev)
    if MS is not None:
        measure("sphere_lattice_256", *vol.extract_mesh(1.0), dict(cell=2.0 * vol.voxel_size, origin=tuple(vol.origin)),
                lines, out)
        measure("one_cell_1m", *one_cell(dev), dict(cell=1.0, origin=(0.0, 0.0, 0.0)), lines, out)
    walls = [CP.median_us(lambda: vol.extract_mesh(1.0), 3, 21) for _ in range(3)]
    out["extract_mesh_default"] = {"wall_us_three_runs": [round(w, 1) for w in walls]}
    lines.append(f"sphere_lattice_256: extract_mesh() without the keyword {min(walls):.0f} .. {max(walls):.0f} us per call "
                 "(wall; three medians of 21 calls)")
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
