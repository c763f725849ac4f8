"""Mesh clean-up on the GPU box:

    python profiles/mesh_clean_profile.py [output file]          # default: profiles/mesh_clean_profile.txt

clean_mesh(keep_largest=1) on two meshes: (a) the extraction of the 256^3 / 300 000-Gaussian case of
profiles/tsdf_profile.py (one 640x480 view), (b) an analytic mesh of about a million faces - a lattice of 8 x 8 x 8
spheres in a 256^3 volume, one cluster each.  Per mesh: the wall time per call (warm; the median of repeated calls, each
ended by a synchronise - the call synchronises itself anyway, by its one host read of the counts), the kernels' own
times per launch from the library's events (mean of five warm calls), and on the host the NumPy mirror and, where SciPy
is present, scipy.sparse.csgraph.connected_components on the same input (labels only; arrays already on the host).  No
threshold is set anywhere: the numbers are written down.  One human-readable line per measurement, then one JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import tsdf_profile as TP  # noqa: E402
from monogs_amd import _cabi, mesh_clean as MC, tsdf as T  # noqa: E402


def median_us(fn, warm, timed):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(timed):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def kernels_us(fn, calls=5):
    _cabi.profile_enable(True)
    for _ in range(calls):
        fn()
    p = _cabi.profile_read()
    _cabi.profile_enable(False)
    return {n: round(v[0] / v[1] * 1e3, 1) for n, v in p.items()}


def host_us(fn, repeats=3):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), out


def sphere_lattice(dev, n=256, pitch=32, radius=4.3):
    """A TSDF volume of n^3 points holding (n / pitch)^3 spheres."""
    vol = T.TSDFVolume((0.0, 0.0, 0.0), 1.0, (n, n, n), device=dev)
    ax = torch.arange(n, dtype=torch.float32, device=dev)
    d = lambda a, off: (torch.remainder(a - off, float(pitch)) - 0.5 * pitch) ** 2
    r = torch.sqrt(d(ax, 0.37)[None, None, :] + d(ax, 0.61)[None, :, None] + d(ax, 0.13)[:, None, None])
    vol.tsdf.copy_(torch.clamp((r - radius) / 3.0, -1.0, 1.0))
    vol.weight.fill_(1.0)
    return vol


def measure(name, verts, faces, colors, lines, out):
    run = lambda: MC.clean_mesh(verts, faces, colors, keep_largest=1)
    ov, of, _, info = run()
    wall = median_us(run, 3, 21)
    k = kernels_us(run)
    labels_run = lambda: MC.connected_components(verts.shape[0], faces)
    lab_wall = median_us(labels_run, 3, 21)
    hv, hf, hc = verts.cpu().numpy(), faces.cpu().numpy(), colors.cpu().numpy()
    t_np, ref = host_us(lambda: MC.clean_mesh_numpy(hv, hf, hc, keep_largest=1))
    agrees = bool(np.array_equal(ref[0].view(np.int32), ov.cpu().numpy().view(np.int32))
                  and np.array_equal(ref[1], of.cpu().numpy()) and ref[3] == info)
    rec = {"info": info, "clean_mesh_wall_us": round(wall, 1), "kernels_us_per_launch": k,
           "kernels_sum_us": round(sum(k.values()), 1), "connected_components_wall_us": round(lab_wall, 1),
           "numpy_mirror_host_us": round(t_np, 1), "mirror_agrees": agrees}
    line = (f"{name}: {info['verts_in']} vertices, {info['faces_in']} faces, {info['num_clusters']} clusters -> "
            f"{info['verts_out']} / {info['faces_out']} in {info['kept_clusters']}; clean_mesh(keep_largest=1) {wall:.0f} us "
            f"per call (wall, with its host read and output allocations), kernels {sum(k.values()):.1f} us in all "
            f"(us per launch: {k}); connected_components alone {lab_wall:.0f} us per call; clean_mesh_numpy on the host "
            f"{t_np / 1e3:.1f} ms (agrees bit for bit: {agrees})")
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        def scipy_labels():
            f = hf.astype(np.int64)
            rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
            g = coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(len(hv), len(hv)))
            return connected_components(g, directed=False)

        t_sp, (ncomp, _) = host_us(scipy_labels)
        rec["scipy_connected_components_host_us"] = round(t_sp, 1)
        rec["scipy_components"] = int(ncomp)
        line += f"; scipy.sparse.csgraph.connected_components on the host {t_sp / 1e3:.1f} ms ({ncomp} components)"
    except ImportError:
        line += "; SciPy is not installed"
    out[name] = rec
    lines.append(line)


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "mesh_clean_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    vol = TP.volume_for(gm, n, dev)
    vol.integrate(pkg["depth"], view.T, view.fx, view.fy, view.cx, view.cy, image=pkg["render"], opacity=pkg["opacity"],
                  normalize=True, min_opacity=0.95)
    measure("view_256", *vol.extract_mesh(1.0), lines, out)
    del vol, gm, pkg
    measure("sphere_lattice_256", *sphere_lattice(dev).extract_mesh(1.0), lines, out)
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
