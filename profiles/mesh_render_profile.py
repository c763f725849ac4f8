"""Mesh rendering and culling on the GPU box:

    python profiles/mesh_render_profile.py [output file]          # default: profiles/mesh_render_profile.txt

render_mesh_depth at 640 x 480 and 1200 x 680 on (a) the extraction of the 256^3 / 300 000-Gaussian view of
profiles/mesh_clean_profile.py, from the pose it was fused from, (b) that file's lattice of 8 x 8 x 8 spheres with about a
million faces, from outside, where many small faces land on the same pixels, and (c) a 12-face room seen from inside -
without near-plane clipping only its far wall is drawn, two faces that each cover the whole image; (c) also with the
large-face threshold above H W, i.e. one lane per face, and (a) with thresholds of 256, 64 and 16 pixels.  Per case: the wall time per call (warm, median of 11 calls), the
kernels' own times per launch from the library's events (mean of five warm calls), the record, and the NumPy mirror on the
host (on the first 16 384 faces only for (b): the mirror is a Python loop over faces) with the check that the device
equals it bit for bit.  Then cull_by_visibility over 20 views of (a), and evaluate_mesh with and without `cull` on (a)
and (b) as profiles/mesh_eval_profile.py runs it.  No threshold is set anywhere: the numbers are written down.  One
human-readable line per measurement, then one JSON line."""
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
from monogs_amd import mesh_eval as ME, mesh_render as MR  # noqa: E402
from monogs_amd.pose import SE3_exp  # noqa: E402

SIZES = ((480, 640), (680, 1200))
N_SAMPLES = 200_000
MIRROR_FACES = 16384


def scaled(view, H, W):
    """The view's pose and intrinsics at another image size."""
    T, fx, fy, cx, cy, H0, W0 = view
    sx, sy = W / W0, H / H0
    return T, fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5, H, W


def measure_render(name, verts, faces, view, lines, out, mirror_faces=None, **kw):
    T, fx, fy, cx, cy, H, W = view
    run = lambda: MR.render_mesh_depth(verts, faces, T, fx, fy, cx, cy, H, W, **kw)
    depth, face, record = run()
    wall = CP.median_us(run, 2, 11)
    k = CP.kernels_us(run)
    hv, hf = verts.cpu().numpy(), faces.cpu().numpy()
    hT = T.cpu().numpy() if torch.is_tensor(T) else T
    sub = hf if mirror_faces is None else hf[:mirror_faces]
    t0 = time.perf_counter()
    md, mf, mrec = MR.render_mesh_depth_numpy(hv, sub, hT, fx, fy, cx, cy, H, W, **{a: b for a, b in kw.items() if a != "large_grid"})
    t_np = time.perf_counter() - t0
    if mirror_faces is None:
        agrees = bool(np.array_equal(md.view(np.int32), depth.cpu().numpy().view(np.int32))
                      and np.array_equal(mf, face.cpu().numpy()) and mrec.tolist() == record.cpu().tolist())
    else:
        agrees = None
    covered = int((face >= 0).sum())
    rec = {"verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "H": H, "W": W, "options": kw,
           "record": record.cpu().tolist(), "covered_pixels": covered, "wall_us": round(wall, 1), "kernels_us_per_launch": k,
           "kernels_sum_us": round(sum(k.values()), 1), "mirror_ms": round(t_np * 1e3, 1), "mirror_faces": int(sub.shape[0]),
           "device_equals_mirror": agrees}
    top = max(k, key=k.get)
    lines.append(f"{name} {W}x{H} {kw or ''}: {rec['faces']} faces, record {rec['record']}, {covered} pixels covered; "
                 f"render_mesh_depth {wall:.0f} us per call (wall); kernels, us per launch: {k} (sum {rec['kernels_sum_us']}, "
                 f"largest: {top}); NumPy mirror on {rec['mirror_faces']} faces {t_np * 1e3:.0f} ms; device equals mirror: {agrees}")
    out[f"{name}_{W}x{H}" + "".join(f"_{a}_{b}" for a, b in kw.items())] = rec


def orbit(view, n, dev):
    """n views around the view's pose: small rigid motions applied in the camera's frame."""
    T, fx, fy, cx, cy, H, W = view
    T = torch.as_tensor(T).to(dev).float()
    g = torch.Generator().manual_seed(0)
    taus = (torch.rand(n, 6, generator=g) - 0.5) * torch.tensor([0.6, 0.6, 0.6, 0.3, 0.3, 0.3])
    return [((SE3_exp(tau).to(dev) @ T).contiguous(), fx, fy, cx, cy, H, W) for tau in taus]


def measure_protocol(name, verts, faces, view, lines, out):
    dev = verts.device
    views = orbit(view, 20, dev)
    run = lambda: MR.cull_by_visibility((verts, faces), views)
    info = run()[3]
    wall = CP.median_us(run, 1, 5)
    k = CP.kernels_us(run, calls=2)
    lo, hi = verts.min(dim=0).values, verts.max(dim=0).values
    diag = float((hi - lo).norm())
    shift = torch.tensor([0.62, -0.34, 0.46], device=dev) * (1e-3 * diag)
    gt = ((verts + shift).contiguous(), faces)
    thr = 2e-3 * diag
    plain = lambda: ME.evaluate_mesh((verts, faces), gt, n_samples=N_SAMPLES, threshold=thr)
    cull = dict(views=views, occlusion="gt", eps=thr)
    culled = lambda: ME.evaluate_mesh((verts, faces), gt, n_samples=N_SAMPLES, threshold=thr, cull=cull)
    s_plain, s_cull = plain(), culled()
    w_plain, w_cull = CP.median_us(plain, 2, 11), CP.median_us(culled, 1, 5)
    l1 = MR.mesh_depth_l1((verts, faces), gt, views)
    w_l1 = CP.median_us(lambda: MR.mesh_depth_l1((verts, faces), gt, views), 1, 5)
    rec = {"cull_by_visibility_20_views_wall_us": round(wall, 1), "cull_info": info, "cull_kernels_us_per_launch": k,
           "evaluate_mesh_wall_us": round(w_plain, 1), "evaluate_mesh_cull_20_views_wall_us": round(w_cull, 1),
           "scores": s_plain, "scores_culled": s_cull, "mesh_depth_l1": l1, "mesh_depth_l1_20_views_wall_us": round(w_l1, 1)}
    lines.append(f"{name} protocol at {view[6]}x{view[5]}: cull_by_visibility over 20 views {wall:.0f} us per call (wall, one "
                 f"host read; 20 renders, 20 visibility launches, one cull), {info}; kernels, us per launch: {k}; "
                 f"evaluate_mesh {w_plain:.0f} us without cull, {w_cull:.0f} us with cull over the 20 views (two culls and "
                 f"20 renders of the ground truth more); mesh_depth_l1 over the 20 views {w_l1:.0f} us, value {l1}; "
                 f"scores {s_plain}; culled {s_cull}")
    out[f"{name}_protocol"] = rec


def room(dev):
    lo, hi = np.array([-2.0, -1.5, -3.0]), np.array([2.0, 1.5, 1.0])
    c = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])], np.float32)
    q = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    f = np.array([t for a, b, cc, d in q for t in ((a, b, cc), (a, cc, d))], np.int32)
    return torch.from_numpy(c).to(dev), torch.from_numpy(f).to(dev)


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "mesh_render_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    vol = TP.volume_for(gm, n, dev)
    vol.integrate(pkg["depth"], view.T, view.fx, view.fy, view.cx, view.cy, image=pkg["render"], opacity=pkg["opacity"],
                  normalize=True, min_opacity=0.95)
    v, f, _ = vol.extract_mesh(1.0)
    base = (view.T.detach().clone(), view.fx, view.fy, view.cx, view.cy, H, W)
    for h, w in SIZES:
        measure_render("view_256", v, f, scaled(base, h, w), lines, out)
    for thr in (256, 64, 16):                                              # where the split between the two paths sits
        measure_render("view_256", v, f, base, lines, out, large_threshold=thr)
    measure_protocol("view_256", v, f, base, lines, out)
    del vol, gm, pkg
    v, f, _ = CP.sphere_lattice(dev).extract_mesh(1.0)
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([-128.0, -128.0, 150.0])                       # the camera at (128, 128, -150) looks along +z
    outside = (T, 500.0, 500.0, 319.5, 239.5, H, W)
    for h, w in SIZES:
        measure_render("sphere_lattice_256", v, f, scaled(outside, h, w), lines, out, mirror_faces=MIRROR_FACES)
    measure_protocol("sphere_lattice_256", v, f, outside, lines, out)
    v, f = room(dev)
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([0.1, -0.05, 2.5])                             # the camera at (-0.1, 0.05, -2.5), inside
    inside = (T, 600.0, 600.0, 319.5, 239.5, H, W)
    for h, w in SIZES:
        measure_render("room_12", v, f, scaled(inside, h, w), lines, out)
        measure_render("room_12", v, f, scaled(inside, h, w), lines, out, large_threshold=h * w + 1)
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out, default=str))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
