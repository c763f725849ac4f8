"""The sparse TSDF volume on the GPU box:

    python profiles/sparse_tsdf_profile.py [output file]          # default: profiles/sparse_tsdf_profile.txt

The 256^3 / 640 x 480 / 300 000-Gaussian case of profiles/tsdf_profile.py, dense (tsdf.TSDFVolume, the code of the commit
before: tsdf.hip is untouched) against sparse (sparse_tsdf.SparseTSDFVolume, same origin and voxel size): per view the
wall time of integrate() and the kernels' own times from the library's events, split into the allocation launches and
the update; extract_mesh() per launch; bytes held.  A view is measured twice: FIRST (a reset volume: every brick is
new) and AGAIN (every candidate is found in the map).  Then the same scene at a quarter of the voxel size, which
check_dims refuses for the dense volume.  The update's grid is the pool (workgroups past the brick count leave at once):
it is timed with a pool just above the need and with one of 65 536 bricks, which is what the idle workgroups cost.
Wall times are medians of repeated calls, each ended by a synchronise; kernel times are means over five warm calls.  No
threshold is set anywhere: the numbers are written down.  One human-readable line per measurement, then one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import mesh_clean_profile as CP  # noqa: E402
import tsdf_profile as TP  # noqa: E402
from monogs_amd import tsdf as T  # noqa: E402
from monogs_amd.sparse_tsdf import SparseTSDFVolume, samples_of  # noqa: E402

ALLOC = ("sparse_alloc_candidates", "sparse_alloc_insert", "sparse_alloc_flag", "sparse_alloc_scan", "sparse_alloc_commit")


def sparse_case(name, origin, vs, cap, view, pkg, lines, out, dev):
    cam = (view.fx, view.fy, view.cx, view.cy)
    kw = dict(image=pkg["render"], opacity=pkg["opacity"], normalize=True, min_opacity=0.95)
    vol = SparseTSDFVolume(origin, vs, cap, device=dev)
    integ = lambda: vol.integrate(pkg["depth"], view.T, *cam, **kw)

    def first():
        vol.reset()
        integ()

    first()
    st = vol.stats()
    # FIRST: the reset is outside the events (fill kernels of torch), inside the wall time of `first_wall` only
    k_first = CP.kernels_us(first)
    k_again = CP.kernels_us(integ)
    wall_again = CP.median_us(integ, 3, 21)
    reset_us = CP.median_us(vol.reset, 2, 11)
    wall_first = CP.median_us(first, 2, 11) - reset_us
    vol.reset()
    integ()                                             # one view, as the dense volume holds it
    ext = lambda: vol.extract_mesh(1.0)
    verts, faces, _ = ext()
    wall_ext = CP.median_us(ext, 3, 21)
    k_ext = CP.kernels_us(ext)
    split = lambda k: (round(sum(k.get(n, 0.0) for n in ALLOC), 1), k.get("sparse_integrate", 0.0))
    rec = {"voxel_size": vs, "max_bricks": cap, "stats": st, "samples_per_pixel": samples_of(vol.trunc, vs),
           "integrate_first_wall_us": round(wall_first, 1), "integrate_again_wall_us": round(wall_again, 1),
           "kernels_first_us": k_first, "kernels_again_us": k_again,
           "alloc_update_first_us": split(k_first), "alloc_update_again_us": split(k_again),
           "extract_wall_us": round(wall_ext, 1), "extract_kernels_us": k_ext, "verts": int(verts.shape[0]),
           "faces": int(faces.shape[0]), "alloc_scratch_bytes": int(vol._alloc_scratch.numel())}
    out[name] = rec
    lines.append(f"{name}: voxel {vs:.5f}, pool {cap} bricks: one 640x480 view allocates {st['bricks']} bricks "
                 f"({st['bricks'] * 512} points, {st['bytes_in_use']} B of planes in use, {st['bytes']} B held by the pool "
                 f"and the map, {rec['alloc_scratch_bytes']} B of allocation scratch; dropped {st['dropped']}, out of range "
                 f"{st['out_of_range']}); integrate() FIRST {wall_first:.0f} us per call (wall), kernels: allocation "
                 f"{split(k_first)[0]} us + update {split(k_first)[1]} us {k_first}; AGAIN {wall_again:.0f} us (wall), "
                 f"allocation {split(k_again)[0]} us + update {split(k_again)[1]} us {k_again}; extract_mesh "
                 f"{verts.shape[0]} vertices / {faces.shape[0]} faces, {wall_ext:.0f} us per call (wall, two host reads), "
                 f"kernels (us per launch) {k_ext}, {sum(k_ext.values()):.1f} us in all")
    return vol, verts, faces


def main():
    dev = torch.device("cuda:0")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else os.path.join(ROOT, "profiles", "sparse_tsdf_profile.txt")
    lines, out = [], {}
    W, H, N, n = 640, 480, 300000, 256
    gm, view, pkg = TP.setup(dev, W, H, N)
    cam = (view.fx, view.fy, view.cx, view.cy)
    kw = dict(image=pkg["render"], opacity=pkg["opacity"], normalize=True, min_opacity=0.95)
    # ---- dense: the code of the commit before (profiles/tsdf_profile.txt holds that commit's own run) ----
    dense = TP.volume_for(gm, n, dev)
    integ = lambda: dense.integrate(pkg["depth"], view.T, *cam, **kw)
    integ()
    torch.cuda.synchronize()
    updated = int((dense.weight > 0).sum())
    walls_i = [CP.median_us(integ, 3, 21) for _ in range(3)]
    k_i = CP.kernels_us(integ)
    dense.reset()
    integ()
    ext = lambda: dense.extract_mesh(1.0)
    dv, df, _ = ext()
    walls_e = [CP.median_us(ext, 3, 21) for _ in range(3)]
    k_e = CP.kernels_us(ext)
    held = 20 * n ** 3
    recorded = {}
    try:
        with open(os.path.join(ROOT, "profiles", "tsdf_profile.txt"), encoding="utf-8") as fh:
            rec = json.loads(fh.read().strip().splitlines()[-1])
        recorded = {"integrate_wall_us": rec["integrate"]["wall_us"], "integrate_kernel_us": rec["integrate"]["kernel_us"],
                    "extract_wall_us": rec["extract"]["wall_us"], "extract_kernels_us": rec["extract"]["kernels_us"]}
    except (OSError, ValueError, KeyError):
        pass
    out["dense_256"] = {"voxel_size": dense.voxel_size, "updated_points": updated, "integrate_wall_us_three_runs":
                        [round(w, 1) for w in walls_i], "integrate_kernels_us": k_i, "extract_wall_us_three_runs":
                        [round(w, 1) for w in walls_e], "extract_kernels_us": k_e, "verts": int(dv.shape[0]),
                        "faces": int(df.shape[0]), "bytes": held, "recorded_by_tsdf_profile_txt": recorded}
    lines.append(f"dense {n}^3 (voxel {dense.voxel_size:.5f}), {held} B of planes: integrate {min(walls_i):.0f} .. "
                 f"{max(walls_i):.0f} us per call (wall; three medians of 21), kernels {k_i}, {updated} of {n ** 3} points "
                 f"updated; extract_mesh {dv.shape[0]} vertices / {df.shape[0]} faces, {min(walls_e):.0f} .. "
                 f"{max(walls_e):.0f} us per call (wall), kernels (us per launch) {k_e}, {sum(k_e.values()):.1f} us in all; "
                 f"profiles/tsdf_profile.txt, the dense file's own run, recorded {recorded}")
    origin, vs = dense.origin, dense.voxel_size
    # ---- sparse, the same lattice ----
    vol, sv, sf = sparse_case("sparse_256", origin, vs, 65536, view, pkg, lines, out, dev)
    need = vol.stats()["bricks"]
    same = bool(sv.shape[0] == dv.shape[0] and sf.shape[0] == df.shape[0])
    out["sparse_256"]["mesh_counts_equal_dense"] = same
    lines.append(f"sparse_256 against dense_256: the same numbers of vertices and faces: {same}")
    del vol, dense
    tight = 1 << max(8, (2 * need - 1).bit_length())
    sparse_case("sparse_256_tight_pool", origin, vs, tight, view, pkg, lines, out, dev)
    a, b = out["sparse_256"]["kernels_again_us"]["sparse_integrate"], out["sparse_256_tight_pool"]["kernels_again_us"]["sparse_integrate"]
    lines.append(f"the update's grid is the pool: sparse_integrate {a} us over 65536 workgroups against {b} us over {tight} "
                 f"({need} of them with a brick): {a - b:.1f} us for {65536 - tight} workgroups that leave at once")
    # ---- a quarter of the voxel size: 1021^3 points, which the dense volume refuses ----
    fine = 4 * (n - 1) + 1
    try:
        T.check_dims((fine, fine, fine))
        refused = False
    except ValueError:
        refused = True
    lines.append(f"a quarter of the voxel size: the dense volume would hold {fine}^3 points = {20 * fine ** 3} B; check_dims "
                 f"refuses it: {refused}")
    out["dense_quarter_refused"] = refused
    sparse_case("sparse_quarter_voxel", origin, vs / 4.0, 262144, view, pkg, lines, out, dev)
    for ln in lines:
        print(ln, flush=True)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
