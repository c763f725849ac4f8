"""The `--eval` tail of a run (slam.py:128-194) enqueued natively: every scored view is ONE C-ABI call
(mgs_eval_view: camera matrices, rasteriser forward, mgs_eval_score) that writes one record of a device table, and the
whole table comes to the host in one copy at the end.

Mirror of utils/eval_utils.py:114-194 (eval_rendering, save_gaussians); PSNR is image_utils.py:19-21 over the elements
with gt > 0 (eval_utils.py:150-152), SSIM loss_utils.py:61-101.  Added here: the L1 of the image and, when the dataset
yields a depth, the L1 of the rendered depth over the pixels with a measurement.  LPIPS stays None (its AlexNet weights
are a download).  There is no CPU path: off the GPU the evaluator raises."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import _cabi
from .ply_io import read_gaussian_ply, write_gaussian_ply  # noqa: F401  (the free functions of the map export)


def scores_from_records(table: np.ndarray, num_pixels: int) -> Dict[str, np.ndarray]:
    """Per-view scores in fp64 from the records [V, EVAL_RECORD_DOUBLES] of mgs_eval_score.  psnr is
    10 log10(n_mask / sse): inf for sse == 0 and nan for an empty mask, as torch gives them; psnr_all is the same over
    all 3 H W elements; depth_l1 is nan for a view scored without depth (or without a single measurement)."""
    t = np.asarray(table, np.float64).reshape(-1, _cabi.EVAL_RECORD_DOUBLES)
    m = 3.0 * float(num_pixels)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {
            "psnr": 10.0 * np.log10(t[:, _cabi.EVAL_N_MASK] / t[:, _cabi.EVAL_SSE]),
            "psnr_all": 10.0 * np.log10(m / t[:, _cabi.EVAL_SSE_ALL]),
            "ssim": t[:, _cabi.EVAL_SSIM] / m,
            "l1": t[:, _cabi.EVAL_ABS] / m,
            "depth_l1": t[:, _cabi.EVAL_DEPTH_ABS] / t[:, _cabi.EVAL_N_DEPTH],
            "pairs": t[:, _cabi.EVAL_PAIRS].astype(np.int64),
        }


def _nanmean(a: np.ndarray) -> float:
    a = a[~np.isnan(a)]
    return float(a.mean()) if a.size else float("nan")


class NativeEvaluator:
    """Scores views of one map.  begin() activates the map once (mgs_map_activate), score() enqueues one
    mgs_eval_view and reads nothing back, finish() copies the record table once, scores again - at a grown capacity -
    every view whose pair count exceeded the fixed pair capacity (as NativeTracker.run does), and returns the per-view
    arrays and their means.  The model is a GaussianModel (or anything with its raw parameter attributes).

    Memory: so that an overflowed row can be scored again, every scored view's ground truth (and depth, T, projection)
    stays referenced on the device until finish().  A uint8 ground truth makes that a quarter of the float image, but
    a batch still holds one image per view: score a long sequence in several begin() ... finish() batches, as
    eval_rendering_native does (its `chunk`), which costs one synchronisation per batch."""

    def __init__(self, gaussians, background, H: int, W: int, device, capacity: Optional[int] = None,
                 max_views: int = 4096, capacity_margin: float = 1.5):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("NativeEvaluator runs on the GPU only (HIP kernels, gfx950)")
        self.gaussians, self.H, self.W = gaussians, int(H), int(W)
        self.max_views, self.capacity_margin = int(max_views), capacity_margin
        self.bg = background.detach().to(self.dev, torch.float32).reshape(-1).contiguous()
        count = int(_cabi.lib().mgs_eval_score_partial_count(self.H, self.W))
        if count < 0 or self.max_views < 1:
            raise ValueError(f"NativeEvaluator: unsupported size {self.H} x {self.W} / {self.max_views} views")
        self.partial = torch.zeros(count, device=self.dev)      # the ticket behind it: zero once, kept by the kernel
        self.table = torch.zeros(self.max_views, _cabi.EVAL_RECORD_DOUBLES, dtype=torch.float64, device=self.dev)
        self.view_m, self.full_m = torch.empty(4, 4, device=self.dev), torch.empty(4, 4, device=self.dev)
        self.color = torch.empty(3, self.H, self.W, device=self.dev)
        self.depth = torch.empty(1, self.H, self.W, device=self.dev)
        self.opacity = torch.empty(1, self.H, self.W, device=self.dev)
        self.capacity = 0 if capacity is None else max(1024, int(capacity))
        self.overflow_regrows = 0
        self.first_pass = None          # the records as first scored (before any re-score), for the caller to inspect
        self._N, self.K, self._cap_alloc, self._geom_key = -1, -1, 0, None
        self._jobs = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    # ---- per-map state ---------------------------------------------------------------------------
    def begin(self):
        g = self.gaussians
        N = int(g._xyz.shape[0])
        if N < 1:
            raise RuntimeError("NativeEvaluator: the map is empty")
        K = int(g._features_dc.shape[1] + g._features_rest.shape[1])
        sd = int(g._scaling.shape[1])
        dev = self.dev
        if (N, K) != (self._N, self.K):
            self.scales, self.rots = torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev)
            self.opac = torch.empty(N, device=dev)
            self.shs = torch.empty(N, K, 3, device=dev) if K > 1 else None
            self.radii = torch.empty(N, dtype=torch.int32, device=dev)
            self.n_touched = torch.empty(N, dtype=torch.int32, device=dev)
        self._N, self.K, self.sd = N, K, sd
        if self.capacity == 0:          # no probe (it would need a host read): a guess that finish() corrects
            self.capacity = max(65536, (16 * N + 1023) // 1024 * 1024)
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        p = self._params = {k: f32(getattr(g, k)) for k in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc",
                                                            "_features_rest")}
        a = _cabi.MapActivateArgs()
        a.num_gaussians, a.scale_dims, a.sh_coeffs = N, sd, K
        a.log_scales, a.raw_rotations = p["_scaling"].data_ptr(), p["_rotation"].data_ptr()
        a.opacity_logits, a.features_dc = p["_opacity"].data_ptr(), p["_features_dc"].data_ptr()
        a.features_rest = p["_features_rest"].data_ptr() if K > 1 else None
        a.scales, a.rotations, a.opacities = self.scales.data_ptr(), self.rots.data_ptr(), self.opac.data_ptr()
        a.shs = self.shs.data_ptr() if K > 1 else None
        _cabi.check(_cabi.lib().mgs_map_activate(C.byref(a), self._stream()), "mgs_map_activate")
        self._jobs = []
        self.first_pass = None

    def _ensure_workspaces(self, deg):
        key = (self._N, self.K, deg)
        if key != self._geom_key:
            sizes = _cabi.workspace_sizes(_cabi.RasterShape(self._N, self.W, self.H, deg, self.K, 1024, 1.0, 1.0, 1.0))
            self.geom = torch.empty(int(sizes.geom_bytes), dtype=torch.uint8, device=self.dev)
            self._geom_key = key
        if self._cap_alloc != self.capacity:
            sizes = _cabi.workspace_sizes(_cabi.RasterShape(self._N, self.W, self.H, deg, self.K, self.capacity, 1.0, 1.0,
                                                            1.0))
            self.bins = torch.empty(int(sizes.bins_bytes), dtype=torch.uint8, device=self.dev)
            self._cap_alloc = self.capacity

    # ---- one view ----------------------------------------------------------------------------------
    def _view_args(self, row, job):
        """The argument block of mgs_eval_view for `job` (see _make_job) into record `row`."""
        view, gt, gt_depth, T, proj, ea, eb, eps, apply_exposure = job
        deg = int(self.gaussians.active_sh_degree)
        self._ensure_workspaces(deg)
        a = _cabi.EvalViewArgs()
        f, p = a.fwd, self._params
        f.shape = _cabi.RasterShape(self._N, self.W, self.H, deg, self.K, self.capacity,
                                    math.tan(0.5 * view.FoVx), math.tan(0.5 * view.FoVy), 1.0)
        f.means3D, f.scales, f.rotations = p["_xyz"].data_ptr(), self.scales.data_ptr(), self.rots.data_ptr()
        f.opacities = self.opac.data_ptr()
        f.shs = p["_features_dc"].data_ptr() if self.K == 1 else self.shs.data_ptr()
        f.viewmatrix, f.projmatrix, f.projmatrix_raw = self.view_m.data_ptr(), self.full_m.data_ptr(), proj.data_ptr()
        f.campos, f.bg = self.view_m.data_ptr(), self.bg.data_ptr()      # camera_center as render() passes it
        f.geom, f.bins = self.geom.data_ptr(), self.bins.data_ptr()
        f.out_color, f.out_depth, f.out_opacity = self.color.data_ptr(), self.depth.data_ptr(), self.opacity.data_ptr()
        f.radii, f.n_touched = self.radii.data_ptr(), self.n_touched.data_ptr()
        a.T = T.data_ptr()
        s = a.score
        s.height, s.width = self.H, self.W
        s.gt_format = _cabi.EVAL_GT_U8_HWC if gt.dtype == torch.uint8 else _cabi.EVAL_GT_F32_CHW
        s.row, s.num_rows = row, self.max_views
        s.gt = gt.data_ptr()
        s.gt_depth = None if gt_depth is None else gt_depth.data_ptr()
        s.apply_exposure = 1 if apply_exposure else 0
        if apply_exposure:
            s.exposure_a, s.exposure_b, s.exposure_eps = ea.data_ptr(), eb.data_ptr(), eps
        s.partial, s.table = self.partial.data_ptr(), self.table.data_ptr()
        return a

    def _enqueue(self, row, job):
        a = self._view_args(row, job)
        _cabi.check(_cabi.lib().mgs_eval_view(C.byref(a), self._stream()), "mgs_eval_view")

    def score(self, view, gt_image, gt_depth=None, apply_exposure: bool = False) -> int:
        """Enqueue the scoring of `view` (T, projection_matrix, FoVx, FoVy; exposure_a / exposure_b / exposure_eps when
        apply_exposure) against gt_image - float [3,H,W] in [0, 1] or uint8 [H,W,3] - and optionally gt_depth [H,W]
        (or [1,H,W]) in the units of the map; returns the row of the record.  Nothing is read from the device."""
        if self._jobs is None:
            raise RuntimeError("NativeEvaluator.score: call begin() first")
        row = len(self._jobs)
        if row >= self.max_views:
            raise RuntimeError(f"NativeEvaluator: more than max_views = {self.max_views} views")
        job = self._make_job(view, gt_image, gt_depth, apply_exposure)
        self._enqueue(row, job)
        self._jobs.append(job)
        return row

    def _make_job(self, view, gt_image, gt_depth, apply_exposure):
        """Checks the shapes and puts what a view's call reads on the device (a tensor already there is used in place)."""
        dev, H, W = self.dev, self.H, self.W
        gt = torch.as_tensor(gt_image)
        if gt.dtype == torch.uint8:
            if tuple(gt.shape) != (H, W, 3):
                raise ValueError(f"uint8 gt_image must be [{H},{W},3], got {tuple(gt.shape)}")
            gt = gt.to(dev).contiguous()
        else:
            if tuple(gt.shape) != (3, H, W):
                raise ValueError(f"gt_image must be [3,{H},{W}], got {tuple(gt.shape)}")
            gt = gt.detach().to(dev, torch.float32).contiguous()
        if gt_depth is not None:
            gt_depth = torch.as_tensor(gt_depth).detach().to(dev, torch.float32).contiguous()
            if gt_depth.numel() != H * W:
                raise ValueError(f"gt_depth must hold {H} x {W} values, got {tuple(gt_depth.shape)}")
        if int(view.image_height) != H or int(view.image_width) != W:
            raise ValueError(f"view is {view.image_height} x {view.image_width}, evaluator {H} x {W}")
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        ea = eb = None
        eps = 0.0
        if apply_exposure:
            ea, eb, eps = f32(view.exposure_a), f32(view.exposure_b), float(getattr(view, "exposure_eps", 1e-8))
        return (view, gt, gt_depth, f32(view.T), f32(view.projection_matrix), ea, eb, eps, apply_exposure)

    # ---- the end -----------------------------------------------------------------------------------
    def finish(self) -> Dict[str, object]:
        if self._jobs is None:
            raise RuntimeError("NativeEvaluator.finish: call begin() first")
        n = len(self._jobs)
        table = self.table[:n].cpu().numpy()                 # the one device-to-host copy (and wait)
        self.first_pass = table.copy()
        for _ in range(3):
            pairs = table[:, _cabi.EVAL_PAIRS]
            over = np.nonzero(pairs > self.capacity)[0]
            if over.size == 0:
                break
            self.capacity = (int(pairs.max() * self.capacity_margin) + 1023) // 1024 * 1024
            self.overflow_regrows += 1
            for row in over.tolist():
                self._enqueue(row, self._jobs[row])
            table = self.table[:n].cpu().numpy()
        else:
            if (table[:, _cabi.EVAL_PAIRS] > self.capacity).any():
                raise RuntimeError("pair capacity still exceeded after growing the workspaces three times")
        out: Dict[str, object] = dict(scores_from_records(table, self.H * self.W))
        out["records"] = table
        with_depth = np.array([j[2] is not None for j in self._jobs], bool)
        out["depth_l1"] = np.where(with_depth, out["depth_l1"], np.nan)
        for k in ("psnr", "psnr_all", "ssim", "l1"):
            out["mean_" + k] = float(np.mean(out[k])) if n else float("nan")
        out["mean_depth_l1"] = _nanmean(out["depth_l1"]) if with_depth.any() else None
        self._jobs = None
        return out


def eval_rendering_native(frames, gaussians, dataset, pipe, background, kf_indices, save_dir: Optional[str] = None,
                          iteration="final", interval: int = 5, evaluator=None, chunk: int = 64):
    """eval_metrics.eval_rendering (eval_utils.py:114-178) on the device: every `interval`-th non-keyframe view of
    range(0, len(frames) - 1) is rendered and scored against `dataset[idx][0]` through a NativeEvaluator.  Same result dict and JSON path (psnr/<iteration>/final_result.json,
    mean_lpips None); `mean_depth_l1` is added when `dataset[idx][1]` is a depth.  `pipe` is accepted for the
    signature's sake (the native forward has no Python covariance / SH option).  The views are scored in batches of
    `chunk` (one begin / finish, i.e. one synchronisation, per batch), so that at most `chunk` ground-truth images are
    resident on the device.  `evaluator`: an object with begin / score / finish (per-view "psnr", "ssim", "depth_l1")
    to use instead of a new NativeEvaluator."""
    end_idx = len(frames) - 1
    chosen = [idx for idx in range(0, end_idx, interval) if idx not in kf_indices]
    out = {"mean_psnr": float("nan"), "mean_ssim": float("nan"), "mean_lpips": None}
    if chosen:
        ev = evaluator
        if ev is None:
            f0 = frames[chosen[0]]
            ev = NativeEvaluator(gaussians, background, int(f0.image_height), int(f0.image_width), gaussians._xyz.device,
                                 max_views=min(len(chosen), chunk))
        ps, ss, ds = [], [], []
        for start in range(0, len(chosen), chunk):       # at most `chunk` ground-truth images resident at a time
            ev.begin()
            for idx in chosen[start:start + chunk]:
                item = dataset[idx]
                depth = item[1] if isinstance(item, (tuple, list)) and len(item) > 1 else None
                ev.score(frames[idx], item[0], gt_depth=depth)
            res = ev.finish()
            ps.append(np.asarray(res["psnr"], np.float64))
            ss.append(np.asarray(res["ssim"], np.float64))
            ds.append(np.asarray(res["depth_l1"], np.float64))
        out["mean_psnr"], out["mean_ssim"] = float(np.mean(np.concatenate(ps))), float(np.mean(np.concatenate(ss)))
        depth_l1 = np.concatenate(ds)
        if not np.isnan(depth_l1).all():
            out["mean_depth_l1"] = _nanmean(depth_l1)
    if save_dir is not None:
        d = os.path.join(save_dir, "psnr", str(iteration))
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "final_result.json"), "w", encoding="utf-8") as fh:
            json.dump(out, fh, indent=4)
    return out


def save_gaussians(gaussians, name, iteration, final: bool = False):
    """eval_utils.py:181-190: <name>/point_cloud/final or <name>/point_cloud/iteration_<n>, file point_cloud.ply."""
    if name is None:
        return None
    sub = "point_cloud/final" if final else "point_cloud/iteration_{}".format(str(iteration))
    path = os.path.join(name, sub, "point_cloud.ply")
    gaussians.save_ply(path)
    return path


def save_mesh(gaussians_or_volume, name, iteration=None, final: bool = True, cameras=None, background=None,
              voxel_size: float = 0.02, margin: float = 0.1, min_weight: float = 1.0, clean=None, gt=None, eval_kw=None,
              cull=None, normals: bool = False, preview=None, simplify=None, smooth=None, topology: bool = False, sparse=None,
              volume_preview=None, volume_preview_kw=None, **fuse_kw):
    """The map's surface next to its point cloud: <name>/point_cloud/final/mesh.ply (or iteration_<n>), where
    save_gaussians puts point_cloud.ply.  A tsdf.TSDFVolume is extracted as it stands; a Gaussian model is first fused
    from its own rendered depth at `cameras` (tsdf.fuse_map, which takes `fuse_kw`: depth_mode="median" fuses the median
    depth instead of depth / opacity; `background` defaults to black).  `clean` - a dict of mesh_clean.clean_mesh
    keyword arguments, e.g. dict(keep_largest=1) - drops the floaters before the file is written.  Returns the path, or
    None without a name.  With `gt` - a (verts, faces) mesh or a point tensor [M,3] on the device - the mesh is scored
    against it (mesh_eval.evaluate_mesh, which takes `eval_kw`), the scores are written as mesh_eval.json next to
    mesh.ply, and the dict of scores is returned instead of the path.  `cull` - evaluate_mesh's dict(views=..., ...) - culls
    both meshes by visibility first; the scores then hold culled_pred_faces and culled_gt_faces.  eval_kw=dict(normals=True)
    adds the normal-consistency numbers.  `normals=True` writes the vertex normals of the final mesh
    (mesh_normals.vertex_normals, after `clean`) into mesh.ply.  `preview` - a view as mesh_render.view_tuple takes it -
    writes the shaded frame of the mesh at that view (mesh_render.render_mesh_frame) as mesh_preview.png next to
    mesh.ply (viewer.save_frame: a .ppm without PIL).  `simplify` - a dict of mesh_simplify.simplify_mesh keyword
    arguments, e.g. dict(factor=2) for cells of two voxels (TSDFVolume.extract_mesh) - merges the vertices of every cell
    after `clean` and before the normals, the preview and the scores, so that all three describe the file written.
    `smooth` - a dict of mesh_smooth.smooth_mesh keyword arguments, e.g. dict(iterations=10) - moves the vertices after
    `clean` and before `simplify`.  `topology=True` writes mesh_topology.json next to mesh.ply: the dict of
    mesh_topology.mesh_topology(faces, V, components=True) for the mesh as written.  A
    sparse_tsdf.SparseTSDFVolume is extracted as it stands, too; `sparse` - True, or dict(max_bricks=, origin=) - fuses a
    Gaussian model into one (tsdf.fuse_map's `sparse`).  `volume_preview` - a view as mesh_render.view_tuple takes it -
    writes the shaded ray cast of the VOLUME at that view (tsdf_raycast.raycast_frame, which takes `volume_preview_kw`;
    z_far defaults to 10) as volume_preview.png next to mesh.ply: the surface the volume holds, before extraction, clean-up
    and simplification touched it.  None adds no call."""
    from . import tsdf
    from .ply_io import write_mesh_ply
    if name is None:
        return None
    vol = gaussians_or_volume
    from .sparse_tsdf import SparseTSDFVolume
    if not isinstance(vol, (tsdf.TSDFVolume, SparseTSDFVolume)):
        if cameras is None:
            raise ValueError("save_mesh: a Gaussian model needs the cameras to fuse from")
        if background is None:
            background = torch.zeros(3, device=vol.get_xyz.device)
        if sparse is not None and sparse is not False:
            vol = tsdf.fuse_map(vol, cameras, background, voxel_size, sparse=sparse, **fuse_kw)
        else:
            vol = tsdf.fuse_map(vol, cameras, background, voxel_size, margin=margin, **fuse_kw)
    if smooth is not None:
        verts, faces, colors = vol.extract_mesh(min_weight, clean=clean, simplify=simplify, smooth=smooth)
    elif simplify is not None:
        verts, faces, colors = vol.extract_mesh(min_weight, clean=clean, simplify=simplify)
    else:
        verts, faces, colors = vol.extract_mesh(min_weight) if clean is None else vol.extract_mesh(min_weight, clean=clean)
    sub ="point_cloud/final" if final else "point_cloud/iteration_{}".format(str(iteration))
    path = os.path.join(name, sub, "mesh.ply")
    if normals:
        from .mesh_normals import vertex_normals
        write_mesh_ply(path, verts, faces, colors, normals=vertex_normals(verts, faces)[0])
    else:
        write_mesh_ply(path, verts, faces, colors)
    if preview is not None:
        from .mesh_render import render_mesh_frame
        from .viewer import save_frame
        save_frame(os.path.join(name, sub, "mesh_preview.png"), render_mesh_frame(verts, faces, preview))
    if volume_preview is not None:
        from .tsdf_raycast import raycast_frame
        from .viewer import save_frame
        save_frame(os.path.join(name, sub, "volume_preview.png"),
                   raycast_frame(vol, volume_preview, **{"z_far": 10.0, **(volume_preview_kw or {})}))
    if topology:
        import json
        from .mesh_topology import mesh_topology
        with open(os.path.join(name, sub, "mesh_topology.json"), "w", encoding="utf-8") as fh:
            json.dump(mesh_topology(faces, int(verts.shape[0]), components=True), fh, indent=4)
    if gt is None:
        return path
    import json
    from .mesh_eval import evaluate_mesh
    if cull is not None:
        eval_kw = dict(eval_kw or {}, cull=cull)
    scores = evaluate_mesh((verts, faces), gt, **(eval_kw or {}))
    with open(os.path.join(name, sub, "mesh_eval.json"), "w", encoding="utf-8") as fh:
        json.dump(scores, fh, indent=4)
    return scores
