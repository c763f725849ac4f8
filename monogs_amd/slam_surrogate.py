"""Config-4-shaped run without the dataset: a synthetic 640x480 sequence with fr3_office
intrinsics pushed through the hot-path pieces in the order MonoGS chains them, with the
hyper-parameters of configs/mono/tum/base_config.yaml (40 first-order + 10 second-order tracking
iterations per frame :250-268, window 8 / pose window 3 :31-32, 150 mapping iterations per
keyframe :26, densify every 150 at offset 50 :27-28, opacity reset :31, 1050 initialisation
iterations :20-24; `single_thread: True`, i.e. tracking and mapping alternate in one process).

TUM fr3_office itself is not available offline (BASELINE.json config 4); if a copy is mounted,
point MONOGS_TUM_DIR at it and `load_sequence` reads it through eval_metrics.TUMSequence instead
of rendering the synthetic world.  Nothing is downloaded.

What is mirrored (/root/reference utils/slam_frontend.py, slam_backend.py):
  initialisation       frontend.initialize :236-267 + add_new_keyframe(init) :183-230,
                       backend "init" message :413-425 -> initialize_map
  per frame            tracking :340-902 from the previous pose (NativeTracker: first order until
                       converged, then the sketched LM iterations), median depth :900
  keyframe insertion   add_new_keyframe :183-230 (monocular: rendered depth, outliers replaced by the
                       median, noise), backend "keyframe" message :427-493 (extend_from_pcd_seq, new
                       keyframe optimiser, map(iters), map(prune=True))
  keyframe policy      by default NOT the reference's: a keyframe every `kf_interval` frames, window =
                       the newest `window_size` keyframes.  With keyframe_policy=KeyframePolicy(...) the
                       reference's: is_keyframe / add_to_window / the run loop's decision :1692-1783,
                       :1914-1956 (keyframe_policy.py), including the monocular reset :1942-1950.
"""
from __future__ import annotations

import math
import os
import time
from types import SimpleNamespace
from typing import List, Optional

import torch

from . import synthetic as S
from .gaussian_model import GaussianModel
from .keyframe_policy import KeyframePolicy
from .mapping_native import NativeMapper
from .pose import SE3_exp
from .slam_loops import GaussianParams, Pipe, ViewCamera
from .tracking_native import NativeTracker


class Frame:
    """One input frame: image [3,H,W] (or, for a run that undistorts natively, the raw uint8 [H,W,3]), optional sensor
    depth [H,W], ground-truth pose.  `undistorted`: the reader already remapped the image with a distorted calibration
    (run_sequence refuses to remap such a frame a second time).  `image_right`: the right image of a stereo pair, in
    the left image's format (run_sequence(stereo_matcher=...) makes the frame's depth from the two)."""

    def __init__(self, uid, image, depth, T_gt, undistorted: bool = False, image_right=None):
        self.uid, self.image, self.depth, self.T_gt, self.undistorted = uid, image, depth, T_gt, undistorted
        self.image_right = image_right


def make_world(n_gaussians: int, W: int, H: int, poses: List[torch.Tensor], seed: int = 0, sigma_px: float = 2.5):
    """A static world of Gaussians that fills the view frusta along the trajectory: a third of
    them are placed (as synthetic.make_scene places them) in front of the first, the middle and the
    last pose each.  Returns slam_loops.GaussianParams on the CPU."""
    anchors = [poses[0], poses[len(poses) // 2], poses[-1]]
    parts = []
    for k, T in enumerate(anchors):
        sc = S.make_scene(n_gaussians // 3, W, H, seed=seed + 17 * k)
        R, t = T[:3, :3], T[:3, 3]
        xyz_w = (sc.means3D - t) @ R                         # camera -> world: R^T (p - t)
        # (orientations are random, so they are left as drawn)
        scale = sc.log_scales + math.log(sigma_px / 1.5)
        parts.append((xyz_w, scale, sc.rot, sc.opacity_logit + 1.0, sc.features_dc))
    cat = [torch.cat([p[i] for p in parts]) for i in range(5)]
    return GaussianParams(*cat)


def trajectory(n_frames: int, step=(0.012, -0.006, 0.008, 0.004, -0.003, 0.002)) -> List[torch.Tensor]:
    """World-to-camera poses of a smooth hand-held-like motion: ~1.6 cm and ~0.3 deg per frame."""
    tau = torch.tensor(step)
    return [SE3_exp(k * tau) for k in range(n_frames)]


def load_sequence(n_frames: int, W: int = 640, H: int = 480, dev="cuda", world_gaussians: int = 150_000, seed: int = 0,
                  sigma_px: float = 2.5, calibration: Optional[dict] = None, raw: bool = False,
                  stereo_baseline: Optional[float] = None):
    """(frames, camera, source): the mounted TUM sequence if MONOGS_TUM_DIR is set, else frames
    rendered from a synthetic world along `trajectory`.  `calibration`: a MonoGS Dataset.Calibration dict; the camera
    is built from its fx, fy, cx, cy.  A mounted sequence with a `distorted` calibration is, by default, undistorted on
    the host (TUMSequence(calibration=...)): the frames are pinhole images, marked `undistorted`, for a run_sequence
    WITHOUT the calibration in its config.  `raw=True` hands the frames over as they are on disk (float [3,H,W], still
    distorted) with the same camera: the input of run_sequence(native_frame_prepare=True, config=<with that
    Dataset.Calibration>), which undistorts them on the device.  Synthetic frames are rendered with the pinhole camera
    and are never marked: no distorted image exists to read.  `stereo_baseline` (synthetic frames only): every frame
    also gets `image_right`, the view of a second camera shifted by the baseline along the left camera's +x, and both
    views are quantised to grey uint8 [H,W] (stereo_depth.to_grey_numpy's rule for a float image) - a rectified pair
    whose disparity is fx * baseline / depth; `depth` stays the left view's rendered depth."""
    cam = S.make_camera(W, H, intrinsics=None if calibration is None else tuple(
        float(calibration[k]) for k in ("fx", "fy", "cx", "cy")))
    tum = os.environ.get("MONOGS_TUM_DIR")
    if tum and os.path.isdir(tum):
        if stereo_baseline is not None:
            raise ValueError("stereo_baseline renders a second view of the synthetic world; a mounted sequence has none")
        from .eval_metrics import TUMSequence
        from .frame_prepare import calibration_remap
        seq = TUMSequence(tum, calibration=None if raw else calibration)
        done = not raw and calibration_remap(calibration) is not None
        frames = []
        for k in range(min(n_frames, len(seq))):
            img, depth, T = seq[k]
            frames.append(Frame(k, img.to(dev), None if depth is None else depth.to(dev), T, undistorted=done))
        return frames, cam, f"TUM sequence at {tum}"
    from .gaussian_renderer import render
    poses = trajectory(n_frames)
    world = make_world(world_gaussians, W, H, poses, seed=seed, sigma_px=sigma_px)
    world = GaussianParams(*(t.to(dev) for t in (world._xyz.data, world._scaling.data, world._rotation.data,
                                                 world._opacity.data, world._features_dc.data)))
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    bg = torch.zeros(3, device=dev)
    frames = []

    def grey_u8(img):
        k = (img.to(torch.float32) * 255.0).round().clamp(0, 255).to(torch.int64)
        return ((4899 * k[0] + 9617 * k[1] + 1868 * k[2] + 8192) >> 14).to(torch.uint8)

    with torch.no_grad():
        for k, T in enumerate(poses):
            v = ViewCamera(k, torch.zeros(3, H, W), T, cam.projmatrix_raw, fovx, fovy, H, W, dev)
            pkg = render(v, world, Pipe, bg)
            image, depth = pkg["render"].clamp(0, 1).clone(), pkg["depth"][0].clone()
            if stereo_baseline is None:
                frames.append(Frame(k, image, depth, T))
                continue
            Tr = T.clone()
            Tr[0, 3] -= float(stereo_baseline)                    # the right camera's centre: +baseline along the left's x
            vr = ViewCamera(k, torch.zeros(3, H, W), Tr, cam.projmatrix_raw, fovx, fovy, H, W, dev)
            right = render(vr, world, Pipe, bg)["render"].clamp(0, 1)
            frames.append(Frame(k, grey_u8(image), depth, T, image_right=grey_u8(right)))
    return frames, cam, f"synthetic world, {world_gaussians} Gaussians, {n_frames} frames @ {W}x{H}"


def _median_depth(depth, opacity, mask=None):
    """get_median_depth (utils/slam_utils.py:286-297) with the std."""
    valid = (depth > 0) & (opacity > 0.95)
    if mask is not None:
        valid = valid & mask
    d = depth[valid]
    if d.numel() < 2:
        return None, None, valid
    return d.median(), d.std(), valid


def keyframe_depth(frame_image, depth, opacity, sensor_depth=None, generator=None, rgb_boundary_threshold=0.01):
    """add_new_keyframe (utils/slam_frontend.py:183-234): the depth map a new keyframe's Gaussians
    are back-projected with.  Monocular: the depth rendered at the tracked pose, outliers (beyond one
    std of the median, or not opaque) replaced by the median, plus noise; first keyframe: 2 m +- 0.3.
    With a depth sensor: the observed depth.  Pixels without image content are dropped (depth 0)."""
    valid_rgb = (frame_image.sum(dim=0) > rgb_boundary_threshold)[None]
    dev = frame_image.device
    if sensor_depth is not None:
        d = sensor_depth.reshape(1, *frame_image.shape[1:]).clone()
    elif depth is None:
        d = 2 * torch.ones(1, *frame_image.shape[1:], device=dev)
        d += torch.randn(d.shape, device=dev, generator=generator) * 0.3
    else:
        d = depth.detach().clone()
        med, std, valid = _median_depth(d, opacity.detach(), valid_rgb)
        if med is None:
            d = 2 * torch.ones_like(d)
        else:
            bad = (d > med + std) | (d < med - std) | ~valid
            d[bad] = med
            d = d + torch.randn(d.shape, device=dev, generator=generator) * torch.where(bad, std * 0.5, std * 0.2)
    d[~valid_rgb] = 0
    return d[0]


def run_sequence(frames, cam, dev, *, sensor_depth: bool = False, kf_interval: int = 5, window_size: int = 8,
                 init_iters: int = 1050, mapping_iters: int = 150, first_order_iters: int = 40,
                 second_order_iters: int = 10, seed: int = 0, config: Optional[dict] = None, log=None,
                 use_first_order_best: bool = True, use_best_loss: bool = True, rgbd_tracking: bool = False,
                 alpha: float = 0.95, num_pixels: int = -1, keyframe_policy: Optional[KeyframePolicy] = None,
                 native_keyframe_seed: bool = False, native_frame_prepare: bool = False, track_on_edges: bool = False,
                 stereo_matcher=None, second_order_exact: bool = False, viewer_every: int = 0,
                 viewer_modes=("rgb",), viewer_follow: bool = True, mesh_volume=None, mesh_every: int = 1,
                 mesh_preview_every: int = 0, mesh_preview_kw=None, icp_init: bool = False, icp_kw=None):
    """Tracking + mapping over `frames`; returns a dict with the estimated poses, timings and the
    final map.  `sensor_depth`: insert keyframes from the frames' depth (RGB-D initialisation) instead
    of the monocular prior / rendered depth.  `rgbd_tracking` (needs sensor_depth): track every frame with
    the stacked RGB-D objective against its depth (NativeTracker(gt_depth=..., alpha=alpha)).  `num_pixels` > 0: the
    first-order tracking iterations take the pixel-sampled gradient (NativeTracker(num_pixels=...); see
    slam_loops.sampled_num_pixels for reading it from a config).  `keyframe_policy`: None inserts a keyframe every
    `kf_interval` frames into a FIFO window; a KeyframePolicy decides every tracked frame the reference's way
    (keyframe_policy.py; its window_size and kf_interval are used), and a monocular reset re-initialises a fresh map
    on the frame that triggered it, at its ground-truth pose - the reference's loop reads that frame again
    (:1942-1950, initialize :236-252).  The result then also holds `decisions` (one per tracked frame), `windows`
    (the window after each tracked frame) and `resets` (the frames that re-initialised the map).
    `native_keyframe_seed`: the three insertion sites (first frame, reset, keyframe) go through
    keyframe_seed.KeyframeSeeder (one mgs_keyframe_seed call and one host read each) instead of keyframe_depth +
    extend_from_pcd_seq; the result then also holds `seed_records` ({frame: the call's record}).
    `native_frame_prepare`: every frame goes through one frame_prepare.FramePreparer (one mgs_frame_prepare call, the
    reference's per-frame compute_grad_mask) when its camera is made, inside the timed tracking section (frame 0:
    initialisation): the camera's grad_mask, rgb_pixel_mask, rgb_pixel_mask_mapping (and gt_depth with `sensor_depth`)
    are the preparer's, with Training.edge_threshold / rgb_boundary_threshold and Dataset.type from `config`; the
    result then also holds `t_prepare`, the host time spent enqueuing those calls.  The preparer is built from `config`,
    so a Dataset.Calibration with `distorted: True` there turns the undistortion on (mgs_frame_prepare_remapped, the map
    built once on the device): the frames must then be RAW, distorted images - load_sequence(calibration=..., raw=True)'s
    float [3,H,W], or uint8 [H,W,3] (TUMSequence.image_u8) - and frames a reader already undistorted
    (load_sequence(calibration=...) without raw) are refused.  Every camera's original_image is then the preparer's
    undistorted image, and everything downstream of the camera - keyframe seeding (keyframe_depth's content mask, the
    seeder's colours) and evaluate()'s PSNR - reads that image, never the raw frame.  The sensor depth is left as it
    is, as the reference's dataset leaves it.  `track_on_edges` (needs
    native_frame_prepare): tracking takes rgb_pixel_mask, upstream MonoGS's high-gradient pixels, as its pixel mask.
    `stereo_matcher`: a stereo_depth.StereoMatcher; every frame then carries a pair (`image`, `image_right`), its depth
    is the matcher's (one mgs_stereo_depth call when its camera is made), the
    camera's image is the matcher's rectified left image, and from there the run is `sensor_depth=True`'s with that
    depth in the place of `frame.depth` - what the reference's stereo dataset hands its frontend.
    `second_order_exact` (slam_loops.second_order_exact reads it from a config): the second-order iterations are dense
    Gauss-Newton steps (NativeTracker.enable_second_order(exact=True)) instead of sketched ones.
    `viewer_every` = k > 0: after every k-th tracked frame (and its keyframe work), outside the timed sections, a
    viewer.NativeViewer takes one frame per mode of `viewer_modes` of the map as it then is - from the follow-camera
    behind the tracked pose (`viewer_follow`) or from the tracked camera itself - with the keyframe frusta, the current
    camera and the trajectory so far drawn over it; the result then also holds `view_frames`:
    {frame id: {mode: uint8 [H,W,3] device tensor}}.  Tracking and mapping never read anything the viewer writes.
    `mesh_volume`: a caller-owned sparse_tsdf.SparseTSDFVolume; every `mesh_every`-th keyframe (the first frame is
    keyframe 0) is integrated into it as the run goes, after its mapping and outside the timed sections - from the
    frame's sensor depth with the camera's image when there is one (`sensor_depth`, a stereo matcher), else from the
    map's rendered view at the keyframe's pose (integrate_view) - which a dense box, sized from a finished map, cannot
    serve.  The result then also holds `mesh_keyframes`, the keyframes fused.  Tracking and mapping read nothing the
    volume writes; None leaves the run as it is.  `mesh_preview_every` = m > 0 (needs mesh_volume): after every m-th
    keyframe fused, the volume is ray cast at that keyframe's tracked pose (tsdf_raycast.raycast_frame, which takes
    `mesh_preview_kw`; z_far defaults to 10) - no mesh, no host read, so the stream does not stall - and the result
    also holds `mesh_previews`: {frame id: uint8 [H,W,3] device tensor}.  0 adds no call.
    `icp_init` (needs mesh_volume and a sensor or stereo depth): every tracked frame, once the volume holds a keyframe,
    first ray casts the volume at the previous frame's pose and aligns the frame's depth to it (icp.track_against_volume,
    which takes `icp_kw`); the tracker's camera starts from the ICP pose when its status is converged or out of
    iterations, else from the previous pose as without it - chosen on the device by the status word, no host read, inside
    the timed tracking section.  The result then also holds `icp_records`: {frame id: icp.read_record's dict}, read once
    after the run.  icp_kw=dict(photo_weight=...) > 0 adds the photometric rows (icp.align's RGB-D path): the camera's
    original_image goes with the depth, the volume must have been fused with colour (it is, from a sensor depth with an
    image), and the records carry "photo" and "sum_ri2".  False makes no ICP or ray-cast call."""
    if icp_init and (mesh_volume is None or not (sensor_depth or stereo_matcher is not None)):
        raise ValueError("icp_init needs mesh_volume and a sensor or stereo depth (sensor_depth=True or a stereo_matcher)")
    if icp_init and stereo_matcher is None and any(f.depth is None for f in frames):
        raise ValueError("icp_init needs a depth image in every frame")
    if stereo_matcher is not None:
        if any(getattr(f, "image_right", None) is None for f in frames):
            raise ValueError("stereo_matcher needs image_right in every frame (load_sequence(stereo_baseline=...))")
        sensor_depth = True
    if track_on_edges and not native_frame_prepare:
        raise ValueError("track_on_edges needs native_frame_prepare=True (the edge mask is the preparer's)")
    if rgbd_tracking and (not sensor_depth or (stereo_matcher is None and any(f.depth is None for f in frames))):
        raise ValueError("rgbd_tracking needs sensor_depth=True and a depth image in every frame")
    policy = keyframe_policy
    if policy is not None:
        window_size, kf_interval = policy.window_size, policy.kf_interval
        policy.reset_state()
    H, W = cam.H, cam.W
    fovx, fovy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    gen = torch.Generator(device=dev).manual_seed(seed)
    bg = torch.zeros(3, device=dev)
    cfg = {"Training": {"window_size": window_size, "monocular": True},
           "Dataset": {"sensor_type": "depth" if sensor_depth else "monocular", "pcd_downsample": 64,
                       "pcd_downsample_init": 32, "point_size": 0.01, "adaptive_pointsize": True}}
    for k, v in (config or {}).items():
        cfg.setdefault(k, {}).update(v)
    gm = GaussianModel(0, config=cfg, device=dev)
    gm.init_lr(6.0)
    gm.training_setup()
    mapper = NativeMapper(gm, bg, config=cfg, cameras_extent=6.0, seed=seed)
    seeder, seed_records = None, {}
    if native_keyframe_seed:
        from .keyframe_seed import MODE_INITIAL, MODE_RENDERED, MODE_SENSOR, KeyframeSeeder
        seeder = KeyframeSeeder(H, W, dev, cfg, isotropic=gm.isotropic, max_sh_degree=gm.max_sh_degree)
    preparer, t_prepare = None, 0.0
    if native_frame_prepare:
        from .frame_prepare import FramePreparer
        preparer = FramePreparer(H, W, dev, cfg)
        if preparer.map_q5 is not None and any(getattr(f, "undistorted", False) for f in frames):
            raise ValueError("the frames were undistorted by their reader and config's Dataset.Calibration would remap "
                             "them again: read them with load_sequence(..., raw=True) or drop the calibration")
    if preparer is None and stereo_matcher is None and any(f.image.dtype == torch.uint8 for f in frames):
        raise ValueError("uint8 frames need native_frame_prepare=True (the preparer converts them)")

    stereo_depths = {}

    def depth_of(fr: Frame):
        """The frame's sensor depth [H,W]: its own, or the one the matcher made when its camera was."""
        return stereo_depths[fr.uid][0] if stereo_matcher is not None else fr.depth

    def insert(gm_, fr: Frame, view, k, init, depth=None, opacity=None):
        """New Gaussians of keyframe k: add_new_keyframe's depth map, then create_pcd + extend_from_pcd.  The image
        is the camera's (the frame's own, or the preparer's undistorted one), never the raw frame."""
        if seeder is None:
            dm = keyframe_depth(view.original_image, depth, opacity, depth_of(fr) if sensor_depth else None, gen)
            gm_.extend_from_pcd_seq(view, kf_id=k, init=init, depthmap=dm, generator=gen)
            return
        if sensor_depth:
            mode, depth, opacity = MODE_SENSOR, depth_of(fr), None
        else:
            mode = MODE_INITIAL if depth is None else MODE_RENDERED
        seed_records[k] = gm_.extend_from_keyframe(seeder, view, view.original_image, depth, opacity, mode, init,
                                                   seed * 1_000_003 + k, kf_id=k)

    def camera(fr: Frame, T):
        # (a raw uint8 [H,W,3] frame: the camera starts empty and the preparer below converts the frame into it)
        image = fr.image
        if stereo_matcher is not None:                  # the pair becomes the camera's image and the frame's depth
            rectified = SimpleNamespace()
            stereo_depths[fr.uid] = stereo_matcher.compute_into(rectified, fr.image, fr.image_right)
            image = rectified.original_image
        first = image if image.dtype != torch.uint8 else torch.zeros(3, H, W, device=dev)
        v = ViewCamera(fr.uid, first, T, cam.projmatrix_raw, fovx, fovy, H, W, dev,
                       intrinsics=(cam.fx, cam.fy, cam.cx, cam.cy))
        v.T_gt = fr.T_gt
        if preparer is not None:
            nonlocal t_prepare
            tp = time.perf_counter()
            preparer.prepare_into(v, image, depth_of(fr) if sensor_depth else None)
            t_prepare += time.perf_counter() - tp
        return v

    view_frames, viewer = {}, None

    def take_views(k):
        """The viewer's frames of the map after frame k (viewer_every): outside the timed sections."""
        nonlocal viewer
        from .viewer import NativeViewer, follow_camera
        if viewer is None or viewer.gaussians is not gm:        # (a monocular reset starts a fresh map)
            viewer = NativeViewer(gm, bg, H, W, dev)
        vp_k = cams[k]
        vcam = follow_camera(vp_k.T, H, W, fovy, behind=True, device=dev) if viewer_follow else vp_k
        c2w = {i: torch.linalg.inv(cams[i].T.detach()) for i in sorted(cams)}
        overlay = dict(keyframes=torch.stack([c2w[i] for i in kf_ids]), current=c2w[k],
                       trajectory=torch.stack([c2w[i][:3, 3] for i in sorted(c2w)]))
        for _ in range(3):
            shots = {m: viewer.frame(vcam, m, **overlay) for m in viewer_modes}
            if viewer.check_capacity():
                break
        else:
            raise RuntimeError("viewer: pair capacity still exceeded after growing the workspaces three times")
        view_frames[k] = shots

    mesh_keyframes, n_keyframes, mesh_previews = [], 0, {}

    def fuse_keyframe(k, fr):
        """Keyframe k into `mesh_volume` (every mesh_every-th one): outside the timed sections."""
        nonlocal n_keyframes
        n_keyframes += 1
        if mesh_volume is None or (n_keyframes - 1) % max(1, int(mesh_every)) != 0:
            return
        v = cams[k]
        if sensor_depth:
            img = v.original_image
            img = img if torch.is_tensor(img) and img.dtype == torch.float32 and img.dim() == 3 else None
            mesh_volume.integrate(depth_of(fr), v.T.detach(), v.fx, v.fy, v.cx, v.cy, image=img)
        else:
            mesh_volume.integrate_view(gm, v, bg)
        mesh_keyframes.append(k)
        if mesh_preview_every > 0 and (len(mesh_keyframes) - 1) % int(mesh_preview_every) == 0:
            from .tsdf_raycast import raycast_frame
            mesh_previews[k] = raycast_frame(mesh_volume, v, **{"z_far": 10.0, **(mesh_preview_kw or {})})

    icp_raw = {}

    def icp_start(k, fr, vp, T_prev):
        """vp.T <- the ICP pose of the frame against the volume's ray cast at T_prev, if its status is ok (on the device)."""
        from . import icp as _icp
        kw = dict(icp_kw or {})
        if float(kw.get("photo_weight", 0.0)) > 0.0:      # RGB-D alignment: the camera's image against the ray cast's colour
            kw.setdefault("image", vp.original_image)
        res = _icp.track_against_volume(mesh_volume, depth_of(fr), T_prev, vp, read=False, **kw)
        with torch.no_grad():
            vp.T.copy_(_icp.select_pose(res, vp.T))
        icp_raw[k] = res["record"]

    t_track = t_map = 0.0
    n_track_iters = n_map_iters = n_map_views = 0
    cams = {}
    # ---- initialisation (frame 0 fixes the world frame at its ground-truth pose) ----
    f0 = frames[0]
    cams[0] = camera(f0, f0.T_gt.to(dev).float().clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    insert(gm, f0, cams[0], 0, True)
    mapper.add_keyframe(0, cams[0])
    mapper.set_window([0])
    mapper.initialize_map(0, iters=init_iters)
    torch.cuda.synchronize()
    t_init = time.perf_counter() - t0
    fuse_keyframe(0, f0)
    window = [0]
    kf_ids = [0]
    last_kf = 0
    decisions, windows, resets = [], [], []
    for k in range(1, len(frames)):
        fr = frames[k]
        if preparer is None:
            vp = camera(fr, cams[k - 1].T.detach().clone())       # previous pose (:358-362)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if preparer is not None:                                  # the frame's preparation is part of its tracking time
            vp = camera(fr, cams[k - 1].T.detach().clone())
        if icp_init and mesh_keyframes:
            icp_start(k, fr, vp, cams[k - 1].T.detach())
        trk = NativeTracker(vp, gm, bg, gt_depth=depth_of(fr) if rgbd_tracking else None, alpha=alpha,
                            num_pixels=num_pixels, sample_seed=seed + k,
                            mask=vp.rgb_pixel_mask if track_on_edges else None)
        if second_order_iters > 0:
            trk.enable_second_order(stack_dim=16, sketch_dim=64, initial_lambda=1e-3, seed=seed + k,
                                    exact=second_order_exact)
        # one frame of the reference's loop incl. its best-iterate bookkeeping (slam_frontend.py:455-822;
        # use_first_order_best / use_best_loss as in configs/mono/tum/base_config.yaml:268-273); the
        # tracker's depth / opacity / n_touched buffers end up rendered at the best iterate
        it = trk.run(max_iters=first_order_iters, check_every=10, second_order_iters=second_order_iters,
                     use_first_order_best=use_first_order_best, use_best_loss=use_best_loss)
        torch.cuda.synchronize()
        t_track += time.perf_counter() - t0
        n_track_iters += it
        cams[k] = vp
        if policy is None:
            create_kf = k - last_kf >= kf_interval
            new_window = ([k] + window)[:window_size]
        else:
            dec = policy.decide(k, cams, window, trk, mapper.occ_aware_visibility)
            decisions.append(dec)
            create_kf, new_window = dec.create_kf, dec.window
            if dec.reset:
                # frontend.initialize + BackEnd.reset: a fresh map from this frame at its ground-truth pose
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                resets.append(k)
                policy.reset_state()
                gm = GaussianModel(0, config=cfg, device=dev)
                gm.init_lr(6.0)
                gm.training_setup()
                mapper = NativeMapper(gm, bg, config=cfg, cameras_extent=6.0, seed=seed)
                cams[k] = camera(fr, fr.T_gt.to(dev).float().clone())
                insert(gm, fr, cams[k], k, True)
                mapper.add_keyframe(k, cams[k])
                mapper.set_window([k])
                mapper.initialize_map(k, iters=init_iters)
                torch.cuda.synchronize()
                t_init += time.perf_counter() - t0
                window, kf_ids, last_kf = [k], [k], k
                windows.append(list(window))
                fuse_keyframe(k, fr)
                if viewer_every > 0 and k % viewer_every == 0:
                    take_views(k)
                continue
        if create_kf:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            insert(gm, fr, vp, k, False, trk.depth, trk.opacity)
            window = new_window
            kf_ids.append(k)
            last_kf = k
            mapper.add_keyframe(k, vp)
            full = len(window) == window_size
            ba = full and not mapper.initialized            # initial BA: all but one keyframe's pose, 300 its (:440-451)
            mapper.set_window(window, frames_to_optimize=window_size - 1 if ba else None)
            iters = mapping_iters
            mapper.map(window, iters=iters)
            mapper.map(window, prune=True)
            torch.cuda.synchronize()
            t_map += time.perf_counter() - t0
            n_map_iters += iters
            n_map_views += iters * (len(window) + min(2, len(kf_ids) - len(window)))
            if log:
                log(f"keyframe {k}: window {window}, {len(gm)} Gaussians, loss {float(mapper.last_loss):.4f}")
            fuse_keyframe(k, fr)
        windows.append(list(window))
        if viewer_every > 0 and k % viewer_every == 0:
            take_views(k)
    ok = mapper.check_capacity()
    result = {"cameras": cams, "kf_ids": kf_ids, "gaussians": gm, "mapper": mapper, "t_init": t_init,
              "t_track": t_track, "t_map": t_map, "n_track_iters": n_track_iters, "n_map_iters": n_map_iters,
              "n_map_views": n_map_views, "capacity_ok": ok, "frames_tracked": len(frames) - 1,
              "decisions": decisions, "windows": windows, "resets": resets}
    if seeder is not None:
        result["seed_records"] = seed_records
    if preparer is not None:
        result["t_prepare"] = t_prepare
    if viewer_every > 0:
        result["view_frames"] = view_frames
    if mesh_volume is not None:
        result["mesh_keyframes"] = mesh_keyframes
        if mesh_preview_every > 0:
            result["mesh_previews"] = mesh_previews
    if icp_init:
        from .icp import read_record
        words = torch.stack([icp_raw[k] for k in sorted(icp_raw)]).cpu().numpy() if icp_raw else []
        rgbd = float((icp_kw or {}).get("photo_weight", 0.0)) > 0.0
        result["icp_records"] = {k: read_record(w, rgbd=rgbd) for k, w in zip(sorted(icp_raw), words)}
    return result


def evaluate(result, frames, dev, every: int = 1, monocular: bool = True, native: bool = False):
    """ATE RMSE over all tracked frames and over the keyframes (Sim(3)-aligned when `monocular`:
    the scale of a monocular map is free; SE(3)-aligned otherwise, eval_utils.py:26-44),
    PSNR of the final map rendered at the estimated poses of the non-keyframes, against each camera's own
    original_image (the frame's image; with a native remap the undistorted one, not the raw frame)."""
    from . import eval_metrics as E
    from .gaussian_renderer import render
    cams, gm = result["cameras"], result["gaussians"]
    ids = sorted(cams)
    ate_all = E.eval_ate(cams, ids, monocular=monocular)
    ate_kf = E.eval_ate(cams, result["kf_ids"], monocular=monocular) if len(result["kf_ids"]) >= 3 else float("nan")
    gt_c = torch.stack([torch.linalg.inv(frames[i].T_gt.double())[:3, 3] for i in ids])
    path = float((gt_c[1:] - gt_c[:-1]).norm(dim=1).sum())
    bg = torch.zeros(3, device=dev)
    if native:
        # the same views through eval_native.NativeEvaluator: one enqueued call per view, one copy at the end.  psnr_db
        # stays the PSNR over ALL elements, as below (psnr_all); ssim and - for a run with sensor depth - depth_l1_m
        # (against the camera's gt_depth, or the frame's depth) come with it.
        from .eval_native import NativeEvaluator
        chosen = [i for i in ids[::every] if i not in result["kf_ids"]]
        res = None
        if chosen:
            v0 = cams[chosen[0]]
            ev = NativeEvaluator(gm, bg, int(v0.image_height), int(v0.image_width), dev, max_views=len(chosen))
            ev.begin()
            for i in chosen:
                v = cams[i]
                depth = None
                if not monocular:
                    depth = getattr(v, "gt_depth", None)
                    if depth is None:
                        depth = getattr(frames[i], "depth", None)
                ev.score(v, v.original_image, gt_depth=depth, apply_exposure=True)
            res = ev.finish()
        out = {"ate_rmse_m": ate_all, "ate_rmse_keyframes_m": ate_kf, "path_length_m": path,
               "psnr_db": res["mean_psnr_all"] if res else 0.0, "psnr_frames": len(chosen), "gaussians": len(gm),
               "ssim": res["mean_ssim"] if res else float("nan")}
        if res and res["mean_depth_l1"] is not None:
            out["depth_l1_m"] = res["mean_depth_l1"]
        return out
    ps = []
    with torch.no_grad():
        for i in ids[::every]:
            if i in result["kf_ids"]:
                continue
            v = cams[i]
            img = render(v, gm, Pipe, bg)["render"]
            img = ((torch.abs(v.exposure_a) + v.exposure_eps) * img + v.exposure_b).clamp(0, 1)
            ps.append(float(E.psnr(img.unsqueeze(0), v.original_image.unsqueeze(0))))
    return {"ate_rmse_m": ate_all, "ate_rmse_keyframes_m": ate_kf, "path_length_m": path,
            "psnr_db": sum(ps) / max(1, len(ps)), "psnr_frames": len(ps), "gaussians": len(gm)}


def reconstruct_mesh(result, voxel_size: float, every_keyframe: int = 1, sensor_depth=None, margin: float = 0.1,
                     min_weight: float = 1.0, clean=None, simplify=None, smooth=None, sparse=None, **fuse_kw):
    """The surface of a finished run: fuses every `every_keyframe`-th keyframe of a run_sequence `result` (its
    "cameras", "kf_ids", "gaussians") into a tsdf.TSDFVolume sized from the map and extracts the mesh:
    (verts [V,3] f32, faces [F,3] i32, colors [V,3] f32) on the device.  By default each keyframe contributes the map's
    own rendered depth at its estimated pose (tsdf.fuse_map); `sensor_depth` - a dict keyframe id -> depth [H,W] in
    the units of the map - fuses measured (sensor or stereo) depth with the keyframe's image instead.  `fuse_kw` goes
    to tsdf.fuse_map: depth_mode="median" fuses the median depth of every rendered view instead of depth / opacity.
    `clean` - a dict of mesh_clean.clean_mesh keyword arguments, e.g. dict(keep_largest=1) - drops the floaters.
    `simplify` - a dict of mesh_simplify.simplify_mesh keyword arguments, e.g. dict(factor=2) for cells of two voxels -
    merges the vertices of every cell afterwards (TSDFVolume.extract_mesh).  `smooth` - a dict of
    mesh_smooth.smooth_mesh keyword arguments, e.g. dict(iterations=10) - moves the vertices after `clean` and before
    `simplify`.  `sparse` - True, or dict(max_bricks=, origin=) - fuses into a sparse_tsdf.SparseTSDFVolume instead
    (tsdf.fuse_map's `sparse`): no bounds pass, no `margin`, memory by the surface seen."""
    from . import tsdf
    gm = result["gaussians"]
    ids = list(result["kf_ids"])[::max(1, int(every_keyframe))]
    cams = [result["cameras"][k] for k in ids]
    if sparse is not None and sparse is not False:
        if sensor_depth is None:
            vol = tsdf.fuse_map(gm, cams, torch.zeros(3, device=gm.get_xyz.device), voxel_size, sparse=sparse, **fuse_kw)
        else:
            vol = tsdf.sparse_volume(sparse, voxel_size, gm.get_xyz.device, trunc=fuse_kw.get("trunc"),
                                     max_weight=fuse_kw.get("max_weight", 64.0))
            for k, cam in zip(ids, cams):
                img = cam.original_image
                img = img if torch.is_tensor(img) and img.dtype == torch.float32 and img.dim() == 3 else None
                vol.integrate(sensor_depth[k], cam.T, cam.fx, cam.fy, cam.cx, cam.cy, image=img,
                              depth_max=fuse_kw.get("depth_max", math.inf))
        return vol.extract_mesh(min_weight, clean=clean, simplify=simplify, smooth=smooth)
    if sensor_depth is None:
        bg = torch.zeros(3, device=gm.get_xyz.device)
        vol = tsdf.fuse_map(gm, cams, bg, voxel_size, margin=margin, **fuse_kw)
    else:
        vol = tsdf.TSDFVolume.for_map(gm, voxel_size, margin, trunc=fuse_kw.get("trunc"),
                                      max_weight=fuse_kw.get("max_weight", 64.0))
        for k, cam in zip(ids, cams):
            img = cam.original_image
            img = img if torch.is_tensor(img) and img.dtype == torch.float32 and img.dim() == 3 else None
            vol.integrate(sensor_depth[k], cam.T, cam.fx, cam.fy, cam.cx, cam.cy, image=img,
                          depth_max=fuse_kw.get("depth_max", math.inf))
    if smooth is not None:
        return vol.extract_mesh(min_weight, clean=clean, simplify=simplify, smooth=smooth)
    if simplify is not None:
        return vol.extract_mesh(min_weight, clean=clean, simplify=simplify)
    if clean is None:
        return vol.extract_mesh(min_weight)
    return vol.extract_mesh(min_weight, clean=clean)


def evaluate_mesh(result, gt, voxel_size: float, monocular: bool = True, mesh_kw=None, cull=None, **kw):
    """The geometry scores of a finished run (mesh_eval.evaluate_mesh: accuracy, completion, precision / recall / F-score,
    Chamfer) against `gt` - a (verts, faces) mesh or a point tensor [M,3] on the device, in the ground truth's frame.  The
    surface is reconstruct_mesh(result, voxel_size, **mesh_kw); it is brought into the ground truth's frame by the
    alignment `evaluate` uses for the ATE over all tracked frames - Sim(3) when `monocular`, SE(3) otherwise - and scored
    with `kw` (n_samples, threshold, seed; normals=True adds the normal-consistency numbers).  `cull` - True, or a dict of mesh_eval.evaluate_mesh's cull keys (occlusion,
    eps, min_views, rule) - applies the visibility protocol first, with the views built from the cameras' ground-truth
    poses T_gt, their intrinsics and their image size (a dict may bring its own `views`)."""
    import numpy as np
    from . import eval_metrics as E
    from .mesh_eval import evaluate_mesh as score
    cams = result["cameras"]
    ids = sorted(cams)
    if cull is not None and cull is not False:
        cull = {} if cull is True else dict(cull)
        if "views" not in cull:
            cull["views"] = [(torch.as_tensor(cams[i].T_gt).float(), cams[i].fx, cams[i].fy, cams[i].cx, cams[i].cy,
                              cams[i].image_height, cams[i].image_width) for i in ids]
        kw["cull"] = cull
    centre = lambda T: np.linalg.inv(torch.as_tensor(T).double().cpu().numpy())[:3, 3]
    est = np.stack([centre(cams[i].T) for i in ids], 1)
    ref = np.stack([centre(cams[i].T_gt) for i in ids], 1)
    R, t, c = E.umeyama_alignment(est, ref, with_scale=monocular)
    verts, faces, _ = reconstruct_mesh(result, voxel_size, **(mesh_kw or {}))
    return score((verts, faces), gt, transform=(c, R, t), **kw)
