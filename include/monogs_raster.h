/* C ABI of the MI355X-native differentiable Gaussian rasteriser + simple-knn.
 *
 * This is the drop-in boundary for the two native extensions MonoGS binds
 * (paths relative to the reference tree /root/reference):
 *
 *   diff_gaussian_rasterization._C.rasterize_gaussians / rasterize_gaussians_backward
 *       - constructed/called at gaussian_splatting/gaussian_renderer/__init__.py:61-77,151-168
 *       - upstream binding: submodules/diff-gaussian-rasterization (git submodule,
 *         .gitmodules:4-7, source absent from the tree)
 *   simple_knn._C.distCUDA2
 *       - called at gaussian_splatting/scene/gaussian_model.py:18,185-191
 *       - upstream binding: submodules/simple-knn (.gitmodules:1-3, source absent)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named host_*; all floats are
 *     fp32, ids/counters int32, sort keys uint64; tensors are dense row-major;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and no
 *     entry point synchronises with the host;
 *   - the library owns no device memory and keeps no state between calls: scratch
 *     lives in caller-owned workspaces whose sizes come from mgs_raster_workspace_query;
 *   - every function returns 0 on success or a negative mgs_status; nothing throws
 *     across this boundary.  mgs_status_string() names a code.
 */
#ifndef MONOGS_RASTER_H
#define MONOGS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_ABI_VERSION 10

typedef enum mgs_status {
  MGS_OK = 0,
  MGS_ERR_BAD_ARGUMENT = -1,   /* null pointer / non-positive size / bad degree */
  MGS_ERR_LAUNCH = -2,         /* hipGetLastError() after a launch was not hipSuccess */
  MGS_ERR_UNSUPPORTED = -3,    /* a size the kernels are not built for (e.g. a backward with pair_capacity > 53 687 091:
                                  the pair records are addressed through a 2-GiB buffer descriptor) */
} mgs_status;

/* Problem shape shared by forward and backward. */
typedef struct mgs_raster_shape {
  int32_t num_gaussians;   /* N >= 1 (N == 0 is handled above the boundary,
                              gaussian_renderer/__init__.py:43-44) */
  int32_t width, height;
  int32_t sh_degree;       /* active degree 0..3 */
  int32_t sh_coeffs;       /* K: coefficient triples stored per Gaussian in `shs` [N,K,3] */
  int32_t pair_capacity;   /* capacity (in (tile,Gaussian) pairs) of the `bins` workspace */
  float tanfovx, tanfovy;
  float scale_modifier;
} mgs_raster_shape;

/* Byte sizes of the caller-owned workspaces for a shape. */
typedef struct mgs_workspace_sizes {
  uint64_t geom_bytes;   /* per-Gaussian records, per-tile ranges, per-pixel blend state;
                            written by forward, read by backward (save it on the autograd ctx) */
  uint64_t bins_bytes;   /* pair_capacity sorted (key, payload) pairs + per-item records, quadrant reach words and blend checkpoints (5 KB + 32 B per 32 pairs and per tile); forward -> backward */
  uint64_t bwd_bytes;    /* backward-only scratch (per-pair reduced gradients, scans) */
  uint64_t sketch_bytes; /* extra backward scratch, only when sketch_mode != 0: 144 B per Gaussian + one 6-KB slab per TWO
                            backward items and per tile, i.e. ~96 B per pair of capacity + 6 KB per tile (no initial state needed) */
  /* byte offsets inside `geom` of arrays tests may inspect */
  uint64_t off_records;      /* N x 48 B  mgs SplatRec                       */
  uint64_t off_pair_count;   /* N x int32 pairs emitted per Gaussian         */
  uint64_t off_tile_offset;  /* (T+1) x int32 exclusive scan of tile counts  */
  uint64_t off_final_T;      /* 256 T x float4 (T, C0, C1, C2), quadrant-major */
  uint64_t off_n_contrib;    /* 256 T x (float depth, int32 n_contrib)       */
  uint64_t off_counters;     /* 4 x int32: [0] = total pairs D               */
  /* byte offsets inside `bins` */
  uint64_t off_keys;         /* capacity x uint64: depth_bits<<32 | gaussian id, sorted per tile */
  uint64_t off_payload;      /* capacity x uint32: pair index within its Gaussian */
} mgs_workspace_sizes;

typedef struct mgs_forward_args {
  mgs_raster_shape shape;
  /* inputs */
  const float* means3D;         /* [N,3] */
  const float* scales;          /* [N,3] or NULL when cov3D_precomp is given */
  const float* rotations;       /* [N,4] (r,x,y,z), used as given */
  const float* cov3D_precomp;   /* [N,6] or NULL */
  const float* opacities;       /* [N] */
  const float* shs;             /* [N,K,3] or NULL when colors_precomp is given */
  const float* colors_precomp;  /* [N,3] or NULL */
  const float* viewmatrix;      /* [4,4] = T_w2c^T     (camera_utils.py:94-96)  */
  const float* projmatrix;      /* [4,4] = view @ proj (camera_utils.py:98-104) */
  const float* projmatrix_raw;  /* [4,4] projection    (slam_frontend.py:1815-1825) */
  const float* campos;          /* >= 3 floats */
  const float* bg;              /* [3] */
  /* workspaces */
  void* geom;
  void* bins;
  /* outputs */
  float* out_color;    /* [3,H,W] */
  float* out_depth;    /* [1,H,W] */
  float* out_opacity;  /* [1,H,W] */
  int32_t* radii;      /* [N] */
  int32_t* n_touched;  /* [N] */
  /* optional, TWO ints: stage 1 also stores [0] = the pair count D and [1] = the largest number of
   * pairs in one tile here.  May be pinned HOST memory (device-accessible): the caller then learns
   * both from an event recorded after stage 1 without a device-to-host copy in the stream. */
  int32_t* pair_count_out;
  /* optional DEVICE counter: stage 1 does atomicMax(*pair_count_max, D).  Never reset by the
   * library, so after any number of fixed-capacity forwards (mgs_tracking_iteration,
   * mgs_mapping_view_iteration) *pair_count_max > pair_capacity says that at least one of them
   * was rendered incompletely, whichever it was. */
  int32_t* pair_count_max;
  /* Stage 2 sorts tiles of up to 1024 pairs in one launch and tiles of 1025..4096 pairs in a second
   * one (16-wave workgroups, 32 KB of LDS) that costs ~6 us even when no such tile exists.
   * 0 (default): always launch it.  -1: skip it - a caller that knows from pair_count_out[1] of the
   * previous, nearly identical view that no tile is that crowded; should one appear after all, the
   * first launch sorts it in place in HBM (slower, same order). */
  int32_t big_tile_pass;
  int32_t reserved0;
} mgs_forward_args;

/* Mapping mode of the backward (row a13, utils/slam_backend.py:171-332): instead of storing
 * the gradients w.r.t. the ACTIVATED attributes of one view, the last kernel of the backward
 * chains them through GaussianModel's activations (gaussian_model.py:54-62,77-102: exp, sigmoid,
 * normalize, cat(features_dc, features_rest)) and accumulates them over the views of the window
 * into the flat buffer the optimiser (and, keyframe-parallel, the all-reduce) consumes - what
 * autograd's accumulation over the summed loss of slam_backend.py:183-247 does - together with
 * the densification statistics of the view (gaussian_model.py:693-697, slam_backend.py:292-299).
 * All pointers are device pointers into caller-owned buffers. */
typedef struct mgs_map_accum_args {
  int32_t scale_dims;           /* 3, or 1: isotropic model, _scaling is [N,1] (renderer broadcast :92-95) */
  int32_t accumulate;           /* 0: overwrite (first view of an iteration), 1: add */
  int32_t add_regulariser;      /* != 0: also add d/d_scaling of  weight * mean|s - mean_k(s)|
                                   (slam_backend.py:244-246; once per iteration, every Gaussian) */
  float regulariser_weight;     /* 10 in the reference */
  const float* raw_rotations;   /* _rotation [N,4] before normalisation */
  float* grad_xyz;              /* [N,3] */
  float* grad_features_dc;      /* [N,1,3] */
  float* grad_features_rest;    /* [N,K-1,3] or NULL when K == 1 */
  float* grad_opacity;          /* [N]   w.r.t. the logit */
  float* grad_scaling;          /* [N,scale_dims] w.r.t. the log scale */
  float* grad_rotation;         /* [N,4] w.r.t. the raw quaternion */
  float* gradnorm_inc;          /* [N] += ||dL/d ndc||  where radii > 0, or NULL */
  float* denom_inc;             /* [N] += 1             where radii > 0, or NULL */
  int32_t* radii_max;           /* [N] max over the views of radii, or NULL */
  uint8_t* visibility;          /* [N] = n_touched > 0 of THIS view (occ-aware visibility,
                                   slam_backend.py:251-255), or NULL */
} mgs_map_accum_args;

typedef struct mgs_backward_args {
  mgs_forward_args fwd;        /* same inputs / workspaces as the forward call */
  const float* grad_color;     /* [3,H,W] */
  const float* grad_depth;     /* [1,H,W] or NULL */
  void* bwd;                   /* bwd_bytes of scratch */
  /* outputs (all overwritten).  The per-Gaussian gradients (means3D, means2D, colors,
   * opacities, scales, rotations, cov3D) may ALL be NULL: pose-only backward (tracking
   * optimises the camera alone, utils/slam_frontend.py:364-392), grad_tau is still produced. */
  float* grad_means3D;         /* [N,3] */
  float* grad_means2D;         /* [N,3]: (dL/dndc_x, dL/dndc_y, 0) - densification statistic,
                                  gaussian_model.py:693-697 */
  float* grad_colors;          /* [N,K,3] when shs, else [N,3] */
  float* grad_opacities;       /* [N] */
  float* grad_scales;          /* [N,3] or NULL */
  float* grad_rotations;       /* [N,4] or NULL */
  float* grad_cov3D;           /* [N,6] or NULL */
  float* grad_tau;             /* [6] = [rho(3); theta(3)]: cam_trans_delta, cam_rot_delta
                                  (pose_utils.py:88-92) */
  /* sketched pose Jacobian (slam_frontend.py:269-338,654-669); sketch_mode 0 = off */
  int32_t sketch_mode;
  int32_t sketch_dim;
  int32_t stack_dim;
  const int32_t* sketch_indices;  /* [stack,H,W] slice for this repeat, bucket id or -1 */
  float* grad_sketch_dtau;        /* [stack,sketch,6] */
  void* sketch_ws;                /* sketch_bytes of scratch (sketch_mode != 0) */
  /* compact alternative to sketch_indices (the buckets of one repeat are disjoint, so one
   * int per pixel suffices): [H,W] = stack * sketch_dim + bucket, or -1.  Used when
   * sketch_indices is NULL. */
  const int32_t* sketch_bucket_flat;
  /* mapping mode (HOST pointer, or NULL): the seven per-Gaussian gradient pointers above must
   * then be NULL, scales / rotations / opacities / shs of `fwd` must be the outputs of
   * mgs_map_activate, and the gradients are chained and accumulated as described above. */
  const mgs_map_accum_args* map_accum;
  /* How the backward treats the field-of-view clamp of the EWA Jacobian, t.x = clamp(x/z) * z
   * (only splats whose centre lies outside 1.3x the field of view are affected; the forward is the
   * same): MGS_CLAMP_GRAD_UPSTREAM = 0 (the default of a zero-initialised block) = t.x held constant
   * in z and its x-gradient zeroed when clamped - what the public CUDA lineage of the absent
   * extension is believed to do, i.e. the gradients the north star's tolerance refers to;
   * MGS_CLAMP_GRAD_EXACT = 1 = the exact derivative of the forward (what plain autograd of the
   * forward gives).  DESIGN.md §2 quantifies the difference.  (ABI 5 had the two values swapped.) */
#define MGS_CLAMP_GRAD_UPSTREAM 0
#define MGS_CLAMP_GRAD_EXACT 1
  int32_t clamp_gradient_mode;
  /* An UPPER BOUND of the forward's pair count D when the caller knows one (the autograd binding has read the
   * exact D from the pinned slot before the backward is enqueued), 0 = none.  Sizes the grid of the blend
   * backward: D / 32 + tiles work items instead of pair_capacity / 32 + tiles.  A value BELOW the true count
   * loses work items - the native entry points, which cannot know D of the forward they have just enqueued,
   * leave it 0.  The kernel notices: counters[2] of the geom workspace (int32 at off_counters + 8, zeroed by every
   * forward) is set to the item count by a backward whose grid did not cover the forward's items - its gradients
   * are then incomplete (the Python binding passes the exact D and checks the word when raster_settings.debug). */
  int32_t pair_count_bound;
} mgs_backward_args;

int32_t mgs_abi_version(void);
/* sizeof() of the argument structs, in declaration order (0 = mgs_raster_shape,
 * 1 = mgs_workspace_sizes, 2 = mgs_forward_args, 3 = mgs_backward_args, 4 = mgs_pose_adam_args,
 * 5 = mgs_mapping_loss_args, 6 = mgs_lm_step_args, 7 = mgs_tracking_loss_args,
 * 8 = mgs_tracking_iter_args, 9 = mgs_sketch_residual_args, 10 = mgs_tracking_so_args,
 * 11 = mgs_adam_group, 12 = mgs_map_plan_args, 13 = mgs_gather_tensor, 14 = mgs_map_gather_args,
 * 15 = mgs_map_accum_args, 16 = mgs_map_activate_args, 17 = mgs_mapping_view_args,
 * 18 = mgs_map_finish_args, 19 = mgs_map_append_args, 20 = mgs_ssim_loss_args,
 * 21 = mgs_refine_view_args, 22 = mgs_tracking_depth_args, 23 = mgs_tracking_sample_args,
 * 24 = mgs_keyframe_args, 25 = mgs_keyframe_seed_args);
 * -1 for an unknown index.  Lets a foreign-language binding verify its struct mirrors. */
int32_t mgs_struct_size(int32_t which);
const char* mgs_status_string(int32_t status);

/* Sizes/offsets of the workspaces for `shape` (uses shape->pair_capacity). */
int32_t mgs_raster_workspace_query(const mgs_raster_shape* shape, mgs_workspace_sizes* out);

/* Forward, stage 1: projection + EWA splat + pair counting + tile scan.
 * Needs `geom` only.  On return (stream order) counters[0] in geom holds D, the
 * number of (tile, Gaussian) pairs; radii is final. */
int32_t mgs_raster_forward_project(const mgs_forward_args* args, void* stream);

/* Forward, stage 2: pair emission, per-tile depth sort, front-to-back blend.
 * Safe for any pair_capacity; results are complete iff D <= pair_capacity. */
int32_t mgs_raster_forward_blend(const mgs_forward_args* args, void* stream);

/* Backward of the whole rasteriser (re-entrant: reads geom/bins, never writes them).
 * MGS_ERR_UNSUPPORTED when shape.pair_capacity * 40 B exceeds 2 GiB. */
int32_t mgs_raster_backward(const mgs_backward_args* args, void* stream);

/* simple-knn: out[i] = mean of the 3 smallest squared distances from points[i] to
 * the other points (exact).  `scratch` must hold mgs_knn_scratch_bytes(P) bytes. */
uint64_t mgs_knn_scratch_bytes(int32_t num_points);
int32_t mgs_knn_dist2(const float* points, int32_t num_points, float* out, void* scratch,
                      void* stream);

/* ---- tracking-loop glue --------------------------------------- */

/* torch.optim.Adam step (betas, eps, bias correction as PyTorch; no weight decay) on the
 * four per-camera parameter groups of utils/slam_frontend.py:364-392, then update_pose
 * (utils/pose_utils.py:88-98): T <- Exp([trans_delta; rot_delta]) T, deltas zeroed,
 * *converged = |tau| < threshold.  State order in exp_avg / exp_avg_sq: rot(3), trans(3),
 * a, b.  A NULL grad skips its group; T == NULL skips the pose update. */
typedef struct mgs_pose_adam_args {
  float* cam_rot_delta;        /* [3] */
  float* cam_trans_delta;      /* [3] */
  float* exposure_a;           /* [1] or NULL */
  float* exposure_b;           /* [1] or NULL */
  const float* grad_rot;
  const float* grad_trans;
  const float* grad_a;
  const float* grad_b;
  float* exp_avg;              /* [8] */
  float* exp_avg_sq;           /* [8] */
  float* T;                    /* [4,4] row-major world-to-camera, updated in place, or NULL */
  int32_t* converged;          /* out, or NULL */
  int32_t step;                /* 1-based */
  float lr_rot, lr_trans, lr_a, lr_b;
  float beta1, beta2, eps;
  float converged_threshold;
  /* optional fusions (NULL / 0 = off), used by mgs_tracking_iteration to save launches:
   * the block partials of dL/dtau ([n,6], instead of grad_trans / grad_rot) and of the exposure
   * gradients ([2,n]: d/da then d/db, instead of grad_a / grad_b) are summed here in index
   * order, and the camera matrices of the UPDATED pose are written (viewmatrix = T^T,
   * projmatrix = viewmatrix @ projection). */
  const float* tau_partials;
  int32_t num_tau_partials;
  const float* exposure_partials;
  int32_t num_exposure_partials;
  const float* projection;
  float* viewmatrix_out;
  float* projmatrix_out;
  /* mgs_mapping_view_iteration extras (all 0 / NULL otherwise).  A NULL parameter pointer
   * (cam_rot_delta, cam_trans_delta, exposure_a, exposure_b) skips that group even when its
   * gradient is available.  no_pose_update != 0: step the deltas but leave T alone (the reference
   * optimises the deltas of `frames_to_optimize` keyframes and applies update_pose to the first
   * `pose_window` only, utils/slam_backend.py:452-474 vs :328-332).  loss_partials: [2,n] block sums of
   * the mapping objective (colour, depth); loss = w_rgb * sum_c + w_depth * sum_d is stored to
   * *loss_view and added to *loss_accum. */
  int32_t no_pose_update;
  const float* loss_partials;
  int32_t num_loss_partials;
  float loss_w_rgb, loss_w_depth;
  float* loss_view;
  float* loss_accum;
  /* loss_norm_mode == 1 (mgs_tracking_iteration): loss_partials are [n] block sums of the squared
   * tracking residuals written by mgs_tracking_loss_onepass together with UN-normalised gradients
   * (the objective is the norm sqrt(sum h^2), its gradient carries 1 / loss; everything between
   * the loss and this kernel is linear in the image gradient).  This kernel forms loss = sqrt(sum),
   * scales every gradient it sums by (*loss_grad_out or 1) / loss before the Adam step and stores
   * loss and 1 / loss to loss_view[0], loss_view[1]. */
  const float* loss_grad_out;
  int32_t loss_norm_mode;
  /* != 0: once *converged is set the kernel does nothing at all (no step, no best-iterate update):
   * the reference leaves its loop at the first converged iteration (utils/slam_frontend.py:623-626);
   * a caller that reads the flag only every few iterations gets the same result. */
  int32_t sticky_converged;
  /* Best-iterate bookkeeping of the tracking loop (utils/slam_frontend.py:423-425, 510, 523-528):
   * l1_partials = [n] block sums of |residual| (UN-Hubered, the reference's
   * loss_tracking_scalar = ||loss_tracking_img||_1) of the render this iteration started from;
   * when their sum is below best[0] the state that was rendered (T, exposure_a, exposure_b BEFORE
   * this step - what TempCamera(viewpoint) copies) is stored: best = float[MGS_TRACK_BEST_FLOATS]
   * {best L1 (caller sets +inf), T[16], a, b, index of the best iteration, iteration counter,
   *  [21] the criterion (L1) of the LAST iteration's render, [22] |step| of the last iteration (|tau| applied by
   *  update_pose, or |x| of the LM solve) - a per-iteration trace for tests and logging, [23] spare}. */
  const float* l1_partials;
  float* best;
  int32_t num_l1_partials;
  /* loss_norm_mode == 1: the objective is the p-norm (sum |h|^p)^(1/p) of utils/slam_frontend.py:596-600
   * (p = 2 with Huber, RGN.pnorm without; configs/mono/tum/base_config.yaml:249); loss_partials are block
   * sums of |h|^p, loss = sum^(1/p) and the gradients are scaled by loss^(1-p).  <= 0 means 2. */
  float loss_pnorm;
} mgs_pose_adam_args;
#define MGS_TRACK_BEST_FLOATS 24

int32_t mgs_pose_adam_step(const mgs_pose_adam_args* args, void* stream);

/* Mapping objective (utils/slam_utils.py:224-253):
 *   loss = w_rgb * mean_{3HW} | m ((|a|+eps) image + b - gt) | + w_depth * mean_{HW} | dm (depth - gt_depth) |
 * m = mask (float 0/1, or NULL), dm = gt_depth > depth_mask_threshold (threshold < 0: no
 * mask).  Monocular: w_rgb = 1, w_depth = 0; RGB-D: w_rgb = alpha, w_depth = 1 - alpha.
 * apply_exposure = 0 is `initialization=True`.  `partial` holds
 * mgs_mapping_loss_partial_count(num_pixels) floats: [4][n] block sums (n = the number of reduction blocks) -
 * sum |colour residual|, sum |depth residual| (written by forward and fused), d/da, d/db (backward and fused) -
 * and one int behind them, the ticket of partial_ticket_ready. */
typedef struct mgs_mapping_loss_args {
  const float* image;        /* [3,H,W] */
  const float* gt;           /* [3,H,W] */
  const float* mask;         /* [1,H,W] or NULL */
  const float* depth;        /* [1,H,W] or NULL (w_depth == 0) */
  const float* gt_depth;     /* [1,H,W] or NULL */
  const float* exposure_a;   /* [1] (apply_exposure != 0) */
  const float* exposure_b;   /* [1] */
  float exposure_eps;
  float w_rgb, w_depth;
  float depth_mask_threshold;
  int32_t apply_exposure;
  int64_t num_pixels;
  float* partial;
  float* loss;               /* [1] out */
  /* backward only */
  const float* grad_out;     /* [1] */
  float* grad_image;         /* [3,H,W] */
  float* grad_depth;         /* [1,H,W] or NULL */
  float* grad_a;             /* [1] or NULL */
  float* grad_b;             /* [1] or NULL */
  /* != 0: the caller guarantees that the int at partial[4 n] (the last slot of the partial count) was zero
   * when the call was enqueued (e.g. a scratch zeroed once and reused: every call restores the zero).
   * mgs_mapping_loss_forward / mgs_mapping_loss_fused then sum the block partials in the workgroup that
   * finishes last instead of launching a second kernel / leaving the sums to the consumer.
   * mgs_mapping_loss_backward ignores it. */
  int32_t partial_ticket_ready;
  int32_t reserved0;
} mgs_mapping_loss_args;

int32_t mgs_mapping_loss_forward(const mgs_mapping_loss_args* args, void* stream);
int32_t mgs_mapping_loss_backward(const mgs_mapping_loss_args* args, void* stream);

/* Sketched Levenberg-Marquardt step (utils/slam_frontend.py:672-697 + TempCamera.step
 * :49-53): solves (SJ^T SJ + lambda I) x = -SJ^T Sf for the 8 unknowns
 * [trans(3), rot(3), exposure_a, exposure_b] (identical to the reference's damped
 * torch.linalg.lstsq), writes x_out[8] and applies T <- Exp(x[:6]) T, exposure += x[6:8]
 * (T / exposure may be NULL to only solve). */
typedef struct mgs_lm_step_args {
  const float* SJ;      /* [rows, 8] */
  const float* Sf;      /* [rows] */
  int32_t rows;
  float lambda;         /* > 0 */
  float* T;             /* [4,4] or NULL */
  float* exposure_a;    /* [1] or NULL */
  float* exposure_b;    /* [1] or NULL */
  float* x_out;         /* [8] */
  /* optional extensions (all NULL / 0 for the plain solve) */
  const float* sj_tau;       /* [rows, 6]: used with sj_exposure when SJ == NULL */
  const float* sj_exposure;  /* [rows, 2] */
  float* lm_state;           /* [4] device-resident trust-region state {lambda, previous loss,
                                has_previous, converged}; when given, `lambda` is ignored and the
                                rule of utils/slam_frontend.py:536-545 runs on the device first:
                                loss < previous ? lambda = max(lambda / decrease, min_lambda)
                                                : lambda = min(lambda * increase, max_lambda) */
  const float* loss;         /* [1] current ||residual||_1 (lm_state only) */
  float increase_factor, decrease_factor, min_lambda, max_lambda;
  float converged_threshold; /* lm_state[3] = |x| < threshold (slam_frontend.py:699) */
  /* With lm_state: a converged step is NOT applied and every later call is a no-op (the reference
   * assigns new_viewpoint_params at slam_frontend.py:690-691 but only APPLIES it at the top of the next
   * iteration, :474-479, and the `break` of :699-706 comes first).  A non-converged step is applied at once
   * here: equal to the reference for every iteration but the LAST of a frame, whose step the reference
   * never applies - a caller that ends a frame on the last rendered state (use_best_loss off) restores it
   * (NativeTracker.run does).
   * best (or NULL): same float[MGS_TRACK_BEST_FLOATS] block as mgs_pose_adam_args.best; *loss is the
   * criterion, the pose / exposure this iteration rendered (before the step) is what is stored. */
  int32_t reserved0;
  float* best;
  /* optional (all three or none): the camera matrices of the STEPPED pose are written here (viewmatrix = T^T,
   * projmatrix = viewmatrix @ projection) - mgs_tracking_iteration_second_order then needs no
   * mgs_camera_from_pose launch in the next iteration (base.camera_matrices_valid) */
  const float* projection;
  float* viewmatrix_out;
  float* projmatrix_out;
  /* optional: zero_count floats at zero_after are set to 0 once every row has been read (the sketch
   * accumulators of the native second-order iteration: their consumer leaves them ready for the next one) */
  float* zero_after;
  int32_t zero_count;
  int32_t reserved1;
} mgs_lm_step_args;

int32_t mgs_lm_solve_step(const mgs_lm_step_args* args, void* stream);

/* Monocular tracking objective (utils/slam_utils.py:188-205, :58-75; norm at
 * utils/slam_frontend.py:596-598):
 *   loss = || Huber_delta( opacity * mask * ((|a| + eps) * image + b - gt) ) ||_p   (p = pnorm, below)
 * huber_delta <= 0 disables Huber.  `partial` holds mgs_tracking_loss_partial_count floats, [4][n] for n
 * reduction blocks: [n] sum |h|^p (forward, onepass, rgbd_fused) | [n] d/da | [n] d/db (backward, onepass,
 * rgbd_fused) | [n] sum |residual| before Huber (onepass, rgbd_fused); an entry leaves the other slots alone,
 * `scalars` 2 floats ([0] = loss, [1] = 1/loss) written by forward and read by backward. */
typedef struct mgs_tracking_loss_args {
  const float* image;          /* [3,H,W] */
  const float* opacity;        /* [1,H,W] */
  const float* gt;             /* [3,H,W] */
  const float* mask;           /* [1,H,W] as float 0/1, or NULL */
  const float* exposure_a;     /* [1] */
  const float* exposure_b;     /* [1] */
  float exposure_eps;
  float huber_delta;
  int64_t num_pixels;          /* H*W */
  float* partial;
  float* scalars;
  /* backward only */
  const float* grad_out;       /* [1] dL/dloss */
  float* grad_image;           /* [3,H,W] */
  float* grad_a;               /* [1] */
  float* grad_b;               /* [1] */
  /* p of the norm, utils/slam_frontend.py:596-600: the reference uses p = 2 when use_huber is on and
   * RGN.pnorm (configs/mono/tum/base_config.yaml:249: 1) when it is off.  <= 0 means 2 (a zero-initialised
   * block keeps the Hubered L2 objective).  p = 1 and p = 2 are closed forms; any other p >= 1 goes
   * through powf.  `partial` then holds block sums of |h|^p, scalars[0] = loss = (sum)^(1/p) and
   * scalars[1] = loss^(1-p), the factor of the norm's derivative. */
  float pnorm;
  int32_t reserved0;
} mgs_tracking_loss_args;

int32_t mgs_tracking_loss_partial_count(int64_t num_pixels);
int32_t mgs_tracking_loss_forward(const mgs_tracking_loss_args* args, void* stream);
int32_t mgs_tracking_loss_backward(const mgs_tracking_loss_args* args, void* stream);
/* ONE launch: block sums of the squared residuals ([n] at partial), UN-normalised image gradient
 * (as if loss were 1) and un-normalised exposure partials ([2,n] at partial + n).  The consumer
 * (mgs_pose_adam_step with loss_norm_mode = 1) applies grad_out / loss.  args->scalars is not
 * written here.  partial + 3n: [n] block sums of |residual| BEFORE Huber (the best-iterate criterion
 * of utils/slam_frontend.py:510).  (reference: utils/slam_utils.py:188-217 get_loss_tracking_rgb + autograd). */
int32_t mgs_tracking_loss_onepass(const mgs_tracking_loss_args* args, int32_t* num_blocks_out, void* stream);


/* ---- native tracking iteration (row a12: utils/slam_frontend.py:493-630) ---------------- */

/* Camera matrices of utils/camera_utils.py:94-108 from the world-to-camera pose:
 * viewmatrix = T^T, projmatrix = viewmatrix @ projection (projection as stored by the
 * reference, i.e. already transposed, camera_utils.py:86-89).  campos is the reference's
 * camera_center, which IS world_view_transform (:106-108): pass the viewmatrix buffer. */
int32_t mgs_camera_from_pose(const float* T, const float* projection, float* viewmatrix,
                             float* projmatrix, void* stream);

/* One first-order monocular tracking iteration, enqueued as a fixed launch sequence with
 * no host round trip (the Python loop body costs ~1 ms of host time per iteration):
 *   camera matrices from T -> rasteriser forward (project + blend at the caller's fixed
 *   pair capacity); the blend pass evaluates the tracking objective in its epilogue (the arithmetic of
 *   mgs_tracking_loss_onepass: d loss / d image into grad_image, the four sums as one partial per 8x8-pixel
 *   quadrant in the geom workspace - loss.partial is not used by this entry) -> pose-only rasteriser
 *   backward -> Adam on (rot, trans, exposure a, b) + update_pose (mgs_pose_adam_step), with
 *   the small reduction kernels and the 1 / loss of the norm folded into their consumers (9 launches).
 * fwd.viewmatrix / fwd.projmatrix / fwd.campos must point at caller-owned device buffers
 * (16/16/>=3 floats; campos may alias viewmatrix) that this call REWRITES from T;
 * fwd.projmatrix_raw is the projection.  The forward is complete iff counters[0] (pair
 * count D, in geom) <= shape.pair_capacity: the caller checks that lazily.  Per-iteration
 * results: loss_scalars[0] = loss, *adam.converged, the updated T / exposure. */
typedef struct mgs_tracking_iter_args {
  mgs_forward_args fwd;
  void* bwd;                  /* bwd_bytes of backward scratch */
  float* grad_image;          /* [3,H,W] scratch: dL/d(render) */
  float* grad_tau;            /* [6] scratch: [rho; theta] */
  float* grad_exposure;       /* [2] scratch: d/da, d/db */
  const float* one;           /* [1] = 1.0f (dL/dloss) */
  mgs_tracking_loss_args loss;   /* image/opacity/grad_* fields are filled in by the call */
  mgs_pose_adam_args adam;       /* grad_* fields are filled in by the call; T must be set */
  int32_t camera_matrices_valid; /* != 0: fwd.viewmatrix / projmatrix already match T (every
                                    mgs_tracking_iteration leaves them so): skip that launch */
  int32_t reserved0;
  float* best;                /* float[MGS_TRACK_BEST_FLOATS] best-iterate block (see mgs_pose_adam_args), or
                                 NULL; shared by the first- and second-order iterations of a frame */
} mgs_tracking_iter_args;

int32_t mgs_tracking_iteration(const mgs_tracking_iter_args* args, void* stream);



/* ---- native second-order (sketched Levenberg-Marquardt) tracking iteration ----------------
 * utils/slam_frontend.py:455-710 with in_second_order = True.
 *
 * mgs_sketch_assign: the CountSketch bookkeeping of :269-338 as one kernel.  The reference
 * draws torch.randperm(H*W) and cuts its first chunk*stack*sketch entries (chunk =
 * H*W / (stack*sketch)) into disjoint buckets; here pixel p gets position q = pi_key(p) of a
 * keyed pseudo-random PERMUTATION of [0, H*W) (invertible multiply / xor-shift rounds on
 * ceil(log2 HW) bits with cycle walking), bucket[p] = q / chunk if q < chunk*stack*sketch else
 * -1, and weights[p] = +-1 from a hash bit.  Same structure (disjoint buckets of exactly
 * `chunk` pixels), no sort, no index tensors. */
int32_t mgs_sketch_assign(int64_t num_pixels, int32_t stack_dim, int32_t sketch_dim, uint64_t key,
                          int32_t* bucket, float* weights, void* stream);

/* Sketched monocular tracking residual (utils/slam_utils.py:188-205 + Huber :58-75 + the
 * bucket sums of slam_frontend.py:636-650 and ApplyExposure's sketched Jacobian
 * slam_utils.py:150-185), one pass over the image:
 *   r_c = opacity * mask * ((|a|+eps) image_c + b - gt_c);  l1 = sum |r_c|
 *   weighted_p = weights_p / (HW / (stack*sketch)) * sum_c Huber(r_c)
 *   Sf[b] += weighted_p;  sj_exposure[b] += d weighted_p / d(a, b);  grad_image = d weighted_p / d image
 * with the derivatives through the exposure taken as the reference's hand-written ApplyExposure.backward takes
 * them (slam_utils.py:145-149; NOT the exact derivative): d/d image carries |a| without eps, d/da carries
 * image WITHOUT sign(a) - identical while exposure_a > 0, pinned for a < 0 by tests/golden/map_update_ref.npz.
 * Sf / sj_exposure / l1 must be zero on entry (they are accumulated with atomics). */
typedef struct mgs_sketch_residual_args {
  const float* image;        /* [3,H,W] */
  const float* opacity;      /* [1,H,W] */
  const float* gt;           /* [3,H,W] */
  const float* mask;         /* [1,H,W] float 0/1 or NULL */
  const float* exposure_a;
  const float* exposure_b;
  float exposure_eps, huber_delta;
  int64_t num_pixels;
  int32_t stack_dim, sketch_dim;
  const int32_t* bucket;     /* from mgs_sketch_assign */
  const float* weights;
  float* grad_image;         /* [3,H,W] out */
  float* Sf;                 /* [stack*sketch] accumulated */
  float* sj_exposure;        /* [stack*sketch, 2] accumulated */
  float* l1;                 /* [1] accumulated */
  /* assign != 0: the partition of mgs_sketch_assign(num_pixels, stack_dim, sketch_dim, assign_key) is
   * evaluated inside this pass and WRITTEN to bucket / weights (which then are outputs): one launch less */
  int32_t assign;
  int32_t reserved0;
  uint64_t assign_key;
} mgs_sketch_residual_args;

int32_t mgs_sketch_residual(const mgs_sketch_residual_args* args, void* stream);

/* One second-order iteration as a fixed launch sequence (no host round trip): camera
 * matrices from T (skipped when base.camera_matrices_valid: the previous iteration's LM kernel wrote them) ->
 * forward -> zero accumulators -> mgs_sketch_residual with the partition of mgs_sketch_assign(key)
 * evaluated inside it -> Jacobian-only backward in sketch mode (grad_sketch_dtau via the compact
 * bucket map; the per-splat sums, the per-Gaussian chain and grad_tau are skipped: the LM step
 * consumes the sketched Jacobian alone) -> mgs_lm_solve_step with the device-resident
 * trust-region state.
 * `base` as for mgs_tracking_iteration (its adam block is unused except T / exposure);
 * `accum` holds repeat*stack*sketch*9 + 4 floats: Sf[R d] | sj_exposure[R d,2] | sj_tau[R d,6] | l1, pad.
 * repeat_dim (RGN.second_order.repeat_dim, configs/mono/tum/base_config.yaml:258; utils/slam_frontend.py:654-669):
 * R backward passes over ONE render, each with its own partition (key + r * golden ratio) and weights; the rows of
 * Sf / SJ are stacked ([R d] rows in the solve).  `bucket` / `weights` then hold R planes of H*W.
 * If a step of the sequence fails after the accumulators were touched, they are cleared before the error is
 * returned, so scratch_kept_zero survives a failed call. */
typedef struct mgs_tracking_so_args {
  mgs_tracking_iter_args base;
  int32_t stack_dim, sketch_dim;
  uint64_t key;              /* changes every iteration */
  int32_t* bucket;           /* [repeat, H*W] scratch */
  float* weights;            /* [repeat, H*W] scratch */
  float* accum;
  void* sketch_ws;           /* sketch_bytes of backward scratch */
  mgs_lm_step_args lm;       /* SJ / Sf / sj_* / loss fields are filled in by the call */
  /* != 0: `accum` was zero-filled before the FIRST call and nobody else writes it; the LM kernel - its consumer -
   * restores the zeros, so no hipMemsetAsync is enqueued per iteration.  (`sketch_ws` needs no initial state:
   * every launch rewrites what it reads - the per-run slabs of Jacobian rows and their masks.) */
  int32_t scratch_kept_zero;
  int32_t repeat_dim;        /* >= 1; 0 means 1 */
} mgs_tracking_so_args;

int32_t mgs_tracking_iteration_second_order(const mgs_tracking_so_args* args, void* stream);

/* ---- RGB-D tracking: the depth residual stacked onto the tracking objective -----------------
 * The reference's unfinished get_loss_tracking_rgbd_per_pixel (utils/slam_utils.py:208-221) with its two terms
 * STACKED along the channel axis instead of added, so that the first-order norm, the best-iterate L1 and the
 * second-order bucket sums all run unchanged on the four rows:
 *   r_c = w_rgb * opacity * mask * ((|a| + eps) image_c + b - gt_c)            c = 0..2 (the monocular rows)
 *   dm  = (gt_depth > depth_threshold) && (opacity > opacity_threshold)        (rendered opacity, not differentiated)
 *   r_d = w_depth * (depth * dm - gt_depth * dm)
 * w_rgb = alpha (config Training.alpha, 0.95 by default), w_depth = 1 - alpha.  Huber acts on the weighted rows.
 * The depth row does not depend on the exposure.  Every *_rgbd entry point takes the monocular argument block
 * unchanged plus this one; grad_depth receives d/d depth where the monocular entry writes d/d image. */
typedef struct mgs_tracking_depth_args {
  const float* depth;          /* [1,H,W] rendered depth (the iteration entry points use fwd.out_depth instead) */
  const float* gt_depth;       /* [1,H,W] sensor depth */
  float* grad_depth;           /* [1,H,W] out (scratch of the iteration entry points) */
  float w_rgb;                 /* alpha */
  float w_depth;               /* 1 - alpha */
  float depth_threshold;       /* 0.01 (slam_utils.py:214) */
  float opacity_threshold;     /* 0.95 (slam_utils.py:215) */
} mgs_tracking_depth_args;

/* mgs_tracking_iteration with the stacked objective: the forward blend's epilogue adds the depth row (grad_depth
 * written there), the pose-only backward consumes grad_depth.  Any p other than 1 and 2 takes
 * mgs_tracking_loss_rgbd_fused (onepass form) between the forward and the backward (loss.partial needed). */
int32_t mgs_tracking_iteration_rgbd(const mgs_tracking_iter_args* args, const mgs_tracking_depth_args* depth,
                                    void* stream);
/* mgs_tracking_iteration_second_order with the stacked objective: the sketched residual pass adds Huber(r_d) to the
 * pixel's bucket, the Jacobian-only sketch backward consumes grad_depth. */
int32_t mgs_tracking_iteration_second_order_rgbd(const mgs_tracking_so_args* args, const mgs_tracking_depth_args* depth,
                                                 void* stream);
/* Stacked objective, value and gradient: ONE pass writes the block sums of mgs_tracking_loss_onepass (partial =
 * [n] sum |h|^p | [n] d/da | [n] d/db | [n] sum |r| over the four rows, n = *num_blocks_out) and the UN-normalised
 * gradients (as if loss^(1-p) were 1) into grad_image and depth->grad_depth.  With scalars != NULL a second launch
 * sums the partials: scalars[0] = loss, scalars[1] = loss^(1-p) (the factor the gradients still need), and
 * grad_a / grad_b (when not NULL) = d loss / d a, d loss / d b including that factor.  `partial` holds
 * mgs_tracking_loss_partial_count floats. */
int32_t mgs_tracking_loss_rgbd_fused(const mgs_tracking_loss_args* args, const mgs_tracking_depth_args* depth,
                                     int32_t* num_blocks_out, void* stream);
/* mgs_sketch_residual with the depth row: hs += Huber(r_d) into the pixel's bucket, l1 += |r_d|,
 * grad_depth = weight * Huber'(r_d) * w_depth * dm. */
int32_t mgs_sketch_residual_rgbd(const mgs_sketch_residual_args* args, const mgs_tracking_depth_args* depth, void* stream);

/* ---- pixel-sampled first-order tracking ("Pixel-sampled first-order tracking") ---------------
 * The reference's RGN.first_order.num_pixels > 0 branch (utils/slam_frontend.py:573-592), with the scaling defined for
 * every norm.  The forward and the objective's value are full-image; only the gradient is estimated:
 *   v_i = sum_c |r_ic| + 1e-8,  q_i = v_i / sum_j v_j,  i_1..i_K iid ~ q,
 *   g = (1/p) Phi^(1-p) (1/K) sum_k grad psi_{i_k} / q_{i_k},  psi_i = sum_c |h(r_ic)|^p,  Phi = (sum_i psi_i)^(1/p)
 * (unbiased for grad Phi: pose and exposure rows alike).  The draw is keyed by `key` (counter-based hash, no host sync)
 * and its flat pixel indices are written to `indices` IN TILE ORDER (16x16 tiles row-major, then 8x8 quadrants,
 * then row-major inside a quadrant): the K draws are generated as sorted uniforms, which is the same distribution
 * as K iid draws.  replay_indices (tests): skip the draw and use these pixels (any order; they are ranked into tile
 * order, an index outside [0, H*W) gets weight 0; O(K^2) work in one workgroup - not for production use). */
#define MGS_TRACK_SAMPLE_MAX 65536
typedef struct mgs_tracking_sample_args {
  int32_t num_samples;             /* K, 1 .. MGS_TRACK_SAMPLE_MAX (else MGS_ERR_UNSUPPORTED) */
  int32_t reserved0;
  uint64_t key;                    /* changes every iteration */
  int32_t* indices;                /* [K] out: drawn flat pixel indices, tile order */
  void* scratch;                   /* mgs_tracking_sample_scratch_bytes(shape, K) bytes, no initial state */
  const int32_t* replay_indices;   /* [K] or NULL */
  float* grad_out;                 /* [8] or NULL: the estimate before the Phi^(1-p) factor - d tau ([rho; theta], the
                                      order of mgs_backward_args.grad_tau), d/da, d/db (tests) */
} mgs_tracking_sample_args;

uint64_t mgs_tracking_sample_scratch_bytes(const mgs_raster_shape* shape, int32_t num_samples);
/* One first-order iteration with the sampled gradient: camera matrices -> forward (plain blend) -> sampling weights
 * and exact objective sums -> draw -> sparse pose backward over the K pixels (no per-Gaussian or per-pixel pass) ->
 * mgs_pose_adam_step with the Phi^(1-p) normalisation and the best-iterate L1, as mgs_tracking_iteration.
 * depth == NULL: monocular; else the stacked RGB-D residual of mgs_tracking_iteration_rgbd.  Any p >= 1. */
int32_t mgs_tracking_iteration_sampled(const mgs_tracking_iter_args* args, const mgs_tracking_depth_args* depth,
                                       const mgs_tracking_sample_args* sample, void* stream);

/* ---- keyframe selection and window management ("Keyframe policy on the device") ----------------------
 * The reference frontend's per-frame decision (utils/slam_frontend.py: is_keyframe :1692-1720, add_to_window
 * :1722-1783, the run loop :1914-1956) from the device-resident inputs, in three stream-ordered launches and with no
 * host synchronisation:
 *   1. median-depth radix pass 1 (bits 31..21) over the valid pixels (depth > 0 && opacity > 0.95) and the
 *      covisibility counts |cur|, |row_w|, |cur & row_w| (cur = n_touched > 0, row_w = visibility[w] != 0);
 *   2. radix pass 2 (bits 20..10) inside the selected bucket;
 *   3. radix pass 3 (bits 9..0), then the workgroup that takes the last ticket selects the lower median
 *      (rank (n - 1) / 2, torch.median's) and evaluates the decision into *result.
 * All counting is integer: two calls give bit-identical records.  The overlap ratios are fp32 divisions of the exact
 * counts (0 / 0 = NaN: compares false), dist is fp32 from T_cur * T_last^-1 (rigid inverse [R^T | -R^T t]), the
 * eviction score takes fp32 norms and fp64 reciprocals / sums / products; ties go to the first position.
 * The window is ordered newest first (window[0] = the last keyframe), as the reference's current_window. */
#define MGS_KF_MAX_WINDOW 16
typedef struct mgs_keyframe_args {
  int32_t num_gaussians;           /* N >= 1 */
  int32_t num_pixels;              /* H * W >= 1 */
  int32_t window_len;              /* W, 1 .. MGS_KF_MAX_WINDOW (above: MGS_ERR_UNSUPPORTED) */
  int32_t window_size;             /* Training.window_size >= 1 */
  int32_t check_time;              /* (cur_frame_idx - window[0]) >= kf_interval */
  int32_t initialized;             /* the frontend's flag (set once the window has been full; !monocular at start) */
  int32_t monocular;
  int32_t single_thread;           /* Dataset.single_thread: create_kf &= check_time */
  float kf_translation, kf_min_translation, kf_overlap, kf_cutoff;
  const int32_t* n_touched;        /* [N] current frame's render (tracking's best iterate) */
  const float* depth;              /* [H*W] */
  const float* opacity;            /* [H*W] */
  const float* T_cur;              /* [4][4] row-major world-to-camera pose of the current frame */
  const float* T_window[MGS_KF_MAX_WINDOW];            /* [4][4] per window keyframe */
  const uint8_t* visibility[MGS_KF_MAX_WINDOW];        /* [N] per window keyframe: occ-aware visibility */
  int64_t visibility_len[MGS_KF_MAX_WINDOW];           /* element count of each row: must equal N */
  void* scratch;                   /* mgs_keyframe_scratch_bytes(N, H*W, W) bytes; zero-filled once before the first
                                      call (every call leaves it as it found it) */
  void* result;                    /* device mgs_keyframe_result */
} mgs_keyframe_args;

typedef struct mgs_keyframe_result {
  int32_t create_kf;               /* the run loop's decision */
  int32_t removed;                 /* window position of add_to_window's removed frame, -1 (only if create_kf) */
  int32_t reset;                   /* monocular && !initialized && removed >= 0 */
  int32_t n_valid;                 /* valid depth pixels */
  int32_t removed_cutoff;          /* position dropped by the kf_cutoff rule (the last one at or below it), -1 */
  int32_t removed_evict;           /* position evicted by the inverse-distance score, -1 */
  int32_t n_cur;                   /* |cur| */
  int32_t flags;                   /* bit 0 dist_check, bit 1 dist_check2, bit 2 is_keyframe() */
  float median_depth;              /* NaN when n_valid == 0 */
  float dist;                      /* |t(T_cur T_last^-1)| */
  float overlap;                   /* |cur & row_0| / |cur | row_0| */
  int32_t window_len;
  float ss_ratio[MGS_KF_MAX_WINDOW];   /* |cur & row_w| / min(|cur|, |row_w|) */
  int32_t n_row[MGS_KF_MAX_WINDOW];    /* |row_w| */
  int32_t n_inter[MGS_KF_MAX_WINDOW];  /* |cur & row_w| */
  double score[MGS_KF_MAX_WINDOW];     /* eviction score by window position; -1 where not a candidate */
} mgs_keyframe_result;

/* 0 for a bad size.  num_pixels = H * W, window_len = W. */
uint64_t mgs_keyframe_scratch_bytes(int32_t num_gaussians, int32_t num_pixels, int32_t window_len);
/* Every argument is checked before anything is launched: a null pointer, a non-positive size or a row whose length is
 * not N gives MGS_ERR_BAD_ARGUMENT, window_len > MGS_KF_MAX_WINDOW MGS_ERR_UNSUPPORTED. */
int32_t mgs_keyframe_decide(const mgs_keyframe_args* args, void* stream);

/* ---- keyframe seeding ("Keyframe seeding on the device") ----------------------------------------------
 * From a tracked frame to the rows of its new Gaussians: the reference frontend's depth prior (add_new_keyframe,
 * utils/slam_frontend.py:183-234), the adaptive point size (np.median of the prepared depth map,
 * gaussian_model.py:143), a random K-subset of the valid pixels, their back-projection and colour
 * (create_pcd_from_image_and_depth :137-205) and the k-nn scale, stream-ordered, with ONE host read (the record, which
 * carries the row count the k-nn launcher and the caller's append need).
 *   mode 0  monocular, rendered depth: valid = depth > 0 && opacity > 0.95 && valid_rgb; med = lower median of the
 *           valid depths (torch.median's element); std = their unbiased standard deviation (fp64 sums over a fixed
 *           tree, rounded once); bad = d > med + std || d < med - std || !valid; d = bad ? med : d;
 *           d += noise * (bad ? 0.5 std : 0.2 std).  Fewer than two valid pixels: d = 2 everywhere.
 *   mode 1  monocular, first keyframe / reset: d = 2 + 0.3 noise.        mode 2  d = depth (the sensor's).
 * Then d = 0 where d is not finite and, in modes 0 and 2, where !valid_rgb (valid_rgb = (r + g) + b >
 * rgb_boundary_threshold; the reference's first-keyframe branch does not apply that mask).
 * point_size = adaptive_pointsize ? min(0.05, point_size * median_all) : point_size, median_all = NumPy's median of
 * all H*W values of d (zeros included; the mean of the two middle order statistics when H*W is even).
 * n = #{0 < d <= depth_trunc}, K = floor(n / downsample); every such pixel has a 32-bit key (keys[i], or drawn) and
 * the K smallest (key, pixel index) pairs are kept, in ascending pixel order.  Row p of the outputs, pixel (u, v),
 * z = d: xyz = R^T (((u - cx) z / fx, (v - cy) z / fy, z) - t); features_dc = RGB2SH(floor(clamp((|a| + eps) image
 * + b, 0, 1) * 255) / 255); rots = (1, 0, 0, 0); opacity_logit = 0; log_scales = log(sqrt(max(dist2, 1e-7) *
 * point_size)), dist2 = mgs_knn_dist2 of xyz[0:K].
 * noise == NULL / keys == NULL: the values are drawn from Philox-4x32-10 keyed by `seed` with the counter
 * (pixel index, 0, stream id, 0), stream 0 = noise (Box-Muller of the first two words), stream 1 = keys (first word).
 * No float atomics: two calls with the same inputs give bit-identical outputs. */
typedef struct mgs_keyframe_seed_result {
  int32_t num_points;              /* K: rows written */
  int32_t n_valid;                 /* mode 0: pixels behind median_depth / std_depth; otherwise 0 */
  int32_t n_outliers;              /* mode 0: pixels whose depth was replaced by the median; otherwise 0 */
  int32_t n_depth;                 /* n = #{0 < d <= depth_trunc} */
  float median_depth, std_depth;   /* mode 0 (NaN with fewer than 1 / 2 valid pixels); otherwise NaN */
  float median_all;                /* np.median of the prepared depth map */
  float point_size;                /* the value behind log_scales */
} mgs_keyframe_seed_result;

typedef struct mgs_keyframe_seed_args {
  int32_t width, height;
  int32_t row_capacity;            /* rows of every output; at least floor(width * height / downsample) */
  int32_t mode;                    /* 0, 1, 2 (above) */
  int32_t adaptive_pointsize, isotropic;   /* isotropic: log_scales is [P,1], else [P,3] (the value repeated) */
  float fx, fy, cx, cy;
  float rgb_boundary_threshold;
  float downsample;                /* >= 1 (the reference keeps 1 / downsample of the points) */
  float depth_trunc;               /* 100 in the reference */
  float exposure_eps;
  double point_size;
  uint64_t seed;
  const float* image;              /* [3][H][W] */
  const float* depth;              /* [H*W]; mode 0: rendered, mode 2: sensor; mode 1: unused (may be NULL) */
  const float* opacity;            /* [H*W]; mode 0 only */
  const float* T;                  /* device [4][4] row-major world-to-camera */
  const float* exposure_a;         /* device scalars */
  const float* exposure_b;
  const float* noise;              /* [H*W] replay of the normal draws, or NULL */
  const uint32_t* keys;            /* [H*W] replay of the sampling keys, or NULL */
  float* xyz;                      /* [P][3] */
  float* features_dc;              /* [P][3] */
  float* log_scales;               /* [P][1 or 3] */
  float* rots;                     /* [P][4] */
  float* opacity_logit;            /* [P][1] */
  int32_t* pixel_index;            /* [P] flat index of each row's pixel (ascending), or NULL */
  float* depth_out;                /* [H*W] the prepared depth map, or NULL */
  void* scratch;                   /* mgs_keyframe_seed_scratch_bytes(H*W, row_capacity) bytes, 16-byte aligned */
  void* result;                    /* device mgs_keyframe_seed_result */
  mgs_keyframe_seed_result* result_host;   /* host copy of the record, valid on return */
} mgs_keyframe_seed_args;

/* 0 for non-positive sizes. */
uint64_t mgs_keyframe_seed_scratch_bytes(int32_t num_pixels, int32_t row_capacity);
/* Every argument is checked before anything is launched or written: a null pointer (depth in modes 0 / 2, opacity in
 * mode 0 and every other pointer not marked optional), a non-positive size, downsample < 1 (or NaN), an unknown mode,
 * a scratch address that is not 16-byte aligned or row_capacity < floor(width * height / downsample) give
 * MGS_ERR_BAD_ARGUMENT.  Synchronises `stream` once. */
int32_t mgs_keyframe_seed(const mgs_keyframe_seed_args* args, void* stream);

/* ---- frame preparation on the device (frame_prepare.hip) ---------------------------------
 * What the reference does to EVERY incoming frame before tracking: the dataset's conversion (utils/dataset.py:269-276)
 * and Camera.compute_grad_mask (utils/camera_utils.py:110-147, stencils utils/slam_utils.py:7-41), stream-ordered, with
 * no host read and no synchronisation.
 *   ingest     uint8 [H][W][3] image: value = (float)(k / 255.0) (a double quotient rounded once, NumPy's);
 *              uint16 [H][W] depth: value = (float)(d / depth_scale), likewise a double quotient.
 *   sum, grey  s = (r + g) + b (two roundings, in this order); grey = s / 3.
 *   masks      rgb_pixel_mask_mapping = s > rgb_boundary_threshold;  rgb_pixel_mask = rgb_pixel_mask_mapping * grad_mask.
 *   gradient   3x3 cross-correlation (not flipped) over the reflect-padded grey (index -1 -> 1, H -> H - 2), times
 *              1 / 32: grad_v with [[3,10,3],[0,0,0],[-3,-10,-3]], grad_h with [[3,0,-3],[10,0,-10],[3,0,-3]].
 *              A pixel is valid when all nine padded neighbours have |grey| > 0.01; otherwise both gradients are 0.
 *              intensity I = sqrt(grad_v^2 + grad_h^2).
 *   global     m = the lower median of all H*W intensities (rank (H*W - 1) / 2, torch.median's element; a three-level
 *              radix select, no sort); grad_mask = I > m * edge_threshold (the product rounded to fp32).
 *   patch      (the reference's Replica branch) 32x32 patches, stride 32, anchored top-left, floor(H/32) x floor(W/32)
 *              of them; m_p = the element of rank 511 of a patch's 1024 intensities; grad_mask = I > m_p *
 *              edge_threshold inside the patches and 0 on every pixel that no whole patch covers.
 * Histogram counting is integer: two calls with the same inputs give bit-identical outputs.  NaN / Inf in the image:
 * unspecified (no out-of-bounds access; the masks and medians are then whatever the comparisons give). */
#define MGS_FRAME_IMAGE_F32_CHW 0
#define MGS_FRAME_IMAGE_U8_HWC 1
#define MGS_FRAME_DEPTH_NONE 0
#define MGS_FRAME_DEPTH_F32 1
#define MGS_FRAME_DEPTH_U16 2
#define MGS_FRAME_MODE_GLOBAL 0
#define MGS_FRAME_MODE_PATCH 1
#define MGS_FRAME_PATCH_SIZE 32

typedef struct mgs_frame_prepare_args {
  int32_t width, height;           /* both >= 2 (reflect padding); patch mode: both >= 32 */
  int32_t mode;                    /* MGS_FRAME_MODE_* */
  int32_t image_format;            /* MGS_FRAME_IMAGE_* */
  int32_t depth_format;            /* MGS_FRAME_DEPTH_* */
  float edge_threshold;
  float rgb_boundary_threshold;
  int32_t reserved0;
  double depth_scale;              /* uint16 depth only; > 0 */
  const void* image_in;            /* float [3][H][W] or uint8 [H][W][3] */
  const void* depth_in;            /* float [H][W] or uint16 [H][W]; NULL without depth */
  float* image;                    /* [3][H][W] the float image; required for uint8 input, for float input optional
                                      (a copy; NULL or image_in itself: nothing is written) */
  float* gt_depth;                 /* [1][H][W]; required for uint16 input, for float input optional likewise */
  float* grad_mask;                /* [1][H][W] 0 / 1 */
  float* rgb_pixel_mask;           /* [1][H][W] 0 / 1 */
  float* rgb_pixel_mask_mapping;   /* [1][H][W] 0 / 1 */
  float* median_out;               /* device; global: 1 float, patch: floor(H/32) * floor(W/32), row-major; or NULL */
  float* intensity_out;            /* [H][W] the gradient intensity, or NULL */
  void* scratch;                   /* mgs_frame_prepare_scratch_bytes(H, W) bytes, 16-byte aligned; the call zeroes
                                      what it counts in itself: no memset is asked of the caller */
} mgs_frame_prepare_args;

/* sizeof(mgs_frame_prepare_args), for a binding to verify its mirror.  The list behind mgs_struct_size() ends at index
 * 25 (bindings and tests rely on -1 from 26 on), so this struct answers for itself. */
int32_t mgs_frame_prepare_args_size(void);
/* 0 for sizes the call refuses. */
uint64_t mgs_frame_prepare_scratch_bytes(int32_t H, int32_t W);
/* Every argument is checked before anything is launched or written: a null required pointer, H or W < 2 (< 32 in patch
 * mode), an unknown mode / format, depth_scale <= 0 (or NaN) with uint16 depth, a scratch address that is not 16-byte
 * aligned give MGS_ERR_BAD_ARGUMENT; an image beyond 2^31 - 1 pixels or 65 535 tiles a side MGS_ERR_UNSUPPORTED.
 * Global mode: one memset node and four launches; patch mode: one launch.  No host read, no synchronisation. */
int32_t mgs_frame_prepare(const mgs_frame_prepare_args* args, void* stream);

/* ---- undistortion / rectification fused into frame preparation (DESIGN.md "Undistort and rectify") ---------------
 * What the reference's dataset does to a frame before anything else sees it when Calibration.distorted is set:
 * cv2.remap(image, map1x, map1y, INTER_LINEAR) with the maps of cv2.initUndistortRectifyMap (utils/dataset.py:226-244,
 * 264-265).  Here the gather is fused into the tile load of mgs_frame_prepare: no launch and no pass over the image is
 * added.  Parity with cv2 is UNPINNED (no cv2 to produce a fixture with); the contract below is this library's own, and
 * kernel and mirror (frame_prepare.remap_build_numpy / remap_torch) agree bit for bit, so the order of operations is
 * part of it.
 *
 * Map build, once per calibration; all arithmetic fp64, no contraction, in this order.  ir[9]: the row-major inverse of
 * new_K * R, computed by the caller in double (nothing is inverted on the device); fx, fy, cx, cy: the source
 * (distorted) camera; dist = (k1, k2, p1, p2, k3), OpenCV's order.  For destination pixel (u, v):
 *   X = (ir0*u + ir1*v) + ir2;  Y = (ir3*u + ir4*v) + ir5;  Wd = (ir6*u + ir7*v) + ir8
 *   x = X / Wd;  y = Y / Wd
 *   x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  txy = (2*x)*y
 *   kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *   xd = (x*kr + p1*txy) + p2*(r2 + 2*x2)
 *   yd = (y*kr + p1*(r2 + 2*y2)) + p2*txy
 *   mx = float32(fx*xd + cx);  my = float32(fy*yd + cy)
 *   ix = rint_half_even(double(mx) * 32) clamped to [-2^30, 2^30];  iy likewise
 * mx or my not finite: ix = iy = -2^30 (every tap falls outside the image).  The map is int32 [H][W][2] holding
 * (ix, iy): the source position in 1/32-pixel fixed point.
 *
 * Remap, for each destination pixel and each reflect-padded halo pixel (the halo of destination (y, x) reads the map at
 * (reflect(y), reflect(x)): padding happens on the undistorted image).  sx = ix >> 5, sy = iy >> 5 (arithmetic shifts);
 * ax = ix & 31, ay = iy & 31; the taps are (sy,sx), (sy,sx+1), (sy+1,sx), (sy+1,sx+1); a tap outside [0,H) x [0,W)
 * reads 0 in every channel, decided per tap (a constant border).  Integer weights w00 = (32-ax)(32-ay),
 * w01 = ax(32-ay), w10 = (32-ax)ay, w11 = ax*ay (they sum to 1024).
 *   uint8 image  k = (w00*v00 + w01*v01 + w10*v10 + w11*v11 + 512) >> 10, then float32(k / 255.0).
 *   float image  (f00*v00 + f01*v01) + (f10*v10 + f11*v11) with f = float(w) / 1024 (exact); every product and sum
 *                rounded on its own (no fma).
 * Everything downstream (sum, grey, gradient, medians, masks) is mgs_frame_prepare's contract on the remapped image.
 *
 * Depth.  MGS_FRAME_REMAP_DEPTH_NONE: gt_depth exactly as mgs_frame_prepare leaves it (the reference remaps the image
 * only).  MGS_FRAME_REMAP_DEPTH_NEAREST: gt_depth = the tap ((iy+16) >> 5, (ix+16) >> 5) of the converted source depth,
 * 0 outside - for callers who want depth and image registered (not the reference's behaviour). */
#define MGS_FRAME_REMAP_DEPTH_NONE 0
#define MGS_FRAME_REMAP_DEPTH_NEAREST 1

typedef struct mgs_remap_build_args {
  int32_t width, height;           /* the destination image; both >= 1 */
  double ir[9];                    /* row-major inverse of new_K * R */
  double fx, fy, cx, cy;           /* the source (distorted) camera */
  double dist[5];                  /* k1, k2, p1, p2, k3 */
  int32_t* map_q5;                 /* device int32 [H][W][2], 8-byte aligned: (ix, iy) per destination pixel */
} mgs_remap_build_args;

typedef struct mgs_frame_remap_args {
  const int32_t* map_q5;           /* device int32 [H][W][2] of the frame's size, 8-byte aligned */
  int32_t depth_mode;              /* MGS_FRAME_REMAP_DEPTH_* */
  int32_t reserved0;
} mgs_frame_remap_args;

int32_t mgs_remap_build_args_size(void);
int32_t mgs_frame_remap_args_size(void);
/* One launch (k_fp_remap_build, a thread per destination pixel).  A null struct or map, a map that is not 8-byte
 * aligned, a side < 1: MGS_ERR_BAD_ARGUMENT; more than 2^31 - 1 pixels: MGS_ERR_UNSUPPORTED. */
int32_t mgs_remap_build(const mgs_remap_build_args* args, void* stream);
/* mgs_frame_prepare on the remapped image: the same stream operations (global mode: one memset node and four launches,
 * patch mode: one launch).  Everything mgs_frame_prepare checks, and MGS_ERR_BAD_ARGUMENT for: a null remap struct or
 * map; a map that is not 8-byte aligned; an unknown depth_mode; a null `image`; image == image_in (either format: a
 * gather cannot run in place); with MGS_FRAME_REMAP_DEPTH_NEAREST no depth, a null gt_depth or gt_depth == depth_in.
 * Checked before anything is launched or written. */
int32_t mgs_frame_prepare_remapped(const mgs_frame_prepare_args* args, const mgs_frame_remap_args* remap, void* stream);

/* ---- stereo depth (stereo_depth.hip; DESIGN.md "Stereo depth on the device") ---------------------------------------
 * What the reference's StereoDataset.__getitem__ does to every frame on the host (utils/dataset.py:367-395): rectify
 * both images, cv2.StereoSGBM_create(minDisparity=0, numDisparities=64, blockSize=20) with setUniquenessRatio(40),
 * depth = bf / disparity.  The algorithm restates OpenCV's single-pass MODE_SGBM from knowledge of it; parity with cv2
 * is UNPINNED (no cv2 to produce a fixture with).  The contract is this library's own: every step is integer arithmetic
 * and kernels and mirror (stereo_depth.stereo_sgbm_numpy) agree bit for bit.
 *
 * Grey.  The rectified grey uint8 images L, R [H][W] come from the inputs by image_format:
 *   U8_GREY  the byte itself;  U8_HWC (RGB order)  (4899*r + 9617*g + 1868*b + 8192) >> 14 (OpenCV's fixed point);
 *   F32_CHW  each channel to k = clamp(rint_half_even(v * 255 in fp32), 0, 255) (NaN: 0), then as U8_HWC.
 * With a map (map_left / map_right, the int32 [H][W][2] 1/32-pixel maps of mgs_remap_build) every channel is first
 * gathered exactly as "Remap" above states it (uint8: the rounded integer blend, a byte again; float: the fp32 blend),
 * with a constant 0 border, and then reduced to grey.  image (optional) = float32(L / 255.0) in all three channels.
 *
 * Constants: D = 64 disparities d = 0..63, minDisparity 0; half block r = block_size / 2 (21 x 21 at 20); P1 = 2,
 * P2 = 5; ftzero = 15; disp12MaxDiff = 0; valid columns x in [D, W).
 *   prefilter   g = clip(2*(I[y,x+1]-I[y,x-1]) + (I[y-1,x+1]-I[y-1,x-1]) + (I[y+1,x+1]-I[y+1,x-1]), -15, 15) + 15, rows
 *               clamped at the border, g = 15 in the first and the last column.
 *   pixel cost  Birchfield-Tomasi on the two channels g and I.  For u at x (neighbours clamped): ul = (u + u[x-1]) / 2,
 *               ur = (u + u[x+1]) / 2, u0 = min(u, ul, ur), u1 = max(u, ul, ur); the same for v = R[x-d];
 *               c = min(max(0, u - v1, v0 - u), max(0, v - u1, u0 - v)) >> 2; the cost is c(g) + c(I), at most 70.
 *   block cost  C(x,y,d) = the pixel cost summed over |dx| <= r, |dy| <= r with y clamped to [0, H-1] and x to [D, W-1].
 *   paths       five, the predecessor q of p = (x,y) being (x-1,y), (x+1,y), (x-1,y-1), (x,y-1), (x+1,y-1):
 *               L(p,d) = C(p,d) + min(L(q,d), L(q,d-1) + P1, L(q,d+1) + P1, m_q + P2) - m_q, m_q = min_d L(q,d), d-1 / d+1
 *               outside 0..63 left out; q outside the valid region: L(p,.) = C(p,.).  S = the sum of the five.
 *   selection   b = argmin_d S (the smallest d on ties).  Not unique - invalid - if some d with |d - b| > 1 has
 *               S[d] * (100 - uniqueness_ratio) < S[b] * 100.  0 < b < 63: den = max(S[b-1] + S[b+1] - 2*S[b], 1),
 *               disp16 = 16*b + ((S[b-1] - S[b+1]) * 16 + den) / (2*den) (C division); else disp16 = 16*b.  Invalid pixels
 *               and all of x < D hold -16.
 *   left-right  every unique pixel votes (S[b], b) into x2 = x - b; a column keeps the smallest S, on ties the smallest
 *               b.  A valid pixel with d1 = disp16 is invalidated if both candidates d1 >> 4 and (d1 + 15) >> 4
 *               disagree: a candidate c disagrees when x - c is inside the row, holds a vote, and that vote's b != c.
 *   depth       disp = disp16 / 16.0 (double); disp == 0 -> 1e10; depth = float32(bf / disp); depth < 0 -> 0.
 * Two calls with the same inputs give identical bits (integer sums only). */
#define MGS_STEREO_IMAGE_U8_GREY 0
#define MGS_STEREO_IMAGE_U8_HWC 1
#define MGS_STEREO_IMAGE_F32_CHW 2
#define MGS_STEREO_DISPARITIES 64

typedef struct mgs_stereo_depth_args {
  int32_t width, height;           /* width > 64 */
  int32_t image_format;            /* MGS_STEREO_IMAGE_*, of both inputs */
  int32_t num_disparities;         /* 64 (anything else: MGS_ERR_UNSUPPORTED) */
  int32_t block_size;              /* the reference's 20; half block block_size / 2 <= 14 */
  int32_t uniqueness_ratio;        /* 0..100; the reference's 40 */
  double bf;                       /* baseline * fx; the reference's 47.90639384423901 */
  const void* left_in;             /* uint8 [H][W], uint8 [H][W][3] or float [3][H][W] */
  const void* right_in;
  const int32_t* map_left;         /* device int32 [H][W][2], 8-byte aligned, or NULL: the input is rectified already */
  const int32_t* map_right;
  float* depth;                    /* [H][W] */
  int16_t* disp16;                 /* [H][W], or NULL */
  float* image;                    /* [3][H][W] the rectified left grey / 255, or NULL */
  void* scratch;                   /* mgs_stereo_scratch_bytes(H, W) bytes, 16-byte aligned; nothing is asked of the
                                      caller */
} mgs_stereo_depth_args;

/* sizeof(mgs_stereo_depth_args), for a binding to verify its mirror (as mgs_frame_prepare_args_size). */
int32_t mgs_stereo_depth_args_size(void);
/* 0 for sizes the call refuses (W <= 64, a side beyond 16 384). */
uint64_t mgs_stereo_scratch_bytes(int32_t H, int32_t W);
/* Every argument is checked before anything is launched or written: a null struct, input, depth or scratch, W <= 64,
 * an unknown format, block_size < 1, a uniqueness_ratio outside 0..100, a misaligned scratch or map give
 * MGS_ERR_BAD_ARGUMENT; num_disparities != 64, block_size / 2 > 14 or a side beyond 16 384 MGS_ERR_UNSUPPORTED.
 * Seven launches and one memset node on `stream`.  No host read, no synchronisation. */
int32_t mgs_stereo_depth(const mgs_stereo_depth_args* args, void* stream);

/* ---- map maintenance on the device ---------------------------------- */

#define MGS_ADAM_MAX_GROUPS 8
#define MGS_GATHER_MAX_TENSORS 24

/* torch.optim.Adam step (betas / eps / bias correction as PyTorch, no weight decay, no
 * amsgrad) over all parameter groups of GaussianModel.training_setup
 * (gaussian_splatting/scene/gaussian_model.py:252-285; stepped at utils/slam_backend.py:142,
 * 322,365) in one launch. */
typedef struct mgs_adam_group {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  float lr;
  int32_t step;          /* 1-based step count of THIS tensor (PyTorch keeps it per parameter:
                            a tensor without a gradient does not advance) */
} mgs_adam_group;

/* betas / eps are doubles so that 1 - beta rounds to fp32 exactly as in PyTorch (which
 * evaluates it in Python floats): with a float beta2 = 0.999f, 1 - beta2 is off by 1.3e-5. */
int32_t mgs_adam_step_multi(const mgs_adam_group* groups, int32_t num_groups, double beta1,
                            double beta2, double eps, void* stream);

/* Keyframe-parallel mapping: one launch packs this rank's parameter gradients
 * and the densification statistics of its view (gaussian_model.py:693-697:
 * ||means2D.grad[:, :2]|| where radii > 0, and the visibility count) into the flat buffer that
 * is all-reduced over RCCL: flat = [grad_0 | ... | grad_{k-1} | grad-norm stat [N] | visible [N]].
 * radii is copied to radii_out (all-reduced with max). */
int32_t mgs_pack_mapping_grads(const float* const* grads, const int64_t* numels, int32_t num_grads,
                               const float* means2D_grad, const int32_t* radii,
                               int64_t num_gaussians, float* flat, int32_t* radii_out, void* stream);

/* Rebuild plan of GaussianModel.densify_and_prune (gaussian_model.py:674-691 =
 * densify_and_clone :636-672, densify_and_split :598-634, prune_points :540-556) or, with
 * prune_mask != NULL, of prune_points(mask) alone.  Rows of the rebuilt arrays, in the
 * reference's order: surviving originals, surviving clones, first split children, second split
 * children (each group in index order - stable).
 *   mgs_map_plan_count: per-Gaussian decisions -> flags, totals[0..3] = surviving originals,
 *                       clones, split parents (so rows = t0 + t1 + 2 * t2) and t3 = ALL Gaussians
 *                       selected for splitting (the reference draws 2 * t3 random offsets at :608-609
 *                       before the final prune removes some children);
 *   mgs_map_plan_emit:  src_index[row] = parent | kind << 30 (kind 0 original, 1 clone,
 *                       2 / 3 first / second child), rows entries; noise_row[k] = row of the
 *                       [2 * t3, 3] noise tensor used by the k-th child row, 2 * t2 entries.
 * The caller reads totals between the two calls to allocate (one host sync per rebuild). */
typedef struct mgs_map_plan_args {
  int32_t n;
  /* densify_and_prune inputs (ignored when prune_mask is given) */
  const float* grad_accum;      /* [n] xyz_gradient_accum */
  const float* denom;           /* [n] */
  const float* log_scales;      /* [n,3] _scaling */
  const float* opacity_logit;   /* [n]   _opacity */
  float grad_threshold;         /* max_grad */
  float dense_extent;           /* percent_dense * extent */
  float min_opacity;
  float big_extent;             /* 0.1 * extent when max_screen_size is set, else <= 0 */
  const uint8_t* prune_mask;    /* [n] 1 = remove, or NULL */
  /* scratch / outputs */
  uint8_t* flags;               /* [n] */
  int32_t* block_counts;        /* [4 * mgs_map_plan_blocks(n)] */
  int32_t* totals;              /* [4] */
  uint32_t* src_index;          /* [rows], mgs_map_plan_emit only */
  int32_t* noise_row;           /* [max(1, 2 * totals[2])], mgs_map_plan_emit only */
} mgs_map_plan_args;

int32_t mgs_map_plan_blocks(int32_t n);
int32_t mgs_map_plan_count(const mgs_map_plan_args* args, void* stream);
int32_t mgs_map_plan_emit(const mgs_map_plan_args* args, void* stream);

/* Rebuild per-Gaussian tensors (32-bit elements, `width` per row) from a plan in one launch:
 * dst[row, :] = f(src[parent(row), :]). */
enum {
  MGS_GATHER_COPY = 0,           /* every row copies its parent (features, opacity, rotation, ids) */
  MGS_GATHER_ZERO_NEW = 1,       /* originals copy, clones / children get 0 (Adam moments, :560-577) */
  MGS_GATHER_SPLIT_SCALING = 2,  /* children: log(exp(s) / 1.6)  (:615-617), float */
  MGS_GATHER_SPLIT_XYZ = 3       /* children: xyz + R(q) (noise * exp(s))  (:609-614), float, width 3 */
};

typedef struct mgs_gather_tensor {
  const void* src;
  void* dst;
  int32_t width;
  int32_t mode;
} mgs_gather_tensor;

typedef struct mgs_map_gather_args {
  mgs_gather_tensor tensors[MGS_GATHER_MAX_TENSORS];
  int32_t num_tensors;
  int64_t rows;                 /* rows of the rebuilt arrays */
  int32_t num_children;         /* totals[2]; the last 2 * num_children rows are split children */
  const uint32_t* src_index;
  const float* rotations;       /* parents' _rotation [n,4]   (MGS_GATHER_SPLIT_XYZ) */
  const float* log_scales;      /* parents' _scaling [n,3]    (MGS_GATHER_SPLIT_XYZ) */
  const float* noise;           /* [2 * totals[3], 3] unit normals */
  const int32_t* noise_row;     /* from mgs_map_plan_emit */
} mgs_map_gather_args;

int32_t mgs_map_gather(const mgs_map_gather_args* args, void* stream);

/* ---- native mapping iteration (row a13: utils/slam_backend.py:171-332) -------------------- */

/* GaussianModel's activations for one mapping iteration (gaussian_model.py:54-62,77-102), one
 * launch: scales = exp(_scaling) (an isotropic [N,1] model is broadcast to 3 axes as the
 * renderer does, gaussian_renderer/__init__.py:92-95), rotations = normalize(_rotation),
 * opacities = sigmoid(_opacity), shs = cat(_features_dc, _features_rest).  `shs` may be NULL
 * when K == 1: features_dc is then used in place. */
typedef struct mgs_map_activate_args {
  int32_t num_gaussians;
  int32_t scale_dims;            /* 3 or 1 */
  int32_t sh_coeffs;             /* K */
  const float* log_scales;       /* [N,scale_dims] */
  const float* raw_rotations;    /* [N,4] */
  const float* opacity_logits;   /* [N] */
  const float* features_dc;      /* [N,1,3] */
  const float* features_rest;    /* [N,K-1,3] or NULL */
  float* scales;                 /* out [N,3] */
  float* rotations;              /* out [N,4] */
  float* opacities;              /* out [N] */
  float* shs;                    /* out [N,K,3] or NULL (K == 1) */
} mgs_map_activate_args;

int32_t mgs_map_activate(const mgs_map_activate_args* args, void* stream);

/* One view of one mapping iteration as a fixed launch sequence with no host round trip
 * (the body of the loops at utils/slam_backend.py:183-242 plus this view's share of :247-332):
 *   camera matrices from T -> rasteriser forward at the caller's fixed pair capacity ->
 *   mapping objective (utils/slam_utils.py:224-253) value + gradients in one pass ->
 *   rasteriser backward in mapping mode (mgs_map_accum_args: gradients chained through the
 *   activations and ACCUMULATED over the views, densification statistics, occ-aware visibility)
 *   -> Adam on this view's (cam_rot_delta, cam_trans_delta, exposure_a, exposure_b) + update_pose
 *   (mgs_pose_adam_args; the keyframe optimiser of :452-489 is per view, so its step commutes
 *   with the other views).
 * forward_only != 0 stops after the forward and only writes accum.visibility (the prune pass of
 * :259-290 consumes nothing else).  loss.image / depth / grad_* / partial and adam.grad_* /
 * *_partials are filled in by the call; loss.partial must hold
 * mgs_mapping_loss_partial_count(HW) floats. */
typedef struct mgs_mapping_view_args {
  mgs_forward_args fwd;
  void* bwd;                     /* bwd_bytes of backward scratch */
  float* grad_image;             /* [3,H,W] scratch */
  float* grad_depth;             /* [1,H,W] scratch, or NULL when loss.w_depth == 0 */
  float* grad_tau;               /* [6] scratch */
  mgs_mapping_loss_args loss;
  mgs_pose_adam_args adam;
  mgs_map_accum_args accum;
  float* loss_view;              /* [1] out: this view's loss, or NULL */
  float* loss_accum;             /* [1] += this view's loss, or NULL */
  int32_t camera_matrices_valid;
  int32_t forward_only;
} mgs_mapping_view_args;

int32_t mgs_mapping_loss_partial_count(int64_t num_pixels);
/* Value and gradients of the mapping objective in one pass (upstream gradient 1 unless
 * grad_out is given): grad_image / grad_depth are written, `partial` receives the block sums
 * [4][*num_blocks_out] = colour residual, depth residual, d/da, d/db for a consumer that sums
 * them (mgs_pose_adam_step: loss_partials / exposure_partials).  With partial_ticket_ready != 0
 * (the int at partial[4 n] zero when enqueued; restored by the call) the workgroup that finishes
 * last also writes *loss, *grad_a, *grad_b (each optional). */
int32_t mgs_mapping_loss_fused(const mgs_mapping_loss_args* args, int32_t* num_blocks_out, void* stream);
int32_t mgs_mapping_view_iteration(const mgs_mapping_view_args* args, void* stream);

/* End of a mapping iteration (after the optional all-reduce of the flat buffer), one launch:
 *   xyz_gradient_accum += gradnorm_inc, denom += denom_inc, max_radii2D = max(max_radii2D, radii_max)
 * (slam_backend.py:292-299; max_radii2D is a float tensor in the reference), and optionally
 * GaussianModel.reset_opacity / reset_opacity_nonvisible (gaussian_model.py:364-377 +
 * replace_tensor_to_optimizer :470-483): opacity logit <- inverse_sigmoid(reset_value) for every
 * Gaussian (reset_mode 1) or for those NOT visible in any view of this iteration, i.e.
 * denom_inc == 0 (reset_mode 2, 3), and the opacity group's Adam moments zeroed (all of them,
 * as the reference does).  reset_mode 2 is the reference to the letter: gaussian_model.py:375 stores
 * the ACTIVATED opacity of a visible Gaussian as its new raw parameter, so its logit l becomes
 * sigmoid(l) (pinned by tests/golden/map_update_ref.npz, generated from the reference's own code);
 * reset_mode 3 leaves the visible Gaussians' logits untouched (what the code presumably meant). */
typedef struct mgs_map_finish_args {
  int32_t num_gaussians;
  const float* gradnorm_inc;     /* [N] or NULL (no statistics this iteration) */
  const float* denom_inc;        /* [N] (also the visibility source of reset_mode 2) */
  const int32_t* radii_max;      /* [N] */
  float* xyz_gradient_accum;     /* [N] */
  float* denom;                  /* [N] */
  float* max_radii2D;            /* [N] */
  int32_t reset_mode;            /* 0 none, 1 reset_opacity, 2 reset_opacity_nonvisible (reference), 3 same, visible logits kept */
  float reset_value;             /* 0.01 / 0.4 */
  float* opacity_logits;         /* [N] (reset_mode != 0) */
  float* opacity_exp_avg;        /* [N] or NULL */
  float* opacity_exp_avg_sq;     /* [N] or NULL */
} mgs_map_finish_args;

int32_t mgs_map_finish_iteration(const mgs_map_finish_args* args, void* stream);

/* GaussianModel.extend_from_pcd (gaussian_model.py:210-245 -> cat_tensors_to_optimizer :525-557,
 * densification_postfix :559-593) in one launch: dst[t] = cat(old[t], new[t]) for up to
 * MGS_GATHER_MAX_TENSORS row-major 32-bit tensors; new == NULL appends zeros (Adam moments). */
typedef struct mgs_map_append_args {
  mgs_gather_tensor tensors[MGS_GATHER_MAX_TENSORS];   /* src = old rows, dst = rebuilt rows, mode unused */
  const void* new_rows[MGS_GATHER_MAX_TENSORS];        /* [rows_new, width] or NULL = zeros */
  int32_t num_tensors;
  int64_t rows_old, rows_new;
} mgs_map_append_args;

int32_t mgs_map_append(const mgs_map_append_args* args, void* stream);

/* ---- colour refinement (utils/slam_backend.py:335-368) ------------------------------------ */

/* Objective of BackEnd.color_refinement (slam_backend.py:355-358; loss_utils.py:21-22,63-101):
 *   l1 = mean |image - gt|,  ssim = mean S (11x11 Gaussian window, sigma 1.5, per channel, zero padding,
 *   C1 = 0.01^2, C2 = 0.03^2),  loss = w_l1 l1 + w_ssim (1 - ssim)
 * over [C,H,W] (means over C H W), value and - unless grad_image is NULL - grad_image = g d loss / d image in ONE
 * launch, g = *grad_out (NULL: 1).  `partial` holds mgs_ssim_loss_partial_count(C, H, W) floats; its last slot is
 * an int ticket that must be zero when the FIRST call on the buffer is enqueued (every call restores it), so calls
 * in stream order may share the buffer.  Deterministic: no float atomics. */
typedef struct mgs_ssim_loss_args {
  int32_t channels, height, width;
  float w_l1, w_ssim;            /* 1 - lambda_dssim, lambda_dssim */
  int32_t reserved0;
  const float* image;            /* [C,H,W] */
  const float* gt;               /* [C,H,W] */
  const float* grad_out;         /* [1] upstream gradient or NULL (1) */
  float* grad_image;             /* [C,H,W] out, or NULL: value only */
  float* partial;                /* scratch, see above */
  float* l1;                     /* [1] out, or NULL */
  float* ssim;                   /* [1] out, or NULL */
  float* loss;                   /* [1] out */
} mgs_ssim_loss_args;

/* Floats of mgs_ssim_loss_args.partial for a [C,H,W] image; -1 for a size the kernel is not built for. */
int32_t mgs_ssim_loss_partial_count(int32_t channels, int32_t height, int32_t width);
int32_t mgs_ssim_loss(const mgs_ssim_loss_args* args, void* stream);

/* One view of one colour-refinement iteration (the body of slam_backend.py:341-365 up to the optimiser step) as a
 * fixed launch sequence with no host round trip:
 *   camera matrices from T (skipped when camera_matrices_valid) -> rasteriser forward at the caller's fixed pair
 *   capacity -> mgs_ssim_loss(out_color, loss.gt) -> rasteriser backward in mapping mode (accum: gradients chained
 *   through the activations, OVERWRITTEN; no regulariser, no densification statistics, no visibility) ->
 *   max_radii2D = max(max_radii2D, radii) where radii > 0.
 * No exposure is applied and no pose or exposure step is taken.  The caller steps the Gaussians' optimiser.
 * loss.image / grad_image / grad_out / channels / height / width are filled in by the call; loss.gt, partial, loss
 * (and optionally l1 / ssim) and the weights come from the caller.  accum.accumulate / add_regulariser /
 * gradnorm_inc / denom_inc / radii_max / visibility are ignored (forced to 0 / NULL). */
typedef struct mgs_refine_view_args {
  mgs_forward_args fwd;
  void* bwd;                     /* bwd_bytes of backward scratch */
  float* grad_image;             /* [3,H,W] scratch */
  float* grad_tau;               /* [6] scratch */
  const float* T;                /* [4,4] world -> camera (the camera matrices are formed from it) */
  mgs_ssim_loss_args loss;
  mgs_map_accum_args accum;
  float* max_radii2D;            /* [N] float */
  int32_t camera_matrices_valid;
  int32_t reserved0;
} mgs_refine_view_args;

int32_t mgs_refine_view_iteration(const mgs_refine_view_args* args, void* stream);

/* ---- evaluation (utils/eval_utils.py:114-178; DESIGN.md: "Evaluation on the device") -------------------- */

/* One launch scores a rendered view against its ground truth and writes ONE record of a caller-owned device table;
 * nothing is read on the host.  With x = clamp(image, 0, 1), or x = clamp((|a| + eps) image + b, 0, 1) when
 * apply_exposure != 0 (a = *exposure_a, b = *exposure_b), and y the ground truth (a uint8 [H,W,3] image is converted as
 * the dataset does, / 255, while it is loaded), the record is MGS_EVAL_RECORD_DOUBLES doubles:
 *   [MGS_EVAL_SSE]        sum (x - y)^2 over the ELEMENTS (channel by channel) with y > 0     (eval_utils.py:150-152)
 *   [MGS_EVAL_SSE_ALL]    sum (x - y)^2 over all 3 H W elements                               (image_utils.py:19-21 as is)
 *   [MGS_EVAL_ABS]        sum |x - y| over all 3 H W elements
 *   [MGS_EVAL_SSIM]       sum S(x, y) over all 3 H W elements, S the SSIM map of mgs_ssim_loss (loss_utils.py:61-101)
 *   [MGS_EVAL_DEPTH_ABS]  sum |depth - gt_depth| over the pixels with gt_depth > 0 (0 without depth)
 *   [MGS_EVAL_N_MASK]     number of elements with y > 0
 *   [MGS_EVAL_N_DEPTH]    number of pixels with gt_depth > 0
 *   [MGS_EVAL_PAIRS]      *pair_count (the forward's pair count D of this view), 0 when pair_count is NULL
 * Every workgroup writes its seven fp32 partial sums in a fixed order and the workgroup that takes the last ticket adds
 * them in index order in double: no float atomics, two calls give the same bits.  `partial` holds
 * mgs_eval_score_partial_count(H, W) floats; its last slot is an int ticket that must be zero when the FIRST call on
 * the buffer is enqueued (every call restores it), so calls in stream order may share the buffer. */
#define MGS_EVAL_RECORD_DOUBLES 8
#define MGS_EVAL_SSE 0
#define MGS_EVAL_SSE_ALL 1
#define MGS_EVAL_ABS 2
#define MGS_EVAL_SSIM 3
#define MGS_EVAL_DEPTH_ABS 4
#define MGS_EVAL_N_MASK 5
#define MGS_EVAL_N_DEPTH 6
#define MGS_EVAL_PAIRS 7
#define MGS_EVAL_GT_F32_CHW 0
#define MGS_EVAL_GT_U8_HWC 1

typedef struct mgs_eval_score_args {
  int32_t height, width;
  int32_t gt_format;             /* MGS_EVAL_GT_F32_CHW: float [3,H,W]; MGS_EVAL_GT_U8_HWC: uint8 [H,W,3] */
  int32_t row, num_rows;         /* the record written, rows of `table`: 0 <= row < num_rows */
  int32_t apply_exposure;        /* != 0: exposure_a / exposure_b are read */
  float exposure_eps;
  int32_t reserved0;
  const float* image;            /* [3,H,W] the raw render */
  const void* gt;                /* see gt_format */
  const float* depth;            /* [H,W] rendered depth, or NULL */
  const float* gt_depth;         /* [H,W], or NULL (both or neither) */
  const float* exposure_a;       /* [1] */
  const float* exposure_b;       /* [1] */
  const int32_t* pair_count;     /* [1] or NULL */
  float* partial;                /* scratch, see above */
  double* table;                 /* [num_rows, MGS_EVAL_RECORD_DOUBLES] */
} mgs_eval_score_args;

/* Floats of mgs_eval_score_args.partial for an [3,H,W] image; -1 for a size the kernel is not built for. */
int32_t mgs_eval_score_partial_count(int32_t height, int32_t width);
int32_t mgs_eval_score(const mgs_eval_score_args* args, void* stream);

/* One scored view as a fixed launch sequence with no host round trip:
 *   camera matrices from T (skipped when camera_matrices_valid) -> rasteriser forward at the caller's fixed pair
 *   capacity -> mgs_eval_score(out_color, and out_depth when score.gt_depth is given) into record score.row.
 * score.image / depth / pair_count are filled in by the call (pair_count: the forward's counter in `geom`, so a record
 * whose MGS_EVAL_PAIRS exceeds fwd.shape.pair_capacity was rendered incompletely and has to be scored again);
 * score.height / width must equal fwd.shape's. */
typedef struct mgs_eval_view_args {
  mgs_forward_args fwd;
  const float* T;                /* [4,4] world -> camera */
  mgs_eval_score_args score;
  int32_t camera_matrices_valid;
  int32_t reserved0;
} mgs_eval_view_args;

int32_t mgs_eval_view(const mgs_eval_view_args* args, void* stream);
/* sizeof() of the two structs above, for a binding to verify its mirrors (as mgs_frame_prepare_args_size). */
int32_t mgs_eval_score_args_size(void);
int32_t mgs_eval_view_args_size(void);

/* ---- dense Gauss-Newton tracking iteration ("Dense Gauss-Newton tracking") -----------------
 * The second-order iteration WITHOUT the sketch: every pixel p is a row of its own,
 *   f_p = s * sum_c Huber(r_pc),  s = stack_dim * sketch_dim / (H*W),  J_p = d f_p / d [rho; theta; a; b]
 * (r_pc, the mask, the opacity, Huber, the depth row and ApplyExposure's hand-written backward exactly as in
 * mgs_sketch_residual[_rgbd] with every weight +1), and the step solves (H + lambda I) x = -g with
 *   H = sum_p J_p^T J_p,  g = sum_p J_p^T f_p   over ALL H*W pixels.
 * stack_dim / sketch_dim only enter through s, which makes H the expectation of the sketched SJ^T SJ, so that the
 * lm block (lambdas, factors, thresholds, lm_state, best) means what it means in mgs_tracking_iteration_second_order.
 * Launch sequence: camera matrices from T (unless base.camera_matrices_valid) -> forward -> exact residual pass beside
 * the per-splat Jacobian preparation (three planes f, df/da, df/db and per-workgroup L1 partials into `scratch`) ->
 * Jacobian-only backward in sketch mode -> normal equations (44 fp32 partial sums per workgroup) -> fp64 sum in index
 * order, Cholesky, lambda rule, best record, step.  No atomics and no memset anywhere: two calls on the same inputs
 * give the same bits.  `scratch` holds mgs_gauss_newton_scratch_bytes(&base.fwd.shape) bytes and needs no initial state.
 * normal_out (or NULL) receives the 44 sums of this iteration as floats: the upper triangle of H row-major
 * (H00 .. H07, H11 .. H17, ..., H77; WITHOUT lambda), then g[8] (the sign of sum J f: the solve negates it). */
typedef struct mgs_tracking_gn_args {
  mgs_tracking_iter_args base;   /* as for mgs_tracking_iteration_second_order */
  int32_t stack_dim, sketch_dim; /* of the configured sketch: only their product enters (s above) */
  void* sketch_ws;               /* sketch_bytes of backward scratch */
  void* scratch;                 /* mgs_gauss_newton_scratch_bytes */
  mgs_lm_step_args lm;           /* SJ / Sf / sj_* / rows / loss / zero_after are ignored */
  float* normal_out;             /* [44] or NULL */
} mgs_tracking_gn_args;

int32_t mgs_tracking_gn_args_size(void);
uint64_t mgs_gauss_newton_scratch_bytes(const mgs_raster_shape* shape);
int32_t mgs_tracking_iteration_gauss_newton(const mgs_tracking_gn_args* args, void* stream);
/* ... with the stacked RGB-D objective (mgs_tracking_depth_args as for mgs_tracking_iteration_second_order_rgbd) */
int32_t mgs_tracking_iteration_gauss_newton_rgbd(const mgs_tracking_gn_args* args, const mgs_tracking_depth_args* depth,
                                                 void* stream);
/* The same sequence up to the sums: normal_out (required) is written, nothing is solved and neither the pose, the
 * exposure, lm_state nor best is touched (the lm block may be zero).  depth may be NULL (monocular). */
int32_t mgs_normal_equations(const mgs_tracking_gn_args* args, const mgs_tracking_depth_args* depth, void* stream);

/* ---- headless viewer ("Headless viewer") -------------------------------------------------------------
 * The last step from the forward's float planes to a finished uint8 [H,W,3] frame, on the device: what the reference's
 * GUI does on the host with NumPy, imgviz, Open3D and OpenGL (gui/slam_gui.py:544-653, gui/gui_utils.py:24-66,
 * gui/gl_render/shaders/gau_frag.glsl:20-35).  Four entry points, all stream-ordered and without a host read. */

/* (a) float planes -> interleaved uint8.
 *   MGS_VIEW_RGB      out = (uint8)(clamp(x, 0, 1) * 255), truncated (slam_gui.py:644-651); src is [3,H,W]
 *   MGS_VIEW_DEPTH    t = (d - 0.1) / (max - 0.1), out = lut[index(t)]; src is [1,H,W]            (:578-588)
 *   MGS_VIEW_OPACITY  t = o / max, out = lut[index(t)]                                            (:590-600)
 * index(t) = min(255, (int)(clamp(t, 0, 1) * 256)).  max is the largest non-negative value of the plane (NaNs are
 * passed over), found by a launch of its own into `scratch`; the subtraction and the division are single correctly
 * rounded fp32 operations.  A NaN pixel is black; max <= lo gives t = 0 everywhere.  `lut` is the 256 x 3 colour map
 * (monogs_amd.viewer.JET_LUT), kept in LDS.  `out` must be 4-byte aligned; H * W * 3 must stay below 2^31. */
#define MGS_VIEW_RGB 0
#define MGS_VIEW_DEPTH 1
#define MGS_VIEW_OPACITY 2
typedef struct mgs_view_compose_args {
  int32_t width, height;
  int32_t mode;
  int32_t reserved0;
  const float* src;        /* [3,H,W] (MGS_VIEW_RGB) or [1,H,W] */
  const uint8_t* lut;      /* [256,3]; may be NULL for MGS_VIEW_RGB */
  uint8_t* out;            /* [H,W,3] */
  void* scratch;           /* mgs_view_compose_scratch_bytes() bytes, no initial state; may be NULL for MGS_VIEW_RGB */
} mgs_view_compose_args;

int32_t mgs_view_compose_args_size(void);
uint64_t mgs_view_compose_scratch_bytes(void);
int32_t mgs_view_compose(const mgs_view_compose_args* args, void* stream);

/* (b) the ellipsoid shader: gau_frag.glsl:20-35 with render_mod -3 (flat ball) and -4 (Gaussian ball) on THIS
 * rasteriser's projection and tile lists.  alpha = min(0.99, opacity * exp(power)) is made binary against a threshold
 * (0.22 / 0.4; `power > 0` and `alpha < 1/255` skip the splat first) and a pixel shows the NEAREST splat with alpha = 1:
 * hit_color = rgb (flat) or rgb * exp(power) (Gaussian), hit_depth = the splat's depth; without a hit the background
 * and 0.  Launch sequence: mgs_raster_forward_project, the pair emission and per-tile sort of
 * mgs_raster_forward_blend, then one forward-only walk of the sorted lists (no blend: fwd.out_color / out_depth /
 * out_opacity must be given as for the forward but are not written, fwd.n_touched is left zero).  Complete iff D <= fwd.shape.pair_capacity, as the blend. */
#define MGS_VIEW_FLAT_BALL 3
#define MGS_VIEW_GAUSSIAN_BALL 4
typedef struct mgs_view_ellipsoid_args {
  mgs_forward_args fwd;    /* the forward's argument block and workspaces */
  int32_t mode;            /* MGS_VIEW_FLAT_BALL or MGS_VIEW_GAUSSIAN_BALL */
  int32_t reserved0;
  float* hit_color;        /* [3,H,W] */
  float* hit_depth;        /* [1,H,W] */
} mgs_view_ellipsoid_args;

int32_t mgs_view_ellipsoid_args_size(void);
int32_t mgs_view_ellipsoid(const mgs_view_ellipsoid_args* args, void* stream);

/* (c) the time shader (slam_gui.py:550-558): out[n,k,:] = 0.1 * features[n,k,:] + 0.9 * lut[index(t_n)] / 255 for every
 * coefficient row k, t_n = (kf_ids[n] - id_min) / (id_max - id_min) (integer difference, one fp32 division; 0 when all
 * ids are equal), index() as in (a).  id_min / id_max are found by a launch of its own; `features` is not modified. */
typedef struct mgs_view_time_colors_args {
  int32_t num_gaussians;   /* N >= 1 */
  int32_t sh_coeffs;       /* K >= 1 */
  const float* features;   /* [N,K,3] */
  const int32_t* kf_ids;   /* [N] */
  const uint8_t* lut;      /* [256,3] */
  float* out;              /* [N,K,3] caller's scratch */
  void* scratch;           /* mgs_view_time_colors_scratch_bytes() bytes, no initial state */
} mgs_view_time_colors_args;

int32_t mgs_view_time_colors_args_size(void);
uint64_t mgs_view_time_colors_scratch_bytes(void);
int32_t mgs_view_time_colors(const mgs_view_time_colors_args* args, void* stream);

/* (d) frusta and free segments as 1-pixel lines over the frame, no depth test.
 * Segments, in index order: eight per pose (gui_utils.py:52-66: points (0,0,0), (1,-.5,2), (-1,-.5,2), (1,.5,2),
 * (-1,.5,2) times frustum_size in the pose's camera frame; lines 0-1 0-2 0-3 0-4 1-2 1-3 2-4 3-4), then the free ones.
 * Step 1 (fp32): world -> view space with T_view, clip at z = near_z, project x = fx X / Z + cx, y = fy Y / Z + cy,
 * clip to the guard rectangle [-W/2, 3W/2] x [-H/2, 3H/2], store round(16 x), round(16 y) and a valid flag in
 * `endpoints` ([S,5] int32: x0, y0, x1, y1, valid; S = 8 num_poses + num_free).  A segment wholly behind the near plane
 * or outside the rectangle is invalid and draws nothing.
 * Step 2 (integers only): n = ceil(max(|dx|, |dy|) / 16) steps; pixel k = 0..n is at
 * ((x0 + floor((2 dx k + n) / (2 n)) + 8) >> 4, likewise y), bounds-tested; n <= 2 max(W, H).  Where segments overlap
 * the pixel takes the colour of the HIGHEST segment index (an int32 owner map in `scratch`, atomicMax, then a second
 * walk that writes the owners' colours): the frame does not depend on the order of execution. */
typedef struct mgs_view_overlay_args {
  int32_t width, height;
  int32_t num_poses;          /* K >= 0 */
  int32_t num_free;           /* M >= 0 */
  float fx, fy, cx, cy;
  float frustum_size;
  float near_z;               /* > 0 */
  const float* T_view;        /* [4,4] row-major world -> camera of the viewing camera */
  const float* poses;         /* [K,4,4] row-major camera -> world, or NULL when K == 0 */
  const float* free_segments; /* [M,2,3] world-space end points, or NULL when M == 0 */
  const uint8_t* pose_colors; /* [K,3] */
  const uint8_t* free_colors; /* [M,3] */
  int32_t* endpoints;         /* [S,5] out (caller-visible) */
  uint8_t* frame;             /* [H,W,3] in / out */
  void* scratch;              /* mgs_view_overlay_scratch_bytes(W, H) bytes, no initial state */
} mgs_view_overlay_args;

int32_t mgs_view_overlay_args_size(void);
uint64_t mgs_view_overlay_scratch_bytes(int32_t width, int32_t height);   /* 0 for a bad size */
int32_t mgs_view_overlay(const mgs_view_overlay_args* args, void* stream);

/* ---- surface planes ("Surface planes") -----------------------------------------------------------------
 * Both calls are stream-ordered and read nothing back.
 *
 * (a) mgs_surface_forward: mgs_raster_forward_project, mgs_raster_forward_blend (fwd.out_color / out_depth /
 * out_opacity ARE written, exactly as by those two calls) and then one forward-only walk of the same sorted per-tile
 * lists.  Per pixel, in sort order: a splat counts iff power <= 0 and alpha = min(0.99, opacity * exp(power)) >= 1/255
 * (the blend's rules); T <- T * (1 - alpha) from T = 1; the MEDIAN splat is the first counting splat after which
 * T <= 0.5.  median_depth = that splat's view depth, median_index = its Gaussian id; 0 and -1 where T never reaches one
 * half (2DGS keeps the last splat there; this contract does not).  The blend's T < 1e-4 stop cannot come before the
 * crossing (T > 0.5 in front of it and alpha <= 0.99 leave T >= 0.005), so the walk has no stop rule.  Complete iff
 * D <= fwd.shape.pair_capacity, as the blend; fwd.bins and a pair capacity >= 1 are required. */
typedef struct mgs_surface_args {
  mgs_forward_args fwd;      /* as for the forward */
  float* median_depth;       /* [1,H,W] */
  int32_t* median_index;     /* [H,W] or NULL */
} mgs_surface_args;

int32_t mgs_surface_args_size(void);
int32_t mgs_surface_forward(const mgs_surface_args* args, void* stream);

/* (b) mgs_depth_normal: camera-frame unit normals of any depth plane (the median plane, the blend's depth / opacity,
 * sensor depth), every operation a single correctly rounded fp32 operation.  A depth is valid iff d > 0 and finite.  A
 * pixel has a normal iff it is not on the image border, its own depth d_c and its left, right, upper and lower
 * neighbours' depths d_n are valid and |d_n - d_c| <= max_jump * d_c for all four; otherwise the normal is (0,0,0).
 *   P(x,y) = (((x + pixel_center - cx) / fx) * d, ((y + pixel_center - cy) / fy) * d, d)
 *   a = P(x+1,y) - P(x-1,y);  b = P(x,y+1) - P(x,y-1);  n = b x a, each component one difference of two products;
 *   len = sqrt((nx^2 + ny^2) + nz^2);  normal = n / len per component, (0,0,0) when len is zero or not finite.
 * A fronto-parallel plane gives exactly (0,0,-1): towards the camera.  pixel_center is 0.5 for this rasteriser's
 * planes (its pixel coordinate is fx X / Z + cx - 0.5) and 0 for sensor planes. */
typedef struct mgs_depth_normal_args {
  int32_t width, height;
  float fx, fy, cx, cy;      /* fx, fy > 0 */
  float pixel_center;
  float max_jump;            /* >= 0 */
  const float* depth;        /* [H,W] */
  float* normal;             /* [3,H,W] */
} mgs_depth_normal_args;

int32_t mgs_depth_normal_args_size(void);
int32_t mgs_depth_normal(const mgs_depth_normal_args* args, void* stream);

/* ---- mesh export ("Mesh export") -----------------------------------------------------------------------
 * A dense lattice of nx x ny x nz sample points, point (i,j,k) at origin + (i,j,k) * voxel_size, i fastest; planes
 * tsdf (initial 1), weight (initial 0) and color [3,nz,ny,nx] (initial 0), all fp32 and caller-owned: the library keeps
 * no state.  Linear keys are 32-bit: 7 nx ny nz >= 2^31 gives MGS_ERR_UNSUPPORTED.
 *
 * (a) mgs_tsdf_integrate: ONE view, one launch, no host read.  Per lattice point, every operation a single fp32
 * rounding, in this order:
 *   p = origin + idx * vs per axis;  pc = ((R_0 px + R_1 py) + R_2 pz) + t  with the world-to-camera T
 *   skip unless zc > z_near;  u = fx * (xc / zc) + cx, v likewise;  pixel = floor(u + 0.5), floor(v + 0.5), tested
 *   against the image in float;  d = depth[v,u];  with `opacity`: skip if o < min_opacity, and with `normalize`
 *   d = d / o;  skip unless d > depth_min and d <= depth_max;  sdf = d - zc;  skip if sdf < -trunc;
 *   tn = min(1, sdf / trunc);  W' = W + weight;  D' = (W * D + weight * tn) / W';  with `image` each colour channel
 *   C' = (W * C + weight * image[c,v,u]) / W';  stored weight min(W', max_weight).
 * Bricks of 32 x 8 x 4 points whose corners all lie beyond one plane of the view volume are left untouched; the
 * result is the un-culled one bit for bit. */
typedef struct mgs_tsdf_integrate_args {
  int32_t nx, ny, nz;
  int32_t width, height;
  int32_t normalize;         /* d = d / o (needs `opacity`) */
  float origin[3];
  float voxel_size;          /* > 0 */
  float trunc;               /* > 0 */
  float fx, fy, cx, cy;      /* fx, fy > 0 */
  float z_near, depth_min, depth_max;
  float min_opacity;
  float weight;              /* of this view, > 0 */
  float max_weight;          /* > 0 */
  int32_t reserved0;
  const float* T;            /* [4,4] row-major world -> camera, on the device */
  const float* depth;        /* [H,W] */
  const float* opacity;      /* [H,W] or NULL */
  const float* image;        /* [3,H,W] or NULL */
  float* tsdf;               /* [nz,ny,nx] */
  float* wsum;               /* [nz,ny,nx] the weight plane */
  float* color;              /* [3,nz,ny,nx]; may be NULL without `image` */
} mgs_tsdf_integrate_args;

int32_t mgs_tsdf_integrate_args_size(void);
int32_t mgs_tsdf_integrate(const mgs_tsdf_integrate_args* args, void* stream);

/* (b) surface extraction: marching tetrahedra over the Kuhn decomposition (six tetrahedra per cell, one per
 * permutation (a,b,c) of the axes: v0 = (0,0,0), v1 = v0 + e_a, v2 = v1 + e_b, v3 = (1,1,1)).  A cell is valid when
 * its eight corners have weight >= min_weight; a corner is inside when tsdf < 0.  A lattice point owns the 7 edges to
 * its neighbours at (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) (slots 0..6), key = 7 * linear + slot; an
 * edge carries a vertex iff its end points differ in sign and a valid cell contains it.  With a the owner and b the
 * other end: f = ta / (ta - tb), position pa + f * (pb - pa) per axis (single roundings), the colour likewise.
 * Vertices come out in ascending key order, faces as int32 triples wound so that (v1 - v0) x (v2 - v0) points to the
 * outside corners, ordered by cell, tetrahedron, triangle: two calls give the same bytes.
 *   mgs_tsdf_mesh_count   classify + scan into `scratch`; counts[0] = V, counts[1] = F (device; saturated at 2^31 - 1)
 *   mgs_tsdf_mesh_emit    after the caller has read counts: writes num_verts vertices / colours and num_faces faces
 *                         (never more: the counts bound every store).  num_verts = num_faces = 0 launches nothing.
 * `scratch` (mgs_tsdf_mesh_scratch_bytes, 0 for a bad size; no initial state) carries the classification from count to
 * emit; the planes must not change in between. */
typedef struct mgs_tsdf_mesh_args {
  int32_t nx, ny, nz;
  int32_t reserved0;
  float origin[3];
  float voxel_size;
  float min_weight;
  int32_t reserved1;
  const float* tsdf;
  const float* weight;
  const float* color;        /* [3,nz,ny,nx] or NULL (then `colors` is not written) */
  void* scratch;
  int32_t* counts;           /* [2] device (count only) */
  float* verts;              /* [num_verts,3] (emit only) */
  int32_t* faces;            /* [num_faces,3] (emit only) */
  float* colors;             /* [num_verts,3] or NULL (emit only) */
  int32_t num_verts, num_faces;   /* as read from counts (emit only) */
} mgs_tsdf_mesh_args;

int32_t mgs_tsdf_mesh_args_size(void);
uint64_t mgs_tsdf_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int32_t mgs_tsdf_mesh_count(const mgs_tsdf_mesh_args* args, void* stream);
int32_t mgs_tsdf_mesh_emit(const mgs_tsdf_mesh_args* args, void* stream);

/* ---- sparse TSDF volume ("Sparse TSDF volume") ---------------------------------------------------------
 * The dense lattice above without its box: point (i,j,k), any sign, lies at origin + (i,j,k) * voxel_size, formed as
 * above with the GLOBAL index.  A brick is 8 x 8 x 8 points, brick (bx,by,bz) holds i in [8 bx, 8 bx + 8) and likewise
 * j, k; brick coordinates lie in [-2^20, 2^20) and pack into the key (bx + 2^20) | (by + 2^20) << 21 | (bz + 2^20) << 42.
 * Storage is a caller-owned pool of max_bricks bricks (7 * 512 * max_bricks < 2^31, i.e. max_bricks <= 599186; more is
 * MGS_ERR_UNSUPPORTED): tsdf [cap,512] (initial 1), weight [cap,512] (initial 0), color [3,cap,512] (initial 0), the
 * local index of a point (lk * 8 + lj) * 8 + li; brick_coords int32 [cap,3]; the persistent map key -> brick id,
 * map_keys uint64 [table_size] (initial all ones) and map_vals int32 [table_size], table_size =
 * mgs_sparse_tsdf_table_size(max_bricks) (the smallest power of two >= 2 max_bricks); state int32 [4] (initial 0):
 * [0] bricks allocated, [1] bricks not allocated for want of capacity (summed over the views), [2] candidates outside
 * the coordinate range (summed), [3] new bricks the last view asked for.  The library keeps no state.
 * The contract: a sparse volume is the dense volume of the same origin and voxel size in which every point of an
 * unallocated brick has weight 0 (tsdf 1, colour 0).
 *
 * (a) mgs_sparse_tsdf_allocate: the bricks ONE view needs, no host read.  For every pixel (x, y) whose depth passes the
 * tests of mgs_tsdf_integrate (d = depth[y,x]; with `opacity`: skip if o < min_opacity, and with `normalize` d = d / o;
 * skip unless d > depth_min and d <= depth_max), for s in [0, samples) - samples = ceil(2 trunc / (4 vs)) + 1, formed
 * by the caller - every operation a single fp32 rounding, in this order:
 *   xn = (x - cx) / fx;  yn = (y - cy) / fy;  z = (d - trunc) + s * (4 * vs);  skip unless z > z_near;
 *   q = (xn * z - t_0, yn * z - t_1, z - t_2);  world p_a = (R_0a q_0 + R_1a q_1) + R_2a q_2  (the transpose of T's
 *   rotation);  l_a = (p_a - origin_a) / vs;  corner c in [0, 8): g_a = l_a + 4 if bit a of c else l_a - 4;
 *   b_a = floor(g_a * 0.125).  A corner with some b_a outside [-2^20, 2^20) (tested in float; NaN is outside) is dropped
 *   and counted in state[2].
 * The candidate index is pixel * 8 samples + 8 s + c (pixel = y * width + x).  Candidates whose key the map holds are
 * discarded; of the others the one of SMALLEST index represents its key; the representatives, in ascending candidate
 * order, are the view's new bricks 0, 1, ...; new brick r gets id state[0] + r; ids >= max_bricks are not allocated and
 * are counted in state[1].  The brick list is therefore a function of the inputs alone
 * (sparse_tsdf.allocate_bricks_torch is the mirror).  `scratch`: mgs_sparse_tsdf_allocate_scratch_bytes, no initial
 * state.  width * height * 8 * samples >= 2^31 is MGS_ERR_UNSUPPORTED.
 *
 * (b) mgs_sparse_tsdf_integrate: the update of mgs_tsdf_integrate, in its order of roundings, on every lattice point
 * of every allocated brick (one workgroup per brick, the grid sized by max_bricks, workgroups past state[0] leave at
 * once); the conservative brick cull of the dense kernel with its margins, on the brick's 8 x 8 x 8 corners.  No host
 * read; `scratch` is not used. */
typedef struct mgs_sparse_tsdf_volume {
  int32_t max_bricks;        /* >= 1 */
  int32_t reserved0;
  float origin[3];
  float voxel_size;          /* > 0 */
  float* tsdf;               /* [cap,512] */
  float* weight;             /* [cap,512] */
  float* color;              /* [3,cap,512]; may be NULL where no colour is read or written */
  int32_t* brick_coords;     /* [cap,3] */
  uint64_t* map_keys;        /* [table_size] */
  int32_t* map_vals;         /* [table_size] */
  int32_t* state;            /* [4] */
} mgs_sparse_tsdf_volume;

typedef struct mgs_sparse_tsdf_view_args {
  mgs_sparse_tsdf_volume vol;
  int32_t width, height;
  int32_t normalize;         /* d = d / o (needs `opacity`) */
  int32_t samples;           /* allocate only: >= 1 */
  float trunc;               /* > 0 */
  float fx, fy, cx, cy;      /* fx, fy > 0 */
  float z_near, depth_min, depth_max;
  float min_opacity;
  float view_weight;         /* integrate only: > 0 */
  float max_weight;          /* integrate only: > 0 */
  int32_t reserved0;
  const float* T;            /* [4,4] row-major world -> camera, on the device */
  const float* depth;        /* [H,W] */
  const float* opacity;      /* [H,W] or NULL */
  const float* image;        /* [3,H,W] or NULL (integrate only) */
  void* scratch;             /* allocate only */
} mgs_sparse_tsdf_view_args;

int32_t mgs_sparse_tsdf_volume_size(void);
int32_t mgs_sparse_tsdf_view_args_size(void);
uint64_t mgs_sparse_tsdf_table_size(int32_t max_bricks);          /* 0 for a bad max_bricks */
uint64_t mgs_sparse_tsdf_allocate_scratch_bytes(int32_t width, int32_t height, int32_t samples);   /* 0 for a bad size */
int32_t mgs_sparse_tsdf_allocate(const mgs_sparse_tsdf_view_args* args, void* stream);
int32_t mgs_sparse_tsdf_integrate(const mgs_sparse_tsdf_view_args* args, void* stream);
/* Enters the bricks [first, first + count) of brick_coords (distinct, in range, not in the map: the caller's word) into
 * the map with their own ids and sets state[0] = first + count: how a volume is built from a brick list. */
int32_t mgs_sparse_tsdf_register(const mgs_sparse_tsdf_volume* vol, int32_t first, int32_t count, void* stream);

/* (c) extraction: mgs_tsdf_mesh_count / _emit on the first num_bricks bricks (the caller has read state[0]).  Every
 * cell, edge and triangle decision is the dense one; a point of an absent brick has the flags of a point outside a dense
 * volume (not inside, no weight).  The virtual linear index of a point is brick * 512 + local: vertices come out in
 * ascending (brick * 512 + local) * 7 + slot, faces by brick, cell, tetrahedron, triangle.
 * `scratch` (mgs_sparse_tsdf_mesh_scratch_bytes(num_bricks)) carries the [num_bricks,27] neighbour table (brick ids,
 * -1 where absent, entry (dx + 1) + 3 (dy + 1) + 9 (dz + 1)) and the classification from count to emit. */
typedef struct mgs_sparse_tsdf_mesh_args {
  mgs_sparse_tsdf_volume vol;
  int32_t num_bricks;        /* 1 .. max_bricks, at most state[0] */
  float min_weight;
  void* scratch;
  int32_t* counts;           /* [2] device (count only) */
  float* verts;              /* [num_verts,3] (emit only) */
  int32_t* faces;            /* [num_faces,3] (emit only) */
  float* colors;             /* [num_verts,3] or NULL (emit only) */
  int32_t num_verts, num_faces;   /* as read from counts (emit only) */
} mgs_sparse_tsdf_mesh_args;

int32_t mgs_sparse_tsdf_mesh_args_size(void);
uint64_t mgs_sparse_tsdf_mesh_scratch_bytes(int32_t num_bricks);  /* 0 for a bad count */
int32_t mgs_sparse_tsdf_mesh_count(const mgs_sparse_tsdf_mesh_args* args, void* stream);
int32_t mgs_sparse_tsdf_mesh_emit(const mgs_sparse_tsdf_mesh_args* args, void* stream);

/* ---- ray cast of the volumes ("Ray cast of the volumes") ------------------------------------------------
 * Depth, normal and colour of the fused surface at a pose, from a dense or a sparse volume, without a mesh and without
 * a host read.  The torch mirror tsdf_raycast.raycast_torch is the contract; the device equals it bit for bit: every
 * pixel is independent and every operation below is a single fp32 rounding.
 *   Ray       pixel (x, y): xn = (x - cx) / fx, yn = (y - cy) / fy.  Samples in camera z: z_n = z_near + n * dz for
 *             n in [0, num_steps); dz = f32(step) * f32(voxel_size) and num_steps = floor((z_far - z_near) / dz) + 1
 *             are formed by the caller; 2 <= num_steps <= 2^20.  World point as mgs_sparse_tsdf_allocate forms it:
 *             q = (xn z - t_0, yn z - t_1, z - t_2), p_a = (R_0a q_0 + R_1a q_1) + R_2a q_2, l_a = (p_a - origin_a) / vs.
 *   Sample    b_a = floor(l_a); invalid unless every |b_a| < 2^23 (tested in float: a NaN is invalid); f_a = l_a - b_a.
 *             The eight points b + d, d in {0,1}^3, must each have weight >= min_weight (false for NaN).  A point
 *             outside the dense box, of an unallocated brick or of a brick coordinate outside [-2^20, 2^20) has weight
 *             0.  The value is lerp(a, b, f) = a + f * (b - a) along x, then y, then z.
 *   March     n ascending.  At a valid sample whose predecessor n - 1 was valid: f_prev > 0 && f <= 0 is a HIT;
 *             f_prev < 0 && f > 0 ends the ray as a back face (a miss); anything else continues.  Running out of n is
 *             a miss.
 *   Outputs   hit: t = f_prev / (f_prev - f), depth = z_{n-1} + t * dz, hit_step = n.  Miss: depth 0, normal and
 *             colour 0, hit_step -1 (ran out) or -2 (back face).
 *   At a hit  l* is formed again from `depth` by the sample expression.  Colour: the trilinear sample of the three
 *             colour planes at l* (0 without colour planes).  Gradient g_a = value(l* + e_a) - value(l* - e_a), the
 *             offset added to l_a in fp32.  L = sqrt((g_0^2 + g_1^2) + g_2^2).  If the sample at l* or one of the six
 *             is invalid, or L is not a finite value > 0, colour and normal are 0; otherwise normal = g / L (as
 *             mgs_face_normals), which points to the positive-TSDF side, and with frame MGS_RAYCAST_FRAME_CAMERA it is
 *             turned by T's rotation, n_r = (R_r0 n_0 + R_r1 n_1) + R_r2 n_2.
 *   skip      1: samples proved invalid (the base point's brick is absent; the ray is outside the dense box) are
 *             passed over; the result is the one of skip = 0, which evaluates every n.
 * One wave owns an 8 x 8 pixel tile.  The sparse ray cast reads the [max_bricks,27] neighbour table in `scratch`
 * (mgs_sparse_tsdf_raycast_scratch_bytes(max_bricks), 0 for a bad count); with build_table = 1 a launch over the pool
 * (entries past 27 * state[0] leave) writes it first - the caller asks for that whenever bricks were added since.  An
 * entry outside [0, max_bricks) is read as absent.
 * A null struct or needed array, H or W < 1, fx or fy not > 0, dz not > 0, a frame or skip outside {0, 1}, num_steps < 2:
 * MGS_ERR_BAD_ARGUMENT.  num_steps > 2^20, H * W >= 2^31 / 3: MGS_ERR_UNSUPPORTED.  A refused call launches nothing.
 *
 * mgs_raycast_shade: out [H,W,3] u8 from the ray cast's planes (normal in the CAMERA frame), one launch, one lane per
 * pixel.  A miss (hit_step < 0) gets `background`.  Channels are quantised as MGS_VIEW_RGB does.
 *   MGS_RAYCAST_SHADE_SHADED  grey 0.25 + 0.75 |n.z| (mgs_mesh_shade's headlight)
 *   MGS_RAYCAST_SHADE_NORMAL  0.5 n + 0.5 with n negated when (n.x rx + n.y ry) + n.z > 0, r the pixel's ray
 *   MGS_RAYCAST_SHADE_COLOR   the colour plane
 *   MGS_RAYCAST_SHADE_DEPTH   t = (d - lo) / (hi - lo), out = lut[min(255, (int)(clamp(t, 0, 1) * 256))]: MGS_VIEW_DEPTH's
 *                             rule with the range [lo, hi] given by the caller (the ray cast's z_near and z_far) in place
 *                             of the plane's maximum, which would cost a launch; a NaN is black */
#define MGS_RAYCAST_FRAME_CAMERA 0
#define MGS_RAYCAST_FRAME_WORLD 1
#define MGS_RAYCAST_MAX_STEPS (1 << 20)
#define MGS_RAYCAST_SHADE_SHADED 0
#define MGS_RAYCAST_SHADE_NORMAL 1
#define MGS_RAYCAST_SHADE_COLOR 2
#define MGS_RAYCAST_SHADE_DEPTH 3

typedef struct mgs_raycast_view {
  int32_t width, height;
  int32_t num_steps;         /* N: 2 .. 2^20 */
  int32_t frame;             /* MGS_RAYCAST_FRAME_* */
  int32_t skip;              /* 0 or 1 */
  int32_t reserved0;
  float fx, fy, cx, cy;      /* fx, fy > 0 */
  float z_near, dz;          /* dz > 0 */
  float min_weight;
  int32_t reserved1;
  const float* T;            /* [4,4] row-major world -> camera, on the device */
  float* depth;              /* [H,W] out */
  float* normal;             /* [H,W,3] out */
  float* color;              /* [H,W,3] out */
  int32_t* hit_step;         /* [H,W] out */
  int32_t* evaluated;        /* [H,W] out or NULL: the samples the march evaluated - a diagnostic, it depends on skip */
} mgs_raycast_view;

typedef struct mgs_tsdf_raycast_args {
  int32_t nx, ny, nz, reserved0;
  float origin[3];
  float voxel_size;          /* > 0 */
  const float* tsdf;         /* [nz,ny,nx] */
  const float* weight;       /* [nz,ny,nx] */
  const float* color;        /* [3,nz,ny,nx] or NULL */
  mgs_raycast_view view;
} mgs_tsdf_raycast_args;

typedef struct mgs_sparse_tsdf_raycast_args {
  mgs_sparse_tsdf_volume vol;
  mgs_raycast_view view;
  void* scratch;             /* the neighbour table */
  int32_t build_table;       /* 1: write the table before the ray cast */
  int32_t reserved0;
} mgs_sparse_tsdf_raycast_args;

typedef struct mgs_raycast_shade_args {
  int32_t width, height;
  int32_t mode;              /* MGS_RAYCAST_SHADE_* */
  float fx, fy, cx, cy;      /* NORMAL; fx, fy > 0 */
  float depth_lo, depth_hi;  /* DEPTH */
  uint8_t background[4];     /* r, g, b, spare */
  const float* depth;        /* [H,W] (DEPTH) */
  const float* normal;       /* [H,W,3] camera frame (SHADED, NORMAL) */
  const float* color;        /* [H,W,3] (COLOR) */
  const int32_t* hit_step;   /* [H,W] */
  const uint8_t* lut;        /* [256,3] (DEPTH) */
  uint8_t* out;              /* [H,W,3] */
} mgs_raycast_shade_args;

int32_t mgs_tsdf_raycast_args_size(void);
int32_t mgs_sparse_tsdf_raycast_args_size(void);
int32_t mgs_raycast_shade_args_size(void);
uint64_t mgs_sparse_tsdf_raycast_scratch_bytes(int32_t max_bricks);
int32_t mgs_tsdf_raycast(const mgs_tsdf_raycast_args* args, void* stream);
int32_t mgs_sparse_tsdf_raycast(const mgs_sparse_tsdf_raycast_args* args, void* stream);
int32_t mgs_raycast_shade(const mgs_raycast_shade_args* args, void* stream);

/* ---- frame-to-model ICP ("Frame-to-model ICP") ----------------------------------------------------------
 * Point-to-plane alignment of a sensor depth plane against a model view (a ray cast's depth and camera-frame normals, or
 * the surface planes of the viewer), the whole coarse-to-fine schedule enqueued at once, no host read.  The NumPy mirror
 * icp.align_numpy (icp_rows_numpy, icp_solve_numpy) is the contract; the device equals it bit for bit and two runs give
 * the same bytes: every fp32 and fp64 operation below is a single rounding and every sum is an integer sum.
 *   Unknown   the rigid D [3,4] that takes sensor-camera to model-camera coordinates, fp64.  D_0 = T_model * T_init^-1
 *             (rigid inverse and product below), the identity when T_init is NULL.
 *   Rigid     inverse: R' = R^T, t'_a = -((R'_a0 t_0 + R'_a1 t_1) + R'_a2 t_2).  Product C = A B: C.R_ab = (A.R_a0 B.R_0b +
 *             A.R_a1 B.R_1b) + A.R_a2 B.R_2b, C.t_a = ((A.R_a0 B.t_0 + A.R_a1 B.t_1) + A.R_a2 B.t_2) + A.t_a.  fp64.
 *   Rows      (mgs k_icp_rows) over the sensor pixels u = 0 (mod stride), v = 0 (mod stride), in fp32, D rounded once to
 *             fp32 (R, t), pixel centre 0 on both sides:
 *             1 d = depth[v,u], n_s = normal[:,v,u].  INVALID unless d > 0, d finite, d <= depth_max and n_s != (0,0,0).
 *             2 rx = (u - cx) / fx, ry = (v - cy) / fy; X = (rx d, ry d, d); p_a = ((R_a0 X_0 + R_a1 X_1) + R_a2 X_2) + t_a;
 *               n'_a = (R_a0 n_s0 + R_a1 n_s1) + R_a2 n_s2.
 *             3 RANGE unless p_2 > 0 and every |p_a| < 16.
 *             4 u' = rintf(mfx (p_0 / p_2) + mcx), v' = rintf(mfy (p_1 / p_2) + mcy).  OUTSIDE unless |u'|, |v'| < 2^23
 *               (in float, before the conversion to int: false for a NaN) and 0 <= u' < model_width, 0 <= v' <
 *               model_height.  Nothing is loaded before this test.
 *             5 d_m = model_depth[v',u'], n = model_normal at (v',u').  NO_MODEL unless d_m > 0, n != (0,0,0) and every
 *               |n_a| <= 1 (false for a NaN: a unit normal passes, and the bound below needs it).
 *             6 q = (((u' - mcx) / mfx) d_m, ((v' - mcy) / mfy) d_m, d_m), e = p - q.
 *             7 DISTANCE unless (e_0^2 + e_1^2) + e_2^2 <= dist * dist; NORMAL unless (n_0 n'_0 + n_1 n'_1) + n_2 n'_2 >=
 *               cos_min.
 *             8 J = [n ; p x n] (translation first, the tau = [rho; theta] of mgs_pose_adam_args),
 *               p x n = (p_1 n_2 - p_2 n_1, p_2 n_0 - p_0 n_2, p_0 n_1 - p_1 n_0); r = (n_0 e_0 + n_1 e_1) + n_2 e_2.
 *             9 with w = [J r], the 28 products w_i w_j (i <= j, row-major) are one fp32 rounding each, and each enters
 *               its sum as the int64 trunc(v * 2^30), exact in fp64.
 *   Sums      28 int64 sums, the count of accepted pixels and one count per rejection (INVALID, RANGE, OUTSIDE,
 *             NO_MODEL, DISTANCE, NORMAL): MGS_ICP_SUMS = 35 words, integer adds only, so any order gives the same bits.
 *             Bound: |n_a| <= 1 and |p_a| < 16 give |J_i| < 2^5; dist <= 8 gives |r| <= sqrt(3) dist < 2^5; a product
 *             is below 2^10, its fixed-point value below 2^40, and width * height <= 2^22 (else MGS_ERR_UNSUPPORTED)
 *             keeps every sum below 2^62.  depth_max > 16 or dist > 8: MGS_ERR_BAD_ARGUMENT.
 *   Solve     (k_icp_solve, one thread, fp64).  accepted < min_pixels: MGS_ICP_TOO_FEW.  H_ij = sum / 2^30 (i, j < 6),
 *             g_i = sum_(i,6) / 2^30; H_ii += damping; m = max_i H_ii.  LDL^T by columns j: with t_k = L_jk d_k,
 *             pivot_j = H_jj - sum_k<j L_jk t_k (k ascending); the pivot is tested BEFORE any division by it: if not
 *             pivot_j > min_pivot_ratio * m the status is MGS_ICP_DEGENERATE, the column of L and d_j count as 0 and the
 *             factorisation goes on so that all six pivots are recorded; else d_j = pivot_j and L_ij = (H_ij - sum_k<j
 *             L_ik t_k) / d_j.  Then H x = -g: y_i = -g_i - sum_k<i L_ik y_k, z_i = y_i / d_i, x_i = z_i - sum_k>i L_ki
 *             x_k (k ascending).
 *   Update    s = (x_3^2 + x_4^2) + x_5^2, xx = x . x summed in index order.  Not s <= 0.25, or xx not finite:
 *             MGS_ICP_STEP_TOO_LARGE.  a = sum_k (-s)^k / (2k+1)!, b = sum_k (-s)^k / (2k+2)!, c = sum_k (-s)^k / (2k+3)!
 *             over k = 0 .. 6 by Horner's rule (MGS_ICP_EXP_TERMS: the first term left out is below one ulp of the
 *             coefficient at s = 0.25; the derivation is in icp.hip).  With W = [theta]x and W2 = theta theta^T - s I:
 *             R_E = (I + a W) + b W2, V = (I + b W) + c W2, t_E = V rho (summed as a rigid product's row), D <- E D.
 *             xx < converged * converged ends the level (MGS_ICP_CONVERGED); the last iteration of the last level
 *             otherwise ends with MGS_ICP_MAX_ITERATIONS.  A failure status leaves D and T_w2c as they were and ends
 *             everything; the launches of a level that has converged, and all launches after a failure, return at once.
 *   Outputs   T_w2c [4,4] f32 = D^-1 T_model (fp64, rounded once; written at the start and after every step), D [3,4]
 *             f64, record [MGS_ICP_RECORD_WORDS] of 8-byte words: 0..27 sums, 28..34 counts (accepted, then the
 *             rejections in the order above), 35..40 x (f64), 41..46 pivots (f64), 47 status, 48 level, 49 iteration
 *             within the level, 50 iterations run, 51 the level that has converged (-1: none), of the last iteration
 *             that ran.  The history, one row of MGS_ICP_HISTORY_WORDS words per enqueued iteration, lies in `scratch`
 *             behind the partial sums, at byte mgs_icp_scratch_bytes(0): accepted, sum r^2 (fixed point), xx (f64),
 *             status, ran (0 / 1), level, iteration, spare.
 * Launches: one to start, then k_icp_rows (a persistent grid of at most MGS_ICP_ROWS_BLOCKS workgroups of 256, a wave per
 * 8 x 8 tile of the stride grid, one plain store of a row of partial sums per workgroup, no atomics) and k_icp_solve per
 * iteration.  `normal` is the plane mgs_depth_normal wrote with pixel_center = 0.
 * A null struct or needed pointer, a side < 1, a focal length not > 0, num_levels outside 1 .. MGS_ICP_MAX_LEVELS, a
 * stride or an iteration count < 1, more than MGS_ICP_MAX_ITERATIONS_TOTAL iterations, a layout flag outside {0, 1},
 * dist, cos_min, depth_max, min_pivot_ratio, damping or converged that is NaN or negative (cos_min: outside [-1, 1]):
 * MGS_ERR_BAD_ARGUMENT.  3 * model_width * model_height >= 2^31: MGS_ERR_UNSUPPORTED.  A refused call launches nothing. */
#define MGS_ICP_ITERATING 0          /* the last iteration stepped; more were enqueued */
#define MGS_ICP_CONVERGED 1
#define MGS_ICP_MAX_ITERATIONS 2
#define MGS_ICP_TOO_FEW 3
#define MGS_ICP_DEGENERATE 4
#define MGS_ICP_STEP_TOO_LARGE 5
#define MGS_ICP_MAX_LEVELS 8
#define MGS_ICP_MAX_ITERATIONS_TOTAL 1024
#define MGS_ICP_SUMS 35
#define MGS_ICP_RECORD_WORDS 56
#define MGS_ICP_HISTORY_WORDS 8
#define MGS_ICP_ROWS_BLOCKS 256
#define MGS_ICP_EXP_TERMS 7
#define MGS_ICP_MAX_PIXELS (1 << 22)

typedef struct mgs_icp_args {
  int32_t width, height;                 /* the sensor planes; width * height <= 2^22 */
  int32_t model_width, model_height;
  int32_t model_normal_chw;              /* 0: model_normal is [H,W,3] (the ray cast), 1: [3,H,W] (mgs_depth_normal) */
  int32_t num_levels;
  int32_t min_pixels;
  int32_t reserved0;
  int32_t stride[MGS_ICP_MAX_LEVELS];
  int32_t iterations[MGS_ICP_MAX_LEVELS];
  float fx, fy, cx, cy;                  /* sensor */
  float mfx, mfy, mcx, mcy;              /* model */
  float dist, cos_min, depth_max;
  float reserved1;
  double min_pivot_ratio, damping, converged;
  const float* depth;                    /* [H,W] sensor */
  const float* normal;                   /* [3,H,W] sensor */
  const float* model_depth;              /* [Hm,Wm] */
  const float* model_normal;
  const float* T_model;                  /* [4,4] world -> model camera */
  const float* T_init;                   /* [4,4] world -> sensor camera at the start, or NULL (= T_model) */
  void* scratch;                         /* mgs_icp_scratch_bytes(total iterations), 8-byte aligned */
  float* T_w2c;                          /* [4,4] out */
  double* D;                             /* [3,4] out */
  int64_t* record;                       /* [MGS_ICP_RECORD_WORDS] out */
} mgs_icp_args;

int32_t mgs_icp_args_size(void);   /* sizeof(mgs_icp_args): the binding checks its mirror against it when the library loads;
                                      the struct is not in mgs_struct_size()'s numbered list, which ends where it ended */
uint64_t mgs_icp_scratch_bytes(int32_t max_iterations_total);   /* 0 for a count outside 0 .. 1024 */
int32_t mgs_icp_align(const mgs_icp_args* args, void* stream);

/* ---- RGB-D alignment: photometric rows in the ICP ("RGB-D alignment") ------------------------------------
 * The combined cost E = sum r_geo^2 + lambda^2 sum r_I^2, r_I = I_model(pi(D p)) - I_sensor(u), lambda = photo_weight.
 * On a textured plane the photometric rows carry the three directions [n ; p x n] cannot see.  The mirror is
 * icp.align_numpy(image=, photo_weight=) (intensity_planes_torch, icp_rows_numpy(photo=)); the device equals it bit for
 * bit.  mgs_icp_align and everything above are untouched by this entry.
 *   Intensity (k_icp_intensity, one launch per image, a thread per pixel).  rgb is [H,W,3] (chw = 0, the ray cast's
 *             colour) or [3,H,W] (chw = 1, a camera's image); `valid` is NULL or an fp32 plane [H,W] that is on where its
 *             value is > 0 (false for a NaN; the model passes the ray cast's depth).  A pixel is VALID iff it lies in the
 *             image, every channel c has 0 <= c <= 1 (false for NaN and inf) and its valid value is on.  Its luma is
 *             I = (0.299 R + 0.587 G) + 0.114 B, fp32, one rounding per operation.  gx = 0.5 (I[y,x+1] - I[y,x-1]) is
 *             valid iff both of those pixels are valid, gy = 0.5 (I[y+1,x] - I[y-1,x]) likewise: the image border has no
 *             gradient.  Output planes [3,H,W] = (I, gx, gy).  k_depth_normal marks a pixel without a normal by a value no
 *             normal has, (0,0,0); in the same way an invalid I is written as -1 and an invalid gx or gy as 2, values no
 *             valid one has (0 <= I <= 1 + 2^-22, |g| <= 0.5 + 2^-23).  A reader takes I as valid iff I >= 0 and a
 *             gradient iff |g| <= 1, both false for a NaN.
 *   Rows      (k_icp_rows_rgbd; grid and lane mapping of k_icp_rows).  Steps 1 - 4 of "Rows" above, with the continuous
 *             position kept: x' = mfx (p_0 / p_2) + mcx, y' = mfy (p_1 / p_2) + mcy, u' = rintf(x'), v' = rintf(y').  A pixel
 *             that passes step 4 then gets BOTH rows, each under its own gates: the photometric row does not depend on
 *             steps 5 - 7 (a ray cast has colour exactly where it has depth, and a frame whose geometric match is rejected
 *             by distance or normal still constrains the in-plane motion), the geometric row and its seven counters are
 *             steps 5 - 9 unchanged, with today's bits.  A pixel that fails steps 1 - 4 enters no photometric counter.
 *             P1 I_s = intensity[0,v,u] must be valid, else PHOTO_INVALID.
 *             P2 x0 = floorf(x'), y0 = floorf(y').  PHOTO_INVALID unless |x0|, |y0| < 2^23 (in float, before the conversion)
 *                and 0 <= x0, x0 + 1 < model_width, 0 <= y0, y0 + 1 < model_height: nothing is loaded before this test.
 *                The four neighbours (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1) must be valid in I, gx and gy, else
 *                PHOTO_INVALID.  With ax = x' - x0, ay = y' - y0 (exact) a plane f is sampled as
 *                top = f00 + ax (f01 - f00), bot = f10 + ax (f11 - f10), f_m = top + ay (bot - top): I_m, gx_m, gy_m.
 *             P3 r_I = I_m - I_s.  a = gx_m mfx, b = gy_m mfy; J_p = (a / p_2, b / p_2, -(((a p_0 + b p_1) / p_2) / p_2));
 *                J = [J_p ; p x J_p] with p x J_p = (p_1 J_p2 - p_2 J_p1, p_2 J_p0 - p_0 J_p2, p_0 J_p1 - p_1 J_p0);
 *                w_i = lambda J_i (i < 6), w_6 = lambda r_I.  One rounding per operation, left to right as written.
 *             P4 PHOTO_BOUND unless every |w_i| < 16 (false for a NaN): fx / p_2 is unbounded at close range, so this is a
 *                gate per pixel and not an argument check.  The pixel's geometric row still counts.
 *             P5 PHOTO_ACCEPTED: the 28 products w_i w_j enter THE SAME 28 sums as trunc(v * 2^30), and trunc((r_I r_I) *
 *                2^30) enters the sum of r_I^2.
 *   Sums      MGS_ICP_RGBD_SUMS = 39 words: the 35 of MGS_ICP_SUMS, then PHOTO_ACCEPTED, PHOTO_INVALID, PHOTO_BOUND and the
 *             fixed-point sum of r_I^2.  Bound: a geometric product is below 2^10 (above), a photometric one below 16 * 16
 *             = 2^8, so a pixel adds less than 2^10 + 2^8 = 1.25 * 2^10 to a sum, in fixed point 1.25 * 2^40, and 2^22
 *             pixels less than 1.25 * 2^62 < 2^63.  r_I^2 <= (1 + 2^-21)^2 stays below 2^53.
 *   Solve     k_icp_solve's arithmetic on the combined sums.  MGS_ICP_TOO_FEW tests accepted + photo_accepted <
 *             min_pixels: a frame with texture and little valid geometry can still align.
 *   Outputs   those of mgs_icp_align; the record's words 52 .. 55 hold PHOTO_ACCEPTED, PHOTO_INVALID, PHOTO_BOUND and the
 *             sum of r_I^2, the history row's word 7 the sum of r_I^2 (its word 1 is the combined sum of r^2, the
 *             photometric part weighted by lambda^2).  `intensity` [3,H,W] and `model_intensity` [3,Hm,Wm] are written
 *             once per call, before the first iteration.
 * Launches: two of k_icp_intensity, one to start, then k_icp_rows_rgbd and the solve per iteration, all enqueued at once.
 * Refused with MGS_ERR_BAD_ARGUMENT, beside what mgs_icp_align refuses: a null image, model_color, intensity or
 * model_intensity, a layout flag outside {0, 1}, photo_weight NaN, negative or above MGS_ICP_PHOTO_WEIGHT_MAX (1024: with
 * |r_I| <= 1 + 2^-21 a larger one could only trip the gate).  3 * width * height >= 2^31: MGS_ERR_UNSUPPORTED. */
#define MGS_ICP_RGBD_SUMS 39
#define MGS_ICP_PHOTO_WEIGHT_MAX 1024.0f

typedef struct mgs_icp_intensity_args {
  int32_t width, height;
  int32_t chw;                           /* 0: rgb is [H,W,3], 1: [3,H,W] */
  int32_t reserved0;
  const float* rgb;
  const float* valid;                    /* [H,W]: on where > 0, or NULL (all on) */
  float* out;                            /* [3,H,W]: I, gx, gy */
} mgs_icp_intensity_args;

typedef struct mgs_icp_rgbd_args {
  mgs_icp_args icp;                      /* as for mgs_icp_align; scratch is mgs_icp_rgbd_scratch_bytes(total iterations) */
  float photo_weight;                    /* lambda, in [0, MGS_ICP_PHOTO_WEIGHT_MAX] */
  int32_t image_chw;                     /* the layout of `image` */
  int32_t model_color_chw;               /* the layout of `model_color` */
  int32_t reserved0;
  const float* image;                    /* the sensor's RGB */
  const float* model_color;              /* the model view's RGB; valid where model_depth > 0 */
  float* intensity;                      /* [3,H,W] out */
  float* model_intensity;                /* [3,Hm,Wm] out */
} mgs_icp_rgbd_args;

int32_t mgs_icp_intensity_args_size(void);
int32_t mgs_icp_rgbd_args_size(void);
uint64_t mgs_icp_rgbd_scratch_bytes(int32_t max_iterations_total);   /* partial rows of 39 words, then the history */
int32_t mgs_icp_intensity(const mgs_icp_intensity_args* args, void* stream);
int32_t mgs_icp_align_rgbd(const mgs_icp_rgbd_args* args, void* stream);

/* ---- mesh clean-up ("Mesh clean-up") -------------------------------------------------------------------
 * Connected components of an indexed triangle mesh (verts [V,3] f32, faces [F,3] i32, colors [V,3] f32 or NULL),
 * clusters kept by size, vertices / colours / faces compacted.  The NumPy mirror mesh_clean.clean_mesh_numpy is the
 * contract; the device equals it bit for bit, and two calls give the same bytes.
 *   Components   two vertices are connected when a face names both (connectivity through shared vertices).
 *   Labels       the label of a vertex is the SMALLEST vertex index of its component; a vertex no face names is its
 *                own label, with a cluster of 0 faces.
 *   Cluster size its number of faces; a face belongs to the cluster of its first index.  Degenerate (a,a,b) and
 *                duplicate faces are ordinary faces: they connect what they name and they count.
 *   Kept         a cluster is kept iff faces >= max(min_faces, 1) and, with keep_largest >= 0, its rank in the order
 *                (face count descending, label ascending) is < keep_largest.  keep_largest = -1, min_faces = 0 drops
 *                only the unreferenced vertices.
 *   Output       the kept vertices and colours in their original relative order, the kept faces in theirs, re-indexed.
 *   Bad indices  a face with an index outside [0,V) connects nothing, is counted into counts[4], never emitted.
 *   mgs_mesh_clean_count   label, count, select, flag and scan into `scratch`;
 *                          counts = (V', F', clusters with >= 1 face, kept clusters, bad faces) on the device
 *   mgs_mesh_clean_emit    after the caller has read counts: writes out_num_verts vertices / colours and out_num_faces
 *                          faces (never more: the counts bound every store).  Both 0 launches nothing.
 *   mgs_mesh_components    labels [V] only, under the same rule (uses `scratch`, `faces`, `labels`)
 * `scratch` (mgs_mesh_clean_scratch_bytes; no initial state) carries the flags from count to emit; `faces` must not
 * change in between.  A null struct, scratch, counts (count), a needed array that is null, a negative size, keep_largest
 * < -1 or min_faces < 0: MGS_ERR_BAD_ARGUMENT.  3 V >= 2^31 or 3 F >= 2^31: MGS_ERR_UNSUPPORTED, and scratch_bytes is
 * 0.  V = 0 or F = 0 is legal.  A refused call launches nothing and writes nothing. */
typedef struct mgs_mesh_clean_args {
  int32_t num_verts, num_faces;
  int32_t keep_largest;      /* -1: no limit */
  int32_t min_faces;         /* >= 0 */
  const float* verts;        /* [V,3] (emit only) */
  const int32_t* faces;      /* [F,3] */
  const float* colors;       /* [V,3] or NULL (emit only; then `out_colors` is not written) */
  void* scratch;
  int32_t* counts;           /* [5] device (count only) */
  int32_t* labels;           /* [V] device (mgs_mesh_components only) */
  float* out_verts;          /* [out_num_verts,3] (emit only) */
  int32_t* out_faces;        /* [out_num_faces,3] (emit only) */
  float* out_colors;         /* [out_num_verts,3] (emit only, with `colors`) */
  int32_t out_num_verts, out_num_faces;   /* as read from counts[0], counts[1] (emit only) */
} mgs_mesh_clean_args;

int32_t mgs_mesh_clean_args_size(void);
uint64_t mgs_mesh_clean_scratch_bytes(int32_t num_verts, int32_t num_faces);
int32_t mgs_mesh_clean_count(const mgs_mesh_clean_args* args, void* stream);
int32_t mgs_mesh_clean_emit(const mgs_mesh_clean_args* args, void* stream);
int32_t mgs_mesh_components(const mgs_mesh_clean_args* args, void* stream);

/* ---- mesh evaluation ("Mesh evaluation") ---------------------------------------------------------------
 * The geometry block of a reconstruction benchmark - accuracy, completion, precision / recall / F-score, Chamfer - from
 * points sampled on two surfaces and their nearest distances in both directions.  Three stages, each with a mirror in
 * monogs_amd/mesh_eval.py that defines it; the library keeps no state between calls.
 *
 * mgs_surface_sample   `num_samples` points uniform on the surface of (verts [V,3] f32, faces [F,3] i32).  Mirror:
 *   sample_surface_numpy, equal bit for bit.
 *     weight   n = (b - a) x (c - a), every product and difference rounded once; A = sqrt(nx^2 + ny^2 + nz^2), the sum
 *              left to right, the root correctly rounded; E = the binary exponent of the largest finite A (an integer
 *              maximum over bit patterns); q = uint32(trunc(A * 2^(30 - E))) < 2^31.  Non-finite A, or an index
 *              outside [0,V) (counted as bad): q = 0.
 *     CDF      C = inclusive prefix sum of q in uint64, T its total: integers, so exact in any order.
 *     words    (x,y,z,w) = row j of `randoms` [n,4] u32 when given, else Philox-4x32-10 of counter (j, 0, 2, 0) keyed by
 *              the halves of `seed`.
 *     sample   t = (x | y << 32) mod T; face = the smallest f with C[f] > t; k1 = z >> 8, k2 = w >> 8, both replaced by
 *              2^24 - k when k1 + k2 > 2^24; u = k * 2^-24; p = (a + u1 (b - a)) + u2 (c - a), every step rounded once.
 *     T = 0    (or F = 0): every face_index -1, every point NaN, record[0] = 1.
 *   record [MGS_SAMPLE_RECORD_INTS] i32 on the device: {T == 0, bad faces, low and high word of T}.
 *
 * mgs_nearest_distance   for every query the exact nearest of `ref`: d2 = min_r ((dx dx + dy dy) + dz dz), dx = q.x - r.x,
 *   every step rounded once; index = the smallest r that attains it ((d2, r) compared lexicographically).  A non-finite
 *   reference point is never a neighbour; a non-finite query, or no finite reference point, gives (inf, -1).  Mirror:
 *   nearest_distance_torch (brute force), equal bit for bit.  The search runs over a uniform grid built on the device
 *   (at most MGS_NEAREST_MAX_CELLS cells, at most MGS_NEAREST_MAX_DIM per axis); cell_size > 0 overrides the chosen
 *   cell size and is raised until the grid fits the same caps.
 *
 * mgs_mesh_eval_stats    one direction (0: pred -> gt, 1: gt -> pred) of d2 [num] into per-workgroup partials in `scratch`:
 *   over the finite d = sqrt(d2) their number, the number with d < threshold, the largest (integer maximum on the bit
 *   pattern) and the fp64 sum.  No float atomics.
 * mgs_mesh_eval_finish   after both directions: ONE workgroup adds the partials in a fixed order into record
 *   [MGS_MESH_EVAL_RECORD_DOUBLES] f64 on the device: {n finite, n below, max d, sum d} of direction 0, of direction 1,
 *   then {T == 0, bad faces} of sample_record[0] and of sample_record[1] (0 where the pointer is NULL).
 *
 * Every scratch (the *_scratch_bytes functions; no initial state) is sized from the host's numbers alone.  A null
 * struct, scratch or needed array, a negative size, a direction outside {0, 1}, a negative or NaN cell_size or
 * threshold: MGS_ERR_BAD_ARGUMENT.  3 V, 3 F, 3 n, 3 P or 3 Q >= 2^31: MGS_ERR_UNSUPPORTED, and scratch_bytes is 0.
 * Sizes of 0 are legal.  A refused call launches nothing and writes nothing. */
#define MGS_SAMPLE_RECORD_INTS 4
#define MGS_NEAREST_MAX_CELLS (1 << 21)
#define MGS_NEAREST_MAX_DIM 1024
#define MGS_MESH_EVAL_RECORD_DOUBLES 12

typedef struct mgs_surface_sample_args {
  int32_t num_verts, num_faces, num_samples, reserved0;
  uint64_t seed;
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3] */
  const uint32_t* randoms;   /* [n,4] or NULL: replayed instead of the generator */
  void* scratch;             /* mgs_surface_sample_scratch_bytes(num_faces) */
  float* points;             /* [n,3] out */
  int32_t* face_index;       /* [n] out */
  int32_t* record;           /* [MGS_SAMPLE_RECORD_INTS] device out */
} mgs_surface_sample_args;

typedef struct mgs_nearest_args {
  int32_t num_query, num_ref;
  float cell_size;           /* 0: chosen on the device */
  int32_t reserved0;
  const float* query;        /* [P,3] */
  const float* ref;          /* [Q,3] */
  void* scratch;             /* mgs_nearest_scratch_bytes(num_ref) */
  float* d2;                 /* [P] out */
  int32_t* index;            /* [P] out */
} mgs_nearest_args;

typedef struct mgs_mesh_eval_args {
  int32_t num, direction;
  float threshold;
  int32_t reserved0;
  const float* d2;                   /* [num] (stats only) */
  void* scratch;                     /* mgs_mesh_eval_scratch_bytes() */
  double* record;                    /* [MGS_MESH_EVAL_RECORD_DOUBLES] device (finish only) */
  const int32_t* sample_record[2];   /* device records of the two samplings, or NULL (finish only) */
} mgs_mesh_eval_args;

int32_t mgs_surface_sample_args_size(void);
uint64_t mgs_surface_sample_scratch_bytes(int32_t num_faces);
int32_t mgs_surface_sample(const mgs_surface_sample_args* args, void* stream);
int32_t mgs_nearest_args_size(void);
uint64_t mgs_nearest_scratch_bytes(int32_t num_ref);
int32_t mgs_nearest_distance(const mgs_nearest_args* args, void* stream);
int32_t mgs_mesh_eval_args_size(void);
uint64_t mgs_mesh_eval_scratch_bytes(void);
int32_t mgs_mesh_eval_stats(const mgs_mesh_eval_args* args, void* stream);
int32_t mgs_mesh_eval_finish(const mgs_mesh_eval_args* args, void* stream);

/* ---- mesh rendering and culling ("Mesh rendering and culling") -----------------------------------------
 * The depth image of a triangle mesh at a pose, the per-view visibility of vertices against such an image, and the cull
 * of what too few views saw - what reconstruction benchmarks apply to both meshes before mgs_surface_sample.  Every
 * output is an integer or a single IEEE rounding and independent of the execution order; the mirrors in
 * monogs_amd/mesh_render.py are the contract and the device equals them bit for bit.
 *
 * Projection (render and visibility; tsdf's): with T [4,4] row-major world-to-camera on the device,
 *   row(r) = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3];  u = fx (xc / zc) + cx, v = fy (yc / zc) + cy; every operation
 *   one fp32 rounding; pixel (x, y) is centred at u = x, v = y.
 *
 * mgs_mesh_render   depth [H,W] f32 (0 without a surface) and face_id [H,W] i32 (-1 without one) of (verts, faces).
 *   snap      X = rint(256 u), Y = rint(256 v) as int32, round-half-even.
 *   bad       a face with an index outside [0,V): counted in record[0], never drawn.
 *   skipped   a face with a vertex that has !(zc > z_near), a non-finite zc, or !(|X| <= 2^24) or !(|Y| <= 2^24) (which
 *             takes NaN and infinite u, v): counted in record[1].  There is NO near-plane clipping.
 *   coverage  int64 edge functions of the snapped vertices at (256 x, 256 y), all three multiplied by the sign of the
 *             doubled area 2A (2A = 0: the face is ignored); covered iff w0, w1, w2 >= 0 - inclusive, two-sided, no
 *             top-left rule.  Only the pixels of the face's box clamped to the image are tested.
 *   depth     iz_i = 1.0 / (double)zc_i; z = (float)((double)|2A| / ((w0 iz0 + w1 iz1) + w2 iz2)), every operation one
 *             fp64 rounding, w_i the weight of vertex i in the face's own order.
 *   winner    the minimum over the covering faces of the key (bits(z) << 32) | face: nearest, then smallest index.
 *   paths     a face whose clamped box holds more than `large_threshold` pixels is appended to a device list and drawn by
 *             a second launch of `large_grid` workgroups that stride the list, 256 threads striding the box; the others
 *             are drawn by one lane each.  Both write the same keys.  record[2] = faces on the list, record[3] = 0.
 *   Four launches (fill, faces, large faces, resolve), no host read.  `scratch`: mgs_mesh_render_scratch_bytes, no
 *   initial state.
 *
 * mgs_vertex_visibility   seen_count[v] += 1 for every vertex with zc > z_near, (floor(u + 0.5), floor(v + 0.5)) inside
 *   the image and - with `depth` [H,W] - d = depth[pixel]: !(d > 0) ? empty_visible : !((zc - d) > eps), one rounding
 *   each.  One thread per vertex, one launch, no atomics.
 *
 * mgs_mesh_cull_count / mgs_mesh_cull_emit   keep a face iff its indices lie in [0,V) and all (rule 0) or any (rule 1)
 *   of its vertices have seen_count >= min_views; keep the vertices a kept face names; both in their order, the faces
 *   re-indexed.  count: counts = (V', F', bad faces, 0) on the device.  emit, after the caller has read counts: as
 *   mgs_mesh_clean_emit.  `faces` and `seen_count` must not change in between.
 *
 * A null struct, scratch or needed array, a negative size, H or W < 1, a rule outside {0, 1}: MGS_ERR_BAD_ARGUMENT.
 * 3 V, 3 F >= 2^31 or H W >= 2^31: MGS_ERR_UNSUPPORTED, and scratch_bytes is 0.  V = 0 or F = 0 is legal.  A refused call
 * launches nothing and writes nothing. */
#define MGS_MESH_RENDER_RECORD_INTS 4
#define MGS_MESH_RENDER_LARGE_BOX 1024     /* the default large_threshold */
#define MGS_MESH_RENDER_LARGE_GRID 256     /* the default large_grid */
#define MGS_MESH_CULL_COUNTS 4

typedef struct mgs_mesh_render_args {
  int32_t num_verts, num_faces, width, height;
  int32_t large_threshold;   /* >= 0; negative: MGS_MESH_RENDER_LARGE_BOX */
  int32_t large_grid;        /* >= 1; 0: MGS_MESH_RENDER_LARGE_GRID */
  float fx, fy, cx, cy, z_near;
  int32_t reserved0;
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3] */
  const float* T;            /* [4,4] device */
  void* scratch;             /* mgs_mesh_render_scratch_bytes(height, width, num_faces) */
  float* depth;              /* [H,W] out */
  int32_t* face_id;          /* [H,W] out */
  int32_t* record;           /* [MGS_MESH_RENDER_RECORD_INTS] device out */
} mgs_mesh_render_args;

typedef struct mgs_vertex_visibility_args {
  int32_t num_verts, width, height, empty_visible;
  float fx, fy, cx, cy, z_near, eps;
  const float* verts;        /* [V,3] */
  const float* T;            /* [4,4] device */
  const float* depth;        /* [H,W] or NULL: the frustum alone */
  int32_t* seen_count;       /* [V] incremented in place */
} mgs_vertex_visibility_args;

typedef struct mgs_mesh_cull_args {
  int32_t num_verts, num_faces, min_views;
  int32_t rule;              /* 0: all three vertices seen, 1: any */
  const float* verts;        /* [V,3] (emit only) */
  const int32_t* faces;      /* [F,3] */
  const float* colors;       /* [V,3] or NULL (emit only) */
  const int32_t* seen_count; /* [V] (count only) */
  void* scratch;             /* mgs_mesh_cull_scratch_bytes(num_verts, num_faces) */
  int32_t* counts;           /* [MGS_MESH_CULL_COUNTS] device (count only) */
  float* out_verts;          /* [out_num_verts,3] (emit only) */
  int32_t* out_faces;        /* [out_num_faces,3] (emit only) */
  float* out_colors;         /* [out_num_verts,3] (emit only, with `colors`) */
  int32_t out_num_verts, out_num_faces;   /* as read from counts[0], counts[1] (emit only) */
} mgs_mesh_cull_args;

int32_t mgs_mesh_render_args_size(void);
uint64_t mgs_mesh_render_scratch_bytes(int32_t height, int32_t width, int32_t num_faces);
int32_t mgs_mesh_render(const mgs_mesh_render_args* args, void* stream);
int32_t mgs_vertex_visibility_args_size(void);
int32_t mgs_vertex_visibility(const mgs_vertex_visibility_args* args, void* stream);
int32_t mgs_mesh_cull_args_size(void);
uint64_t mgs_mesh_cull_scratch_bytes(int32_t num_verts, int32_t num_faces);
int32_t mgs_mesh_cull_count(const mgs_mesh_cull_args* args, void* stream);
int32_t mgs_mesh_cull_emit(const mgs_mesh_cull_args* args, void* stream);

/* ---- mesh normals ("Mesh normals") -----------------------------------------------------------------------
 * Normals of faces and of vertices, the normal-consistency sums of a mesh evaluation, and the last step from a rendered
 * face-id plane to a uint8 frame.  Every output is an integer or a single IEEE rounding and independent of the
 * execution order; the mirrors in monogs_amd/mesh_normals.py and monogs_amd/mesh_render.py are the contract and the
 * device equals them bit for bit.
 *
 * Cross product (all of them; the sampler's): e = b - a, g = c - a, c = (e.y g.z - e.z g.y, e.z g.x - e.x g.z,
 *   e.x g.y - e.y g.x), every product and difference one fp32 rounding.  A face with an index outside [0,V) is BAD:
 *   counted in record[0], and it has no cross product.
 *
 * mgs_face_normals   normals [F,3]: L = sqrt((cx^2 + cy^2) + cz^2), the root correctly rounded; n = c / L by the
 *   correctly rounded division.  A face whose L is 0 or not finite is DEGENERATE: counted in record[1].  Bad and
 *   degenerate faces get (0,0,0).  One launch, one lane per face; `scratch` is not used.
 *
 * mgs_vertex_normals   normals [V,3]: the direction of the sum of the cross products of the faces that name the vertex
 *   (a face counts once per corner), i.e. the area-weighted normal, in fixed point.  A face with a non-finite component,
 *   or with c = (0,0,0), is DEGENERATE (record[1]) and left out.
 *     launch 1   M = the largest |component| over the other faces (an integer maximum over bit patterns); E = its
 *                binary exponent.
 *     launch 2   q = trunc(c 2^(30 - E)) per component, the product exact in fp64, truncated toward zero: |q| < 2^31;
 *                q is added to the int64[3] sums of the face's three corners by 64-bit integer atomics - exact in any
 *                order, and below 2^62 for every F < 2^31.
 *     launch 3   s = (double)sum; n = (float)(s / sqrt((sx^2 + sy^2) + sz^2)), every operation one fp64 rounding;
 *                (0,0,0) where the sum is zero: a vertex no usable face names, faces that cancel, M = 0.
 *   A face whose cross product is below 2^-30 of the largest contributes nothing (the sampler's rule for areas).
 *   `scratch`: mgs_vertex_normals_scratch_bytes(num_verts), no initial state.
 *
 * mgs_mesh_eval_normal_stats   one direction (0: pred -> gt, 1: gt -> pred).  Sample i lies on face `face[i]` of its
 *   mesh and has the neighbour index[i] at squared distance d2[i], which lies on face ref_face[index[i]] of the other.
 *   With n, m the two face normals: t = (n.x m.x + n.y m.y) + n.z m.z, every operation one fp32 rounding.  The pair is
 *   SKIPPED, and counted, when index[i] or either face index is out of range, d2[i] is not finite, or either normal is
 *   (0,0,0).  Per-workgroup partials in `scratch`: pairs, the fp64 sum of |t|, pairs with t < 0, skipped pairs.
 * mgs_mesh_eval_normal_finish  after both directions: ONE workgroup adds the partials in a fixed order into `record`
 *   [MGS_MESH_EVAL_NORMAL_DOUBLES] f64 on the device: {pairs, sum |t|, pairs with t < 0, skipped} of direction 0, of
 *   direction 1.  monogs_amd.mesh_eval passes the tail of a buffer whose head is mgs_mesh_eval_finish's record.
 *
 * mgs_mesh_shade   out [H,W,3] u8 from face_id [H,W] (mgs_mesh_render's); one launch, one lane per pixel.  A pixel with
 *   a face id outside [0,F) gets `background`.  Every channel is quantised as MGS_VIEW_RGB does: (uint8)(clamp(x, 0, 1)
 *   255), truncated.  With R the rotation of T and n the face's normal (face_normal [F,3]), n_c = R n per row as
 *   (r0 n.x + r1 n.y) + r2 n.z:
 *     MGS_MESH_SHADE_SHADED   grey I = 0.25 + 0.75 |n_c.z|: a two-sided headlight.
 *     MGS_MESH_SHADE_NORMAL   0.5 n_c + 0.5 with n_c turned to face the camera, as mgs_depth_normal's normals do: with
 *                             the pixel's ray r = ((x - cx) / fx, (y - cy) / fy, 1), n_c is negated when
 *                             (n_c.x r.x + n_c.y r.y) + n_c.z > 0.  A (0,0,0) normal is mid-grey.
 *     MGS_MESH_SHADE_COLOR    the face is set up again as mgs_mesh_render does (projection, snap, int64 edge functions
 *                             at the pixel centre); t_i = w_i iz_i, c = ((t0 c0 + t1 c1) + t2 c2) / ((t0 + t1) + t2),
 *                             every operation one fp64 rounding, then one conversion to fp32.  colors [V,3] is fp32, or
 *                             uint8 (colors_u8 = 1), which is divided by 255 in fp32 first.  A face that cannot be set
 *                             up (it was not drawn by mgs_mesh_render) gets `background`.
 *     MGS_MESH_SHADE_MASK     writes `background` where there is no face and nothing elsewhere: the depth view is
 *                             mgs_view_compose(MGS_VIEW_DEPTH) of the rendered depth, then this.
 *
 * A null struct or needed array, a negative size, H or W < 1, a direction outside {0, 1}, a mode outside the four:
 * MGS_ERR_BAD_ARGUMENT.  3 V, 3 F, 3 n >= 2^31 or 3 H W >= 2^31: MGS_ERR_UNSUPPORTED, and scratch_bytes is 0.  Sizes of 0
 * are legal.  A refused call launches nothing and writes nothing. */
#define MGS_MESH_NORMAL_RECORD_INTS 2
#define MGS_MESH_EVAL_NORMAL_DOUBLES 8
#define MGS_MESH_SHADE_SHADED 0
#define MGS_MESH_SHADE_NORMAL 1
#define MGS_MESH_SHADE_COLOR 2
#define MGS_MESH_SHADE_MASK 3

typedef struct mgs_mesh_normals_args {
  int32_t num_verts, num_faces;
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3] */
  void* scratch;             /* mgs_vertex_normals_scratch_bytes(num_verts) (vertex normals only) */
  float* normals;            /* [F,3] (face normals) or [V,3] (vertex normals) out */
  int32_t* record;           /* [MGS_MESH_NORMAL_RECORD_INTS] device out: bad faces, degenerate faces */
} mgs_mesh_normals_args;

typedef struct mgs_mesh_eval_normal_args {
  int32_t num, num_ref;              /* samples of this direction's mesh, and of the other */
  int32_t num_faces, num_ref_faces;  /* faces of the two meshes */
  int32_t direction, reserved0;
  const float* d2;                   /* [num] (stats only) */
  const int32_t* index;              /* [num] neighbour among the other mesh's samples (stats only) */
  const int32_t* face;               /* [num] face of every sample (stats only) */
  const int32_t* ref_face;           /* [num_ref] face of every sample of the other mesh (stats only) */
  const float* normals;              /* [num_faces,3] (stats only) */
  const float* ref_normals;          /* [num_ref_faces,3] (stats only) */
  void* scratch;                     /* mgs_mesh_eval_normal_scratch_bytes() */
  double* record;                    /* [MGS_MESH_EVAL_NORMAL_DOUBLES] device (finish only) */
} mgs_mesh_eval_normal_args;

typedef struct mgs_mesh_shade_args {
  int32_t num_verts, num_faces, width, height;
  int32_t mode;              /* MGS_MESH_SHADE_* */
  int32_t colors_u8;         /* 1: colors is uint8 [V,3] */
  float fx, fy, cx, cy, z_near;
  uint8_t background[4];     /* r, g, b, spare */
  const float* verts;        /* [V,3] (COLOR) */
  const int32_t* faces;      /* [F,3] (COLOR) */
  const float* T;            /* [4,4] device (all but MASK) */
  const int32_t* face_id;    /* [H,W] */
  const float* face_normal;  /* [F,3] (SHADED, NORMAL) */
  const void* colors;        /* [V,3] f32 or u8 (COLOR) */
  uint8_t* out;              /* [H,W,3] */
} mgs_mesh_shade_args;

int32_t mgs_mesh_normals_args_size(void);
uint64_t mgs_vertex_normals_scratch_bytes(int32_t num_verts);
int32_t mgs_face_normals(const mgs_mesh_normals_args* args, void* stream);
int32_t mgs_vertex_normals(const mgs_mesh_normals_args* args, void* stream);
int32_t mgs_mesh_eval_normal_args_size(void);
uint64_t mgs_mesh_eval_normal_scratch_bytes(void);
int32_t mgs_mesh_eval_normal_stats(const mgs_mesh_eval_normal_args* args, void* stream);
int32_t mgs_mesh_eval_normal_finish(const mgs_mesh_eval_normal_args* args, void* stream);
int32_t mgs_mesh_shade_args_size(void);
int32_t mgs_mesh_shade(const mgs_mesh_shade_args* args, void* stream);

/* ---- mesh simplification ("Mesh simplification") -------------------------------------------------------
 * Vertex clustering of an indexed triangle mesh (verts [V,3] f32, faces [F,3] i32, colors [V,3] f32 or NULL): the
 * vertices of one cell of a uniform grid become one vertex, faces that collapse or repeat are dropped.  The NumPy mirror
 * mesh_simplify.simplify_mesh_numpy is the contract; the device equals it bit for bit, and two calls give the same bytes.
 *   Origin       `origin`, or with origin_from_verts = 1 the per-axis minimum over the vertices whose three coordinates
 *                are finite (an integer minimum over order-preserving keys of the floats; no host read).
 *   Cell         per axis, one fp32 rounding each: t = (v - o) / cell (IEEE division), c = floor(t), fr = t - c.  fr lies
 *                in [0, 1]: the difference is exact except for a negative t so small that it rounds to 1.  c must lie in
 *                [-2^20, 2^20); the key packs the three c + 2^20 into 63 bits.  A vertex with a non-finite coordinate or a
 *                cell out of range is BAD: it joins no cluster and is counted into counts[5].
 *   Clusters     the vertices of one key; the label of a cluster is its smallest vertex index.
 *   Position     per axis q = trunc(fr 2^24) as int64, S = sum of q over the n vertices of the cluster (< 2^55),
 *                m = double(S) / (double(n) 2^24), position = float(double(o) + (double(c) + m) double(cell)), every fp64
 *                operation one rounding, no contraction.
 *   Colour       x = fminf(fmaxf(x, 0), 1) (NaN gives 0), q = trunc(x 2^24), mean = float(double(S) / (double(n) 2^24)).
 *   Faces        every index is mapped to its label.  A face with two equal labels is COLLAPSED and dropped.  Two
 *                surviving faces whose label triples are equal as sets (any order, either winding) are DUPLICATES: the
 *                one with the smallest face index stays.  Kept faces keep their relative order and their winding.  A
 *                face with an index outside [0,V) is BAD: never emitted, counted into counts[6].
 *   Output       a cluster is emitted iff a kept face names it, in ascending label order; the faces are re-indexed.
 *   mgs_mesh_simplify_count  keys, both hash sets, sums, flags and scan into `scratch`; counts = (V', F', clusters,
 *                            collapsed faces, duplicate faces, bad vertices, bad faces, spare) on the device
 *   mgs_mesh_simplify_emit   after the caller has read counts: writes out_num_verts vertices / colours and out_num_faces
 *                            faces (never more: the counts bound every store).  Both 0 launches nothing.
 * `scratch` (mgs_mesh_simplify_scratch_bytes; no initial state) carries sums and flags from count to emit; `verts`,
 * `faces`, `cell` and the origin must not change in between.  A null struct, scratch, counts (count), a needed array that
 * is null, a negative size, a cell that is not a finite value > 0, a non-finite given origin: MGS_ERR_BAD_ARGUMENT.
 * 3 V >= 2^31 or 3 F >= 2^31: MGS_ERR_UNSUPPORTED, and scratch_bytes is 0.  V = 0 or F = 0 is legal.  A refused call
 * launches nothing and writes nothing. */
#define MGS_MESH_SIMPLIFY_COUNTS 8

typedef struct mgs_mesh_simplify_args {
  int32_t num_verts, num_faces;
  float cell;                /* edge of a cell, finite and > 0 */
  int32_t origin_from_verts; /* 1: the per-axis minimum of the finite vertices instead of `origin` */
  float origin[3];
  int32_t reserved0;
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3] */
  const float* colors;       /* [V,3] or NULL (then `out_colors` is not written) */
  void* scratch;
  int32_t* counts;           /* [MGS_MESH_SIMPLIFY_COUNTS] device (count only) */
  float* out_verts;          /* [out_num_verts,3] (emit only) */
  int32_t* out_faces;        /* [out_num_faces,3] (emit only) */
  float* out_colors;         /* [out_num_verts,3] (emit only, with `colors`) */
  int32_t out_num_verts, out_num_faces;   /* as read from counts[0], counts[1] (emit only) */
} mgs_mesh_simplify_args;

int32_t mgs_mesh_simplify_args_size(void);
uint64_t mgs_mesh_simplify_scratch_bytes(int32_t num_verts, int32_t num_faces);
int32_t mgs_mesh_simplify_count(const mgs_mesh_simplify_args* args, void* stream);
int32_t mgs_mesh_simplify_emit(const mgs_mesh_simplify_args* args, void* stream);

/* ---- mesh edges, topology and smoothing ("Mesh edges and smoothing") ------------------------------------
 * The unique undirected edges of an indexed triangle mesh (faces [F,3] i32 over V vertices) with the number of faces on
 * each, and smoothing over the unique-edge neighbours.  The NumPy mirrors mesh_topology.mesh_edges_numpy and
 * mesh_smooth.smooth_mesh_numpy are the contract; the device equals them bit for bit, and two calls give the same bytes.
 *   Half-edges   half-edge 3 f + k runs from faces[f,k] to faces[f,(k+1)%3]; its key is (lo << 32) | hi of the two.
 *   Faces        a face with an index outside [0,V) is BAD: no edge, counted into record[9].  A face with two equal
 *                indices is DEGENERATE: no edge, counted into record[8].
 *   Edges        the representative of an edge is the smallest half-edge index with its key; edges are emitted in
 *                ascending representative order as (lo, hi), edge_faces is the number of half-edges with the key.
 *   Vertices     vertex_degree: unique edges at the vertex.  vertex_flags bit 0: referenced (degree > 0), bit 1: on an
 *                edge whose count is not 2.
 *   record       [0] edges, [1] sum of the degrees (2 edges), [2] referenced vertices, [3] vertices with flag bit 1,
 *                [4] edges of count 1, [5] of count 2, [6] of count >= 3, [7] of count 2 with both half-edges in one
 *                direction, [8] degenerate faces, [9] bad faces, [10] bad vertices (mgs_mesh_smooth), the rest 0.
 *   mgs_mesh_edges_count  the edge set, the class counters, vertex_degree and vertex_flags; the record on the device
 *   mgs_mesh_edges_emit   after the caller has read record[0]: writes out_num_edges edges and counts (never more: the
 *                         count bounds every store).  0 launches nothing.
 *   mgs_mesh_smooth       `iterations` times a step of weight lam and, with taubin = 1, a step of weight mu; out_verts
 *                         [V,3].  One step, Jacobi style, with E = (bits >> 23) - 127 of the largest |coordinate| of
 *                         the input and K = 28: a vertex of degree 0, and with boundary_free = 0 a vertex whose flag
 *                         bit 1 is set, keeps its bits; every other one, per axis, S = sum over its d neighbours of
 *                         q(p_u) as int64, q(p) = int64(fmax(fmin(ldexp(double(p), K - E), 2^62), -2^62)),
 *                         m = ldexp(double(S) / double(d), E - K), p' = float(double(p) + w (m - double(p))), every
 *                         fp64 operation one rounding, no contraction.  A vertex with a non-finite coordinate is BAD:
 *                         counted into record[10]; the output then means nothing.
 * `scratch` (mgs_mesh_edges_scratch_bytes / mgs_mesh_smooth_scratch_bytes; no initial state) carries the set from count
 * to emit; `faces` must not change in between.  A null struct, scratch, record, a needed array that is null, a negative
 * size, iterations outside [0, MGS_MESH_SMOOTH_MAX_ITERATIONS], lam outside (0, 1], with taubin a mu outside [-1, 0):
 * MGS_ERR_BAD_ARGUMENT.  3 V >= 2^31 or 3 F > 2^30 (the hash table holds at most 2^31 words): MGS_ERR_UNSUPPORTED, and
 * scratch_bytes is 0.  V = 0 or F = 0 is legal.  A refused call launches nothing and writes nothing. */
#define MGS_MESH_EDGES_RECORD_INTS 16
#define MGS_MESH_SMOOTH_MAX_ITERATIONS 1000

typedef struct mgs_mesh_edges_args {
  int32_t num_verts, num_faces;
  const int32_t* faces;      /* [F,3] */
  void* scratch;
  int32_t* record;           /* [MGS_MESH_EDGES_RECORD_INTS] device */
  int32_t* vertex_degree;    /* [V] (count only) */
  int32_t* vertex_flags;     /* [V] (count only) */
  int32_t* edges;            /* [out_num_edges,2] (emit only) */
  int32_t* edge_faces;       /* [out_num_edges] (emit only) */
  int32_t out_num_edges;     /* as read from record[0] (emit only) */
  int32_t reserved0;
} mgs_mesh_edges_args;

typedef struct mgs_mesh_smooth_args {
  int32_t num_verts, num_faces;
  int32_t iterations;        /* in [0, MGS_MESH_SMOOTH_MAX_ITERATIONS] */
  int32_t taubin;            /* 1: every iteration is a lam step and a mu step; 0: a lam step */
  int32_t boundary_free;     /* 0: vertices with flag bit 1 are pinned; 1: they move */
  float lam, mu;
  int32_t reserved0;
  const float* verts;        /* [V,3] */
  const int32_t* faces;      /* [F,3] */
  void* scratch;
  int32_t* record;           /* [MGS_MESH_EDGES_RECORD_INTS] device */
  float* out_verts;          /* [V,3], not `verts` */
} mgs_mesh_smooth_args;

int32_t mgs_mesh_edges_args_size(void);
uint64_t mgs_mesh_edges_scratch_bytes(int32_t num_verts, int32_t num_faces);
int32_t mgs_mesh_edges_count(const mgs_mesh_edges_args* args, void* stream);
int32_t mgs_mesh_edges_emit(const mgs_mesh_edges_args* args, void* stream);
int32_t mgs_mesh_smooth_args_size(void);
uint64_t mgs_mesh_smooth_scratch_bytes(int32_t num_verts, int32_t num_faces);
int32_t mgs_mesh_smooth(const mgs_mesh_smooth_args* args, void* stream);

/* Per-kernel timing (diagnostics; used by bench.py for the roofline line).  While
 * enabled every kernel launch is bracketed by hipEvents on the launch stream.
 * mgs_profile_read waits for the recorded events, aggregates them by kernel name into
 * names[k*32 .. k*32+31] / total_ms[k] / launches[k], clears the log and returns the
 * number of distinct names (<= max_entries), or a negative status. */
int32_t mgs_profile_enable(int32_t on);
int32_t mgs_profile_read(int32_t max_entries, char* names, float* total_ms, int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* MONOGS_RASTER_H */
