// extern "C" entry points declared in include/monogs_raster.h.
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "launch.h"
#include "raster_kernels.h"
#include "sketch_kernels.h"

namespace mgs {
namespace {
struct ProfRec { const char* name; hipEvent_t a, b; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;
}  // namespace
bool profile_on() { return g_prof_on; }
hipError_t& launch_error_slot() {
  static thread_local hipError_t e = hipSuccess;
  return e;
}
void profile_push(const char* name, hipEvent_t a, hipEvent_t b) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.push_back({name, a, b});
}
}  // namespace mgs

namespace mgs {
int launch_forward_project(const KP& P, hipStream_t st);
int launch_forward_blend(const KP& P, hipStream_t st, const KObjDepth* PD = nullptr);
int launch_forward_sort(const KP& P, hipStream_t st);
int launch_view_first_hit(const KP& P, int mode, float* hit_color, float* hit_depth, hipStream_t st);
int launch_surface_median(const KP& P, float* median_depth, int* median_index, hipStream_t st);
int launch_backward(const KP& P, const KB& B, hipStream_t st, bool skip_tau_reduce, const SketchFuse* fuse);
int launch_normal_backward(const KP& P, const KB& B, hipStream_t st, const mgs_sketch_residual_args& A,
                           const mgs_tracking_depth_args* D, float* planes, float* l1_partial, float* partial);
int normal_eq_blocks(int T);
int normal_residual_blocks(long long num_pixels);
int launch_lm_solve_normal(const mgs_lm_step_args& L, const float* partial, int nblk, const float* l1_partial, int nl1,
                           float* normal_out, float* l1_out, int solve, hipStream_t st);
int launch_visibility(const int* n_touched, unsigned char* vis, int n, hipStream_t st);
int launch_radii_fold(const int* radii, float* max_radii, int n, hipStream_t st);
}  // namespace mgs

using namespace mgs;

namespace {

bool shape_ok(const mgs_raster_shape& s) {
  return s.num_gaussians >= 1 && s.width >= 1 && s.height >= 1 && s.sh_degree >= 0 &&
         s.sh_degree <= 3 && s.tanfovx > 0.f && s.tanfovy > 0.f && s.pair_capacity >= 0;
}

int fill_kp(const mgs_forward_args& a, bool need_bins, bool need_outputs, KP& P) {
  const mgs_raster_shape& s = a.shape;
  if (!shape_ok(s)) return MGS_ERR_BAD_ARGUMENT;
  if (!a.means3D || !a.opacities || !a.viewmatrix || !a.projmatrix || !a.projmatrix_raw ||
      !a.campos || !a.bg || !a.geom)
    return MGS_ERR_BAD_ARGUMENT;
  if (!a.cov3D_precomp && (!a.scales || !a.rotations)) return MGS_ERR_BAD_ARGUMENT;
  if (!a.shs && !a.colors_precomp) return MGS_ERR_BAD_ARGUMENT;
  if (a.shs && s.sh_coeffs < (s.sh_degree + 1) * (s.sh_degree + 1)) return MGS_ERR_BAD_ARGUMENT;
  if (need_bins && s.pair_capacity > 0 && !a.bins) return MGS_ERR_BAD_ARGUMENT;
  if (need_outputs &&
      (!a.out_color || !a.out_depth || !a.out_opacity || !a.radii || !a.n_touched))
    return MGS_ERR_BAD_ARGUMENT;
  const Layout L = make_layout(s);
  P.obj = KObj{};
  P.N = s.num_gaussians; P.W = s.width; P.H = s.height;
  P.grid_x = (s.width + kTile - 1) / kTile; P.grid_y = (s.height + kTile - 1) / kTile;
  P.T = P.grid_x * P.grid_y;
  P.pack = (s.num_gaussians <= kPackMaxN && P.T <= (1 << kPackBits)) ? 1 : 0;
  P.deg = s.sh_degree; P.K = a.shs ? s.sh_coeffs : 0; P.cap = s.pair_capacity;
  P.tanfovx = s.tanfovx; P.tanfovy = s.tanfovy;
  P.focal_x = s.width / (2.0f * s.tanfovx); P.focal_y = s.height / (2.0f * s.tanfovy);
  P.mod = s.scale_modifier;
  P.means = a.means3D; P.scales = a.cov3D_precomp ? nullptr : a.scales;
  P.rots = a.cov3D_precomp ? nullptr : a.rotations; P.covp = a.cov3D_precomp;
  P.opac = a.opacities; P.shs = a.colors_precomp ? nullptr : a.shs; P.precol = a.colors_precomp;
  P.V = a.viewmatrix; P.PM = a.projmatrix; P.Praw = a.projmatrix_raw; P.campos = a.campos;
  P.bg = a.bg;
  char* g = (char*)a.geom;
  P.rec = (SplatRec*)(g + L.rec);
  P.pair_count = (int*)(g + L.pair_count);
  P.pair_off = (int*)(g + L.pair_off);
  P.block_prefix = (int*)(g + L.block_prefix);
  P.scan_tmp = (int*)(g + L.scan_tmp);
  P.hit_mask = (unsigned int*)(g + L.hit_mask);
  P.tile_count = (int*)(g + L.tile_count);
  P.tile_offset = (int*)(g + L.tile_offset);
  P.tile_cursor = (int*)(g + L.tile_cursor);
  P.bin_table = (int*)(g + L.bin_table);
  P.final_TC = (float4*)(g + L.final_TC);
  P.final_DL = (int2*)(g + L.final_DL);
  P.seg_offset = (int*)(g + L.seg_offset);
  P.quad_last = (int*)(g + L.quad_last);
  P.counters = (int*)(g + L.counters);
  char* b = (char*)a.bins;
  P.keys = b ? (unsigned long long*)(b + L.keys) : nullptr;
  P.payload = b ? (unsigned int*)(b + L.payload) : nullptr;
  P.seg_rec = b ? (int4*)(b + L.seg_rec) : nullptr;
  P.ckpt = b ? (float*)(b + L.ckpt) : nullptr;
  P.reach = b ? (uint4*)(b + L.reach) : nullptr;
  P.max_segs = (int)L.max_segs;
  P.out_color = a.out_color; P.out_depth = a.out_depth; P.out_opacity = a.out_opacity;
  P.radii = a.radii; P.n_touched = a.n_touched; P.d_out = a.pair_count_out; P.d_max = a.pair_count_max;
  if (P.T <= kBinMaxTilesLds) { int nblk; bin_grid(P.N, nblk, P.per_block); }
  else P.per_block = 0x7fffffff;
  P.big_pass = a.big_tile_pass < 0 ? 0 : 1;
  P.clamp_up = 1;
  return MGS_OK;
}

}  // namespace

extern "C" {

int32_t mgs_abi_version(void) { return MGS_ABI_VERSION; }

int32_t mgs_struct_size(int32_t which) {
  switch (which) {
    case 0: return (int32_t)sizeof(mgs_raster_shape);
    case 1: return (int32_t)sizeof(mgs_workspace_sizes);
    case 2: return (int32_t)sizeof(mgs_forward_args);
    case 3: return (int32_t)sizeof(mgs_backward_args);
    case 4: return (int32_t)sizeof(mgs_pose_adam_args);
    case 5: return (int32_t)sizeof(mgs_mapping_loss_args);
    case 6: return (int32_t)sizeof(mgs_lm_step_args);
    case 7: return (int32_t)sizeof(mgs_tracking_loss_args);
    case 8: return (int32_t)sizeof(mgs_tracking_iter_args);
    case 9: return (int32_t)sizeof(mgs_sketch_residual_args);
    case 10: return (int32_t)sizeof(mgs_tracking_so_args);
    case 11: return (int32_t)sizeof(mgs_adam_group);
    case 12: return (int32_t)sizeof(mgs_map_plan_args);
    case 13: return (int32_t)sizeof(mgs_gather_tensor);
    case 14: return (int32_t)sizeof(mgs_map_gather_args);
    case 15: return (int32_t)sizeof(mgs_map_accum_args);
    case 16: return (int32_t)sizeof(mgs_map_activate_args);
    case 17: return (int32_t)sizeof(mgs_mapping_view_args);
    case 18: return (int32_t)sizeof(mgs_map_finish_args);
    case 19: return (int32_t)sizeof(mgs_map_append_args);
    case 20: return (int32_t)sizeof(mgs_ssim_loss_args);
    case 21: return (int32_t)sizeof(mgs_refine_view_args);
    case 22: return (int32_t)sizeof(mgs_tracking_depth_args);
    case 23: return (int32_t)sizeof(mgs_tracking_sample_args);
    case 24: return (int32_t)sizeof(mgs_keyframe_args);
    case 25: return (int32_t)sizeof(mgs_keyframe_seed_args);
    default: return -1;
  }
}

const char* mgs_status_string(int32_t status) {
  switch (status) {
    case MGS_OK: return "ok";
    case MGS_ERR_BAD_ARGUMENT: return "bad argument (null pointer, non-positive size or unsupported degree)";
    case MGS_ERR_LAUNCH: return "kernel launch failed (the kernel and HIP's message were written to stderr)";
    case MGS_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return "unknown status";
  }
}

int32_t mgs_raster_workspace_query(const mgs_raster_shape* shape, mgs_workspace_sizes* out) {
  if (!shape || !out || !shape_ok(*shape)) return MGS_ERR_BAD_ARGUMENT;
  const Layout L = make_layout(*shape);
  out->geom_bytes = L.geom_bytes; out->bins_bytes = L.bins_bytes; out->bwd_bytes = L.bwd_bytes;
  out->sketch_bytes = L.sketch_bytes;
  out->off_records = L.rec; out->off_pair_count = L.pair_count;
  out->off_tile_offset = L.tile_offset; out->off_final_T = L.final_TC;
  out->off_n_contrib = L.final_DL; out->off_counters = L.counters;
  out->off_keys = L.keys; out->off_payload = L.payload;
  return MGS_OK;
}

int32_t mgs_raster_forward_project(const mgs_forward_args* args, void* stream) {
  if (!args) return MGS_ERR_BAD_ARGUMENT;
  KP P;
  const int rc = fill_kp(*args, false, true, P);
  if (rc != MGS_OK) return rc;
  return launch_forward_project(P, (hipStream_t)stream);
}

int32_t mgs_raster_forward_blend(const mgs_forward_args* args, void* stream) {
  if (!args) return MGS_ERR_BAD_ARGUMENT;
  KP P;
  const int rc = fill_kp(*args, true, true, P);
  if (rc != MGS_OK) return rc;
  return launch_forward_blend(P, (hipStream_t)stream);
}

int32_t mgs_view_ellipsoid_args_size(void) { return (int32_t)sizeof(mgs_view_ellipsoid_args); }

// The ellipsoid shader of the headless viewer: project, emit + sort, then the first-hit walk (viewer.hip) in the
// place of the blend.
int32_t mgs_view_ellipsoid(const mgs_view_ellipsoid_args* args, void* stream) {
  if (!args || !args->hit_color || !args->hit_depth) return MGS_ERR_BAD_ARGUMENT;
  if (args->mode != MGS_VIEW_FLAT_BALL && args->mode != MGS_VIEW_GAUSSIAN_BALL) return MGS_ERR_BAD_ARGUMENT;
  if (!args->fwd.bins || args->fwd.shape.pair_capacity < 1) return MGS_ERR_BAD_ARGUMENT;
  KP P;
  int rc = fill_kp(args->fwd, true, true, P);
  if (rc != MGS_OK) return rc;
  if ((rc = launch_forward_project(P, (hipStream_t)stream)) != MGS_OK) return rc;
  if ((rc = launch_forward_sort(P, (hipStream_t)stream)) != MGS_OK) return rc;
  return launch_view_first_hit(P, args->mode, args->hit_color, args->hit_depth, (hipStream_t)stream);
}

int32_t mgs_surface_args_size(void) { return (int32_t)sizeof(mgs_surface_args); }

// Median depth (surface.hip): the ordinary forward, then one more walk of the lists it sorted.
int32_t mgs_surface_forward(const mgs_surface_args* args, void* stream) {
  if (!args || !args->median_depth) return MGS_ERR_BAD_ARGUMENT;
  if (!args->fwd.bins || args->fwd.shape.pair_capacity < 1) return MGS_ERR_BAD_ARGUMENT;
  KP P;
  int rc = fill_kp(args->fwd, true, true, P);
  if (rc != MGS_OK) return rc;
  if ((rc = launch_forward_project(P, (hipStream_t)stream)) != MGS_OK) return rc;
  if ((rc = launch_forward_blend(P, (hipStream_t)stream)) != MGS_OK) return rc;
  return launch_surface_median(P, args->median_depth, args->median_index, (hipStream_t)stream);
}

// skip_tau_reduce: the caller sums tau_partial itself (*tau_partials / *num_partials are set)
static int32_t raster_backward_impl(const mgs_backward_args* args, void* stream, bool skip_tau_reduce,
                                    const float** tau_partials, int32_t* num_partials,
                                    bool sketch_only = false, bool scratch_kept_zero = false,
                                    const SketchFuse* fuse = nullptr) {
  if (!args) return MGS_ERR_BAD_ARGUMENT;
  KP P;
  const int rc = fill_kp(args->fwd, true, false, P);
  if (rc != MGS_OK) return rc;
  if (!args->grad_color || !args->bwd || !args->grad_tau) return MGS_ERR_BAD_ARGUMENT;
  if (args->clamp_gradient_mode != 0 && args->clamp_gradient_mode != 1) return MGS_ERR_BAD_ARGUMENT;
  P.clamp_up = args->clamp_gradient_mode == MGS_CLAMP_GRAD_UPSTREAM;
  {   // per-Gaussian gradients: all of the mandatory four, or none at all (pose-only / mapping mode)
    const int have = (args->grad_means3D != nullptr) + (args->grad_means2D != nullptr) +
                     (args->grad_colors != nullptr) + (args->grad_opacities != nullptr);
    if (have != 0 && have != 4) return MGS_ERR_BAD_ARGUMENT;
    if (have == 0 && (args->grad_scales || args->grad_rotations || args->grad_cov3D))
      return MGS_ERR_BAD_ARGUMENT;
    if (args->map_accum) {
      const mgs_map_accum_args& m = *args->map_accum;
      if (have != 0 || args->sketch_mode != 0 || !args->fwd.scales || !args->fwd.rotations || !args->fwd.shs ||
          args->fwd.cov3D_precomp || args->fwd.colors_precomp || (m.scale_dims != 1 && m.scale_dims != 3) ||
          !m.raw_rotations || !m.grad_xyz || !m.grad_features_dc || !m.grad_opacity || !m.grad_scaling ||
          !m.grad_rotation || (args->fwd.shape.sh_coeffs > 1 && !m.grad_features_rest) ||
          ((m.gradnorm_inc != nullptr) != (m.denom_inc != nullptr)) || (m.visibility && !args->fwd.n_touched))
        return MGS_ERR_BAD_ARGUMENT;
    }
  }
  if (args->sketch_mode != 0 &&
      ((!args->sketch_indices && !args->sketch_bucket_flat) || !args->grad_sketch_dtau || !args->sketch_ws ||
       args->sketch_dim < 1 || args->stack_dim < 1))
    return MGS_ERR_BAD_ARGUMENT;
  const Layout L = make_layout(args->fwd.shape);
  KB B;
  B.grad_color = args->grad_color; B.grad_depth = args->grad_depth;
  char* w = (char*)args->bwd;
  B.pair_grad = (float*)(w + L.pair_grad);
  B.tau_partial = (float*)(w + L.tau_partial);
  B.g_means3D = args->grad_means3D; B.g_means2D = args->grad_means2D;
  B.g_colors = args->grad_colors; B.g_opac = args->grad_opacities;
  B.g_scales = args->grad_scales; B.g_rots = args->grad_rotations; B.g_cov = args->grad_cov3D;
  B.g_tau = args->grad_tau;
  B.pair_bound = args->pair_count_bound > 0 ? args->pair_count_bound : 0;
  B.sketch_mode = args->sketch_mode; B.sketch_dim = args->sketch_dim; B.stack_dim = args->stack_dim;
  B.sketch_only = (sketch_only && args->sketch_mode != 0) ? 1 : 0;
  B.scratch_kept_zero = (scratch_kept_zero && args->sketch_mode != 0) ? 1 : 0;
  B.sketch_idx = args->sketch_indices; B.g_sketch = args->grad_sketch_dtau;
  B.sketch_flat = args->sketch_indices ? nullptr : args->sketch_bucket_flat;
  char* sw = (char*)args->sketch_ws;
  B.slabs = sw ? (float*)(sw + L.slabs) : nullptr;
  B.slab_mask = sw ? (unsigned int*)(sw + L.slab_mask) : nullptr;
  B.splat_jac = sw ? (float*)(sw + L.splat_jac) : nullptr;
  memset(&B.map, 0, sizeof(B.map));
  if (args->map_accum) {
    const mgs_map_accum_args& m = *args->map_accum;
    KM& M = B.map;
    M.on = 1; M.scale_dims = m.scale_dims; M.accumulate = m.accumulate; M.add_reg = m.add_regulariser;
    M.reg_scale = m.regulariser_weight / (3.0f * (float)P.N);
    M.raw_rot = m.raw_rotations;
    M.g_xyz = m.grad_xyz; M.g_fdc = m.grad_features_dc; M.g_frest = m.grad_features_rest;
    M.g_opacity = m.grad_opacity; M.g_scaling = m.grad_scaling; M.g_rotation = m.grad_rotation;
    M.gradnorm_inc = m.gradnorm_inc; M.denom_inc = m.denom_inc; M.radii_max = m.radii_max;
    M.visibility = m.visibility;
    P.n_touched = args->fwd.n_touched;
  }
  if (tau_partials) *tau_partials = B.tau_partial;
  if (num_partials) *num_partials = (P.N + kPreBlock - 1) / kPreBlock;
  return launch_backward(P, B, (hipStream_t)stream, skip_tau_reduce, fuse);
}

int32_t mgs_raster_backward(const mgs_backward_args* args, void* stream) {
  return raster_backward_impl(args, stream, false, nullptr, nullptr);
}

}  // extern "C"

// D != nullptr: the RGB-D objective (include/monogs_raster.h: mgs_tracking_depth_args); the launch sequence is the
// monocular one with the depth row in the objective and grad_depth handed to the backward.
static int32_t tracking_iteration_impl(const mgs_tracking_iter_args* args, const mgs_tracking_depth_args* D, void* stream) {
  if (!args || !args->bwd || !args->grad_image || !args->grad_tau || !args->grad_exposure ||
      !args->one || !args->adam.T || !args->fwd.viewmatrix || !args->fwd.projmatrix)
    return MGS_ERR_BAD_ARGUMENT;
  if (args->fwd.shape.pair_capacity < 1) return MGS_ERR_BAD_ARGUMENT;
  // 9 launches: camera matrices (unless the caller says they are valid - the previous
  // iteration's Adam kernel has already written them), 5 forward (the last one also evaluates the objective:
  // un-normalised gradients + partial sums), 2 backward, 1 Adam + update_pose (which also sums the tau / exposure / squared-residual block
  // partials, applies the 1 / loss of the norm and refreshes the camera matrices).
  int32_t rc = MGS_OK;
  if (!args->camera_matrices_valid) {
    rc = mgs_camera_from_pose(args->adam.T, args->fwd.projmatrix_raw, const_cast<float*>(args->fwd.viewmatrix),
                              const_cast<float*>(args->fwd.projmatrix), stream);
    if (rc != MGS_OK) return rc;
  }
  if ((rc = mgs_raster_forward_project(&args->fwd, stream)) != MGS_OK) return rc;
  // The objective rides in the epilogue of the forward blend (raster_kernels.h: KObj): the quadrant wave that
  // finishes a pixel forms its residual, writes d(loss)/d(image) and leaves its sums as one partial per wave
  // in the geom workspace - no loss launch between the forward and the backward.
  mgs_tracking_loss_args L = args->loss;
  if (!L.gt || !L.exposure_a || !L.exposure_b || !L.scalars) return MGS_ERR_BAD_ARGUMENT;
  KP P;
  if ((rc = fill_kp(args->fwd, true, true, P)) != MGS_OK) return rc;
  const Layout lay = make_layout(args->fwd.shape);
  float* obj_partial = reinterpret_cast<float*>(static_cast<char*>(args->fwd.geom) + lay.obj_partial);
  if (L.pnorm > 0.f && L.pnorm < 1.f) return MGS_ERR_BAD_ARGUMENT;
  const float pn = L.pnorm > 0.f ? L.pnorm : 2.f;
  int32_t nblk = 4 * P.T;
  if (pn == 1.f || pn == 2.f) {
    P.obj.on = 1;
    P.obj.p1 = pn == 1.f;
    P.obj.exposure_eps = L.exposure_eps; P.obj.huber_delta = L.huber_delta;
    P.obj.gt = L.gt; P.obj.mask = L.mask; P.obj.exposure_a = L.exposure_a; P.obj.exposure_b = L.exposure_b;
    P.obj.grad_image = args->grad_image; P.obj.partial = obj_partial;
    KObjDepth PD{};
    if (D) {
      PD.gt_depth = D->gt_depth; PD.grad_depth = D->grad_depth;
      PD.w_rgb = D->w_rgb; PD.w_depth = D->w_depth;
      PD.depth_thr = D->depth_threshold; PD.opa_thr = D->opacity_threshold;
    }
    if ((rc = launch_forward_blend(P, (hipStream_t)stream, D ? &PD : nullptr)) != MGS_OK) return rc;
    L.partial = obj_partial;
  } else {
    // any other p >= 1 (powf per sample): the plain forward blend, then the one-pass loss kernel
    // (needs loss.partial: mgs_tracking_loss_partial_count floats)
    if (!L.partial) return MGS_ERR_BAD_ARGUMENT;
    if ((rc = launch_forward_blend(P, (hipStream_t)stream)) != MGS_OK) return rc;
    L.image = args->fwd.out_color; L.opacity = args->fwd.out_opacity; L.grad_image = args->grad_image;
    L.num_pixels = (int64_t)P.W * P.H;
    if (D) {
      mgs_tracking_depth_args Dd = *D;
      Dd.depth = args->fwd.out_depth;
      L.scalars = nullptr;                  // onepass form: the Adam kernel finishes the sums
      if ((rc = mgs_tracking_loss_rgbd_fused(&L, &Dd, &nblk, stream)) != MGS_OK) return rc;
      L.scalars = args->loss.scalars;
    } else if ((rc = mgs_tracking_loss_onepass(&L, &nblk, stream)) != MGS_OK) {
      return rc;
    }
  }
  mgs_backward_args B;
  memset(&B, 0, sizeof(B));
  B.fwd = args->fwd;
  B.grad_color = args->grad_image;
  B.grad_depth = D ? D->grad_depth : nullptr;
  B.bwd = args->bwd;
  B.grad_tau = args->grad_tau;
  const float* tau_partials = nullptr;
  int32_t npre = 0;
  if ((rc = raster_backward_impl(&B, stream, true, &tau_partials, &npre)) != MGS_OK) return rc;
  mgs_pose_adam_args A = args->adam;
  A.grad_trans = nullptr; A.grad_rot = nullptr; A.grad_a = nullptr; A.grad_b = nullptr;
  A.tau_partials = tau_partials; A.num_tau_partials = npre;
  A.exposure_partials = L.partial + nblk; A.num_exposure_partials = nblk;
  A.loss_partials = L.partial; A.num_loss_partials = nblk;
  A.loss_norm_mode = 1; A.loss_grad_out = args->one; A.loss_pnorm = pn;
  A.loss_view = L.scalars; A.loss_accum = nullptr;
  A.best = args->best; A.l1_partials = L.partial + 3 * (size_t)nblk; A.num_l1_partials = nblk;
  A.projection = args->fwd.projmatrix_raw;
  A.viewmatrix_out = const_cast<float*>(args->fwd.viewmatrix);
  A.projmatrix_out = const_cast<float*>(args->fwd.projmatrix);
  return mgs_pose_adam_step(&A, stream);
}

static bool depth_args_ok(const mgs_tracking_depth_args* D) {
  return D && D->gt_depth && D->grad_depth && D->w_rgb == D->w_rgb && D->w_depth == D->w_depth;
}

extern "C" {

int32_t mgs_tracking_iteration(const mgs_tracking_iter_args* args, void* stream) {
  return tracking_iteration_impl(args, nullptr, stream);
}

int32_t mgs_tracking_iteration_rgbd(const mgs_tracking_iter_args* args, const mgs_tracking_depth_args* depth,
                                    void* stream) {
  if (!depth_args_ok(depth)) return MGS_ERR_BAD_ARGUMENT;
  return tracking_iteration_impl(args, depth, stream);
}

}  // extern "C"

// Pixel-sampled first-order iteration (sampled_tracking.hip): the plain forward, then the sampled objective and its
// sparse pose backward leave per-tile partials that the Adam kernel sums like those of mgs_tracking_iteration.
static int32_t tracking_iteration_sampled_impl(const mgs_tracking_iter_args* args, const mgs_tracking_depth_args* D,
                                               const mgs_tracking_sample_args* S, void* stream) {
  if (!args || !S || !args->one || !args->adam.T || !args->fwd.viewmatrix || !args->fwd.projmatrix ||
      !S->indices || !S->scratch)
    return MGS_ERR_BAD_ARGUMENT;
  if (S->num_samples < 1 || S->num_samples > MGS_TRACK_SAMPLE_MAX) return MGS_ERR_UNSUPPORTED;
  if (args->fwd.shape.pair_capacity < 1) return MGS_ERR_BAD_ARGUMENT;
  const mgs_tracking_loss_args& L = args->loss;
  if (!L.gt || !L.exposure_a || !L.exposure_b || !L.scalars) return MGS_ERR_BAD_ARGUMENT;
  if (L.pnorm > 0.f && L.pnorm < 1.f) return MGS_ERR_BAD_ARGUMENT;
  int32_t rc = MGS_OK;
  KP P;
  if ((rc = fill_kp(args->fwd, true, true, P)) != MGS_OK) return rc;
  if (!args->camera_matrices_valid) {
    rc = mgs_camera_from_pose(args->adam.T, args->fwd.projmatrix_raw, const_cast<float*>(args->fwd.viewmatrix),
                              const_cast<float*>(args->fwd.projmatrix), stream);
    if (rc != MGS_OK) return rc;
  }
  if ((rc = mgs_raster_forward_project(&args->fwd, stream)) != MGS_OK) return rc;
  if ((rc = launch_forward_blend(P, (hipStream_t)stream)) != MGS_OK) return rc;
  const float pn = L.pnorm > 0.f ? L.pnorm : 2.f;
  const SampLayout SL = samp_layout(P.T, S->num_samples);
  char* w = static_cast<char*>(S->scratch);
  KS K{};
  K.K = S->num_samples; K.T = P.T; K.HW = P.W * P.H; K.replay = S->replay_indices ? 1 : 0; K.rgbd = D ? 1 : 0;
  K.key = S->key;
  K.image = args->fwd.out_color; K.opacity = args->fwd.out_opacity; K.depth = args->fwd.out_depth;
  K.gt = L.gt; K.mask = L.mask; K.exposure_a = L.exposure_a; K.exposure_b = L.exposure_b;
  K.exposure_eps = L.exposure_eps; K.huber_delta = L.huber_delta; K.pnorm = pn;
  if (D) {
    K.gt_depth = D->gt_depth; K.w_rgb = D->w_rgb; K.w_depth = D->w_depth;
    K.depth_thr = D->depth_threshold; K.opa_thr = D->opacity_threshold;
  }
  K.replay_idx = S->replay_indices; K.indices = S->indices; K.grad_out = S->grad_out;
  K.v = reinterpret_cast<float*>(w + SL.v); K.part = reinterpret_cast<float*>(w + SL.part);
  K.prefix = reinterpret_cast<double*>(w + SL.prefix); K.target = reinterpret_cast<double*>(w + SL.target);
  K.pos = reinterpret_cast<int*>(w + SL.pos); K.weight = reinterpret_cast<float*>(w + SL.weight);
  K.tau_part = reinterpret_cast<float*>(w + SL.tau_part); K.expo_part = reinterpret_cast<float*>(w + SL.expo_part);
  if ((rc = launch_sampled_pose(P, K, (hipStream_t)stream)) != MGS_OK) return rc;
  mgs_pose_adam_args A = args->adam;
  A.grad_trans = nullptr; A.grad_rot = nullptr; A.grad_a = nullptr; A.grad_b = nullptr;
  A.tau_partials = K.tau_part; A.num_tau_partials = P.T;
  A.exposure_partials = K.expo_part; A.num_exposure_partials = P.T;
  A.loss_partials = K.part; A.num_loss_partials = P.T;
  A.loss_norm_mode = 1; A.loss_grad_out = args->one; A.loss_pnorm = pn;
  A.loss_view = L.scalars; A.loss_accum = nullptr;
  A.best = args->best; A.l1_partials = K.part + P.T; A.num_l1_partials = P.T;
  A.projection = args->fwd.projmatrix_raw;
  A.viewmatrix_out = const_cast<float*>(args->fwd.viewmatrix);
  A.projmatrix_out = const_cast<float*>(args->fwd.projmatrix);
  return mgs_pose_adam_step(&A, stream);
}

extern "C" {

uint64_t mgs_tracking_sample_scratch_bytes(const mgs_raster_shape* shape, int32_t num_samples) {
  if (!shape || !shape_ok(*shape) || num_samples < 1 || num_samples > MGS_TRACK_SAMPLE_MAX) return 0;
  const int T = ((shape->width + kTile - 1) / kTile) * ((shape->height + kTile - 1) / kTile);
  return samp_layout(T, num_samples).bytes;
}

int32_t mgs_tracking_iteration_sampled(const mgs_tracking_iter_args* args, const mgs_tracking_depth_args* depth,
                                       const mgs_tracking_sample_args* sample, void* stream) {
  if (depth && !depth_args_ok(depth)) return MGS_ERR_BAD_ARGUMENT;
  return tracking_iteration_sampled_impl(args, depth, sample, stream);
}

}  // extern "C"

// Keyframe policy (keyframe_policy.hip): every argument is checked here, before anything is launched.
static int32_t keyframe_args_status(const mgs_keyframe_args* a) {
  if (!a || a->num_gaussians < 1 || a->num_pixels < 1 || a->window_len < 1 || a->window_size < 1)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->window_len > MGS_KF_MAX_WINDOW) return MGS_ERR_UNSUPPORTED;
  if (!a->n_touched || !a->depth || !a->opacity || !a->T_cur || !a->scratch || !a->result) return MGS_ERR_BAD_ARGUMENT;
  for (int w = 0; w < a->window_len; w++)
    if (!a->T_window[w] || !a->visibility[w] || a->visibility_len[w] != (int64_t)a->num_gaussians)
      return MGS_ERR_BAD_ARGUMENT;
  return MGS_OK;
}

extern "C" {

uint64_t mgs_keyframe_scratch_bytes(int32_t num_gaussians, int32_t num_pixels, int32_t window_len) {
  if (num_gaussians < 1 || num_pixels < 1 || window_len < 1 || window_len > MGS_KF_MAX_WINDOW) return 0;
  return kf_layout(num_gaussians, num_pixels).bytes;
}

int32_t mgs_keyframe_decide(const mgs_keyframe_args* args, void* stream) {
  const int32_t rc = keyframe_args_status(args);
  if (rc != MGS_OK) return rc;
  return launch_keyframe_decide(*args, (hipStream_t)stream);
}

}  // extern "C"

// Keyframe seeding (keyframe_seed.hip): likewise, every argument is checked before anything is launched or written.
static int32_t keyframe_seed_args_status(const mgs_keyframe_seed_args* a) {
  if (!a || a->width < 1 || a->height < 1 || a->row_capacity < 1 || (int64_t)a->width * a->height > 0x7fffffff)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->mode < 0 || a->mode > 2 || !(a->downsample >= 1.f)) return MGS_ERR_BAD_ARGUMENT;   // NaN fails too
  const double most = floor((double)a->width * (double)a->height / (double)a->downsample);
  if ((double)a->row_capacity < most) return MGS_ERR_BAD_ARGUMENT;
  if (!a->image || !a->T || !a->exposure_a || !a->exposure_b || !a->xyz || !a->features_dc || !a->log_scales ||
      !a->rots || !a->opacity_logit || !a->scratch || !a->result || !a->result_host)
    return MGS_ERR_BAD_ARGUMENT;
  if ((a->mode != 1 && !a->depth) || (a->mode == 0 && !a->opacity)) return MGS_ERR_BAD_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(a->scratch) & 15u) return MGS_ERR_BAD_ARGUMENT;
  return MGS_OK;
}

extern "C" {

uint64_t mgs_keyframe_seed_scratch_bytes(int32_t num_pixels, int32_t row_capacity) {
  if (num_pixels < 1 || row_capacity < 1) return 0;
  return keyframe_seed_scratch_bytes(num_pixels, row_capacity);
}

int32_t mgs_keyframe_seed(const mgs_keyframe_seed_args* args, void* stream) {
  const int32_t rc = keyframe_seed_args_status(args);
  if (rc != MGS_OK) return rc;
  return launch_keyframe_seed(*args, (hipStream_t)stream);
}

}  // extern "C"

namespace {
// The render and the mapping-mode backward of one view, shared by mgs_mapping_view_iteration and
// mgs_refine_view_iteration (the objective between them differs).
static int32_t map_view_render(const mgs_forward_args& fwd, const float* T, int32_t camera_matrices_valid, void* stream) {
  int32_t rc = MGS_OK;
  if (!camera_matrices_valid) {
    rc = mgs_camera_from_pose(T, fwd.projmatrix_raw, const_cast<float*>(fwd.viewmatrix), const_cast<float*>(fwd.projmatrix),
                              stream);
    if (rc != MGS_OK) return rc;
  }
  if ((rc = mgs_raster_forward_project(&fwd, stream)) != MGS_OK) return rc;
  return mgs_raster_forward_blend(&fwd, stream);
}

static int32_t map_view_backward(const mgs_forward_args& fwd, const float* grad_image, const float* grad_depth, void* bwd,
                                 float* grad_tau, const mgs_map_accum_args* accum, const float** tau_partials,
                                 int32_t* npre, void* stream) {
  mgs_backward_args B;
  memset(&B, 0, sizeof(B));
  B.fwd = fwd;
  B.grad_color = grad_image;
  B.grad_depth = grad_depth;
  B.bwd = bwd;
  B.grad_tau = grad_tau;
  B.map_accum = accum;
  return raster_backward_impl(&B, stream, true, tau_partials, npre);
}
}  // namespace

extern "C" {

int32_t mgs_mapping_view_iteration(const mgs_mapping_view_args* args, void* stream) {
  if (!args || !args->adam.T || !args->fwd.viewmatrix || !args->fwd.projmatrix || args->fwd.shape.pair_capacity < 1)
    return MGS_ERR_BAD_ARGUMENT;
  if (!args->forward_only && (!args->bwd || !args->grad_image || !args->grad_tau || !args->loss.partial || !args->loss.gt))
    return MGS_ERR_BAD_ARGUMENT;
  int32_t rc = MGS_OK;
  if ((rc = map_view_render(args->fwd, args->adam.T, args->camera_matrices_valid, stream)) != MGS_OK) return rc;
  if (args->forward_only) {
    if (args->accum.visibility) {
      return launch_visibility((const int*)args->fwd.n_touched, args->accum.visibility,
                               args->fwd.shape.num_gaussians, (hipStream_t)stream);
    }
    return MGS_OK;
  }
  // objective: value + gradients in one pass; the block sums are consumed by the Adam kernel
  mgs_mapping_loss_args L = args->loss;
  L.image = args->fwd.out_color; L.depth = args->fwd.out_depth;
  L.grad_image = args->grad_image; L.grad_depth = L.w_depth != 0.f ? args->grad_depth : nullptr;
  L.grad_out = nullptr;
  int32_t nblk = 0;
  if ((rc = mgs_mapping_loss_fused(&L, &nblk, stream)) != MGS_OK) return rc;
  // full backward in mapping mode
  const float* tau_partials = nullptr;
  int32_t npre = 0;
  if ((rc = map_view_backward(args->fwd, args->grad_image, L.grad_depth, args->bwd, args->grad_tau, &args->accum,
                              &tau_partials, &npre, stream)) != MGS_OK)
    return rc;
  // this view's pose / exposure optimiser step (+ update_pose), loss value
  mgs_pose_adam_args A = args->adam;
  A.grad_trans = nullptr; A.grad_rot = nullptr; A.grad_a = nullptr; A.grad_b = nullptr;
  A.tau_partials = tau_partials; A.num_tau_partials = npre;
  A.exposure_partials = L.apply_exposure ? L.partial + 2 * nblk : nullptr; A.num_exposure_partials = nblk;
  if (!L.apply_exposure) { A.exposure_a = nullptr; A.exposure_b = nullptr; }
  A.loss_partials = L.partial; A.num_loss_partials = nblk;
  const float hw = (float)L.num_pixels;
  A.loss_w_rgb = L.w_rgb / (3.f * hw); A.loss_w_depth = L.w_depth / hw;
  A.loss_view = args->loss_view; A.loss_accum = args->loss_accum;
  A.projection = args->fwd.projmatrix_raw;
  A.viewmatrix_out = const_cast<float*>(args->fwd.viewmatrix);
  A.projmatrix_out = const_cast<float*>(args->fwd.projmatrix);
  return mgs_pose_adam_step(&A, stream);
}

int32_t mgs_refine_view_iteration(const mgs_refine_view_args* args, void* stream) {
  if (!args || !args->T || !args->fwd.viewmatrix || !args->fwd.projmatrix || !args->fwd.out_color || !args->fwd.radii ||
      args->fwd.shape.pair_capacity < 1 || !args->bwd || !args->grad_image || !args->grad_tau || !args->max_radii2D ||
      !args->loss.gt || !args->loss.partial || !args->loss.loss)
    return MGS_ERR_BAD_ARGUMENT;
  int32_t rc = MGS_OK;
  if ((rc = map_view_render(args->fwd, args->T, args->camera_matrices_valid, stream)) != MGS_OK) return rc;
  // loss = (1 - lambda) l1 + lambda (1 - ssim) on the render as it is: no exposure, no mask (slam_backend.py:355-358)
  mgs_ssim_loss_args L = args->loss;
  L.channels = 3; L.height = args->fwd.shape.height; L.width = args->fwd.shape.width;
  L.image = args->fwd.out_color; L.grad_image = args->grad_image; L.grad_out = nullptr;
  if ((rc = mgs_ssim_loss(&L, stream)) != MGS_OK) return rc;
  // backward in mapping mode: this view's gradients alone, no statistics (no add_densification_stats in :341-367)
  mgs_map_accum_args M = args->accum;
  M.accumulate = 0; M.add_regulariser = 0;
  M.gradnorm_inc = nullptr; M.denom_inc = nullptr; M.radii_max = nullptr; M.visibility = nullptr;
  if ((rc = map_view_backward(args->fwd, args->grad_image, nullptr, args->bwd, args->grad_tau, &M, nullptr, nullptr,
                              stream)) != MGS_OK)
    return rc;
  return launch_radii_fold(args->fwd.radii, args->max_radii2D, args->fwd.shape.num_gaussians, (hipStream_t)stream);
}

}  // extern "C"

static int32_t tracking_iteration_so_impl(const mgs_tracking_so_args* args, const mgs_tracking_depth_args* D,
                                          void* stream) {
  if (!args) return MGS_ERR_BAD_ARGUMENT;
  const mgs_tracking_iter_args& b = args->base;
  if (!b.bwd || !b.grad_image || !b.grad_tau || !b.adam.T || !b.fwd.viewmatrix || !b.fwd.projmatrix ||
      b.fwd.shape.pair_capacity < 1 || !args->bucket || !args->weights || !args->accum || !args->sketch_ws ||
      !args->lm.lm_state || !args->lm.x_out || args->stack_dim < 1 || args->sketch_dim < 1 || args->repeat_dim < 0)
    return MGS_ERR_BAD_ARGUMENT;
  const int64_t HW = (int64_t)b.fwd.shape.width * b.fwd.shape.height;
  const int d = args->stack_dim * args->sketch_dim;
  const int R = args->repeat_dim > 0 ? args->repeat_dim : 1;
  const size_t rows = (size_t)R * d;
  // accum: Sf[R d] | sj_exposure[R d, 2] | sj_tau[R d, 6] | l1, l1 of the later repeats (dropped), pad
  float* Sf = args->accum;
  float* sj_exp = Sf + rows;
  float* sj_tau = sj_exp + 2 * rows;
  float* l1 = sj_tau + 6 * rows;
  hipStream_t st = (hipStream_t)stream;
  int32_t rc = MGS_OK;
  if (!b.camera_matrices_valid) {
    rc = mgs_camera_from_pose(b.adam.T, b.fwd.projmatrix_raw, const_cast<float*>(b.fwd.viewmatrix),
                              const_cast<float*>(b.fwd.projmatrix), stream);
    if (rc != MGS_OK) return rc;
  }
  if ((rc = mgs_raster_forward_project(&b.fwd, stream)) != MGS_OK) return rc;
  if ((rc = mgs_raster_forward_blend(&b.fwd, stream)) != MGS_OK) return rc;
  // Sf, sj_exposure and l1 are accumulated with atomics (sj_tau is zeroed by the backward).  With
  // scratch_kept_zero the caller guarantees zeros on the first call and the LM kernel / the bucket kernel -
  // the consumers - restore them: four hipMemsetAsync launches (~5 us each) less per iteration.
  const bool kept = args->scratch_kept_zero != 0;
  if (!kept && (!hip_ok("memset(sketch accumulators)", hipMemsetAsync(Sf, 0, sizeof(float) * 3 * rows, st)) ||
                !hip_ok("memset(sketch l1)", hipMemsetAsync(l1, 0, sizeof(float) * 4, st)))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  // From here on the accumulators may hold partial sums.  In kept-zero mode only the LAST kernels of the sequence
  // restore the zeros, so a failure in between (bad argument, unsupported size, a failed launch) must not leave
  // them dirty for the next call: clear them before returning the error (the backward's own scratch - slabs and
  // their masks - is rewritten completely by every launch).
  auto fail = [&](int32_t code) {
    if (kept) (void)hipMemsetAsync(args->accum, 0, sizeof(float) * (9 * rows + 4), st);
    return code;
  };
  // `repeat_dim` backward passes over ONE render (utils/slam_frontend.py:654-669): repeat r draws its own
  // partition and weights, sums its residual buckets into Sf[r] and harvests SJ[r]; the rows are stacked.
  for (int r = 0; r < R; r++) {
    mgs_sketch_residual_args Rr;
    memset(&Rr, 0, sizeof(Rr));
    Rr.image = b.fwd.out_color; Rr.opacity = b.fwd.out_opacity; Rr.gt = b.loss.gt; Rr.mask = b.loss.mask;
    Rr.exposure_a = b.loss.exposure_a; Rr.exposure_b = b.loss.exposure_b;
    Rr.exposure_eps = b.loss.exposure_eps; Rr.huber_delta = b.loss.huber_delta; Rr.num_pixels = HW;
    Rr.stack_dim = args->stack_dim; Rr.sketch_dim = args->sketch_dim;
    Rr.bucket = args->bucket + (size_t)r * HW; Rr.weights = args->weights + (size_t)r * HW; Rr.grad_image = b.grad_image;
    Rr.Sf = Sf + (size_t)r * d; Rr.sj_exposure = sj_exp + 2 * (size_t)r * d;
    Rr.l1 = r == 0 ? l1 : l1 + 1;               // the L1 criterion is the render's: counted once
    Rr.assign = 1;                              // the bucket partition is drawn inside the residual pass
    Rr.assign_key = args->key + 0x9E3779B97F4A7C15ull * (uint64_t)r;
    // the residual pass runs in ONE launch with the per-splat Jacobian preparation of the backward (first repeat;
    // the preparation depends on the camera alone, the later repeats reuse it)
    SketchFuse fuse;
    fuse.residual = &Rr; fuse.skip_prep = r > 0 ? 1 : 0;
    mgs_tracking_depth_args Dd;
    if (D) { Dd = *D; Dd.depth = b.fwd.out_depth; }
    fuse.depth = D ? &Dd : nullptr;
    if (!Rr.gt || !Rr.exposure_a || !Rr.exposure_b || !sketch_keys(HW, args->stack_dim, args->sketch_dim, Rr.assign_key, fuse.keys))
      return fail(MGS_ERR_BAD_ARGUMENT);
    fuse.keys.on = 1;
    mgs_backward_args B;
    memset(&B, 0, sizeof(B));
    B.fwd = b.fwd; B.grad_color = b.grad_image; B.bwd = b.bwd; B.grad_tau = b.grad_tau;
    B.grad_depth = D ? D->grad_depth : nullptr;
    B.sketch_mode = 1; B.sketch_dim = args->sketch_dim; B.stack_dim = args->stack_dim;
    B.sketch_bucket_flat = args->bucket + (size_t)r * HW; B.grad_sketch_dtau = sj_tau + 6 * (size_t)r * d;
    B.sketch_ws = args->sketch_ws;
    // only grad_sketch_dtau is consumed by the LM step: J-only backward (no per-splat sums,
    // no preprocess backward, no grad_tau)
    if ((rc = raster_backward_impl(&B, stream, true, nullptr, nullptr, true, kept, &fuse)) != MGS_OK) return fail(rc);
  }
  mgs_lm_step_args L = args->lm;
  L.SJ = nullptr; L.sj_tau = sj_tau; L.sj_exposure = sj_exp; L.Sf = Sf; L.rows = (int32_t)rows; L.loss = l1;
  L.T = b.adam.T; L.exposure_a = b.adam.exposure_a; L.exposure_b = b.adam.exposure_b;
  L.best = b.best;
  if (kept) { L.zero_after = args->accum; L.zero_count = (int32_t)(9 * rows + 4); }
  L.projection = b.fwd.projmatrix_raw;
  L.viewmatrix_out = const_cast<float*>(b.fwd.viewmatrix);
  L.projmatrix_out = const_cast<float*>(b.fwd.projmatrix);
  if ((rc = mgs_lm_solve_step(&L, stream)) != MGS_OK) return fail(rc);
  return MGS_OK;
}

// scratch of the dense Gauss-Newton iteration: planes [3][HW] | normal-equation partials | L1 partials | L1 total
namespace {
struct GnLayout { uint64_t planes, partial, l1_partial, l1, bytes; };
GnLayout gn_layout(const mgs_raster_shape& s) {
  GnLayout L;
  const uint64_t HW = (uint64_t)s.width * s.height;
  const uint64_t T = (uint64_t)((s.width + kTile - 1) / kTile) * ((s.height + kTile - 1) / kTile);
  uint64_t o = 0;
  L.planes = o; o = align_up(o + 3 * HW * 4);
  L.partial = o; o = align_up(o + (uint64_t)normal_eq_blocks((int)T) * kNormalSums * 4);
  L.l1_partial = o; o = align_up(o + (uint64_t)normal_residual_blocks((long long)HW) * 4);
  L.l1 = o; o = align_up(o + 16);
  L.bytes = o;
  return L;
}
}  // namespace

// solve == 0: mgs_normal_equations (the sums only)
static int32_t gauss_newton_impl(const mgs_tracking_gn_args* args, const mgs_tracking_depth_args* D, void* stream,
                                 int solve) {
  if (!args) return MGS_ERR_BAD_ARGUMENT;
  const mgs_tracking_iter_args& b = args->base;
  if (!b.bwd || !b.grad_image || !b.fwd.viewmatrix || !b.fwd.projmatrix || b.fwd.shape.pair_capacity < 1 ||
      !args->sketch_ws || !args->scratch || args->stack_dim < 1 || args->sketch_dim < 1 || !b.loss.gt ||
      !b.loss.exposure_a || !b.loss.exposure_b || !shape_ok(b.fwd.shape))
    return MGS_ERR_BAD_ARGUMENT;
  if (!b.camera_matrices_valid && !b.adam.T) return MGS_ERR_BAD_ARGUMENT;
  if (solve ? (!b.adam.T || !args->lm.lm_state || !args->lm.x_out || !(args->lm.increase_factor > 0.f) ||
               !(args->lm.decrease_factor > 0.f))
            : !args->normal_out)
    return MGS_ERR_BAD_ARGUMENT;
  if (D && !depth_args_ok(D)) return MGS_ERR_BAD_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  int32_t rc = MGS_OK;
  if (!b.camera_matrices_valid) {
    rc = mgs_camera_from_pose(b.adam.T, b.fwd.projmatrix_raw, const_cast<float*>(b.fwd.viewmatrix),
                              const_cast<float*>(b.fwd.projmatrix), stream);
    if (rc != MGS_OK) return rc;
  }
  if ((rc = mgs_raster_forward_project(&b.fwd, stream)) != MGS_OK) return rc;
  if ((rc = mgs_raster_forward_blend(&b.fwd, stream)) != MGS_OK) return rc;
  KP P;
  if ((rc = fill_kp(b.fwd, true, false, P)) != MGS_OK) return rc;
  const Layout L = make_layout(b.fwd.shape);
  const GnLayout G = gn_layout(b.fwd.shape);
  const int64_t HW = (int64_t)P.W * P.H;
  char* gs = (char*)args->scratch;
  float* planes = (float*)(gs + G.planes);
  float* partial = (float*)(gs + G.partial);
  float* l1_partial = (float*)(gs + G.l1_partial);
  float* l1 = (float*)(gs + G.l1);
  KB B;
  memset(&B, 0, sizeof(B));
  B.grad_color = b.grad_image; B.grad_depth = D ? D->grad_depth : nullptr;
  B.pair_grad = (float*)((char*)b.bwd + L.pair_grad);
  B.tau_partial = (float*)((char*)b.bwd + L.tau_partial);
  B.sketch_mode = 1; B.sketch_only = 1; B.sketch_dim = args->sketch_dim; B.stack_dim = args->stack_dim;
  char* sw = (char*)args->sketch_ws;
  B.slabs = (float*)(sw + L.slabs);
  B.slab_mask = (unsigned int*)(sw + L.slab_mask);
  B.splat_jac = (float*)(sw + L.splat_jac);
  mgs_sketch_residual_args Rr;
  memset(&Rr, 0, sizeof(Rr));
  Rr.image = b.fwd.out_color; Rr.opacity = b.fwd.out_opacity; Rr.gt = b.loss.gt; Rr.mask = b.loss.mask;
  Rr.exposure_a = b.loss.exposure_a; Rr.exposure_b = b.loss.exposure_b;
  Rr.exposure_eps = b.loss.exposure_eps; Rr.huber_delta = b.loss.huber_delta; Rr.num_pixels = HW;
  Rr.stack_dim = args->stack_dim; Rr.sketch_dim = args->sketch_dim;
  Rr.grad_image = b.grad_image;
  mgs_tracking_depth_args Dd;
  if (D) { Dd = *D; Dd.depth = b.fwd.out_depth; }
  if ((rc = launch_normal_backward(P, B, st, Rr, D ? &Dd : nullptr, planes, l1_partial, partial)) != MGS_OK) return rc;
  mgs_lm_step_args S = args->lm;
  S.SJ = nullptr; S.sj_tau = nullptr; S.sj_exposure = nullptr; S.Sf = nullptr; S.rows = 0; S.loss = l1;
  S.T = b.adam.T; S.exposure_a = b.adam.exposure_a; S.exposure_b = b.adam.exposure_b;
  S.best = b.best;
  S.zero_after = nullptr; S.zero_count = 0;
  S.projection = b.fwd.projmatrix_raw;
  S.viewmatrix_out = const_cast<float*>(b.fwd.viewmatrix);
  S.projmatrix_out = const_cast<float*>(b.fwd.projmatrix);
  return launch_lm_solve_normal(S, partial, normal_eq_blocks(P.T), l1_partial, normal_residual_blocks(HW),
                                args->normal_out, l1, solve, st);
}

extern "C" {

int32_t mgs_tracking_gn_args_size(void) { return (int32_t)sizeof(mgs_tracking_gn_args); }

uint64_t mgs_gauss_newton_scratch_bytes(const mgs_raster_shape* shape) {
  return shape && shape_ok(*shape) ? gn_layout(*shape).bytes : 0;
}

int32_t mgs_tracking_iteration_gauss_newton(const mgs_tracking_gn_args* args, void* stream) {
  return gauss_newton_impl(args, nullptr, stream, 1);
}

int32_t mgs_tracking_iteration_gauss_newton_rgbd(const mgs_tracking_gn_args* args, const mgs_tracking_depth_args* depth,
                                                 void* stream) {
  if (!depth_args_ok(depth)) return MGS_ERR_BAD_ARGUMENT;
  return gauss_newton_impl(args, depth, stream, 1);
}

int32_t mgs_normal_equations(const mgs_tracking_gn_args* args, const mgs_tracking_depth_args* depth, void* stream) {
  return gauss_newton_impl(args, depth, stream, 0);
}

int32_t mgs_tracking_iteration_second_order(const mgs_tracking_so_args* args, void* stream) {
  return tracking_iteration_so_impl(args, nullptr, stream);
}

int32_t mgs_tracking_iteration_second_order_rgbd(const mgs_tracking_so_args* args, const mgs_tracking_depth_args* depth,
                                                 void* stream) {
  if (!depth_args_ok(depth)) return MGS_ERR_BAD_ARGUMENT;
  return tracking_iteration_so_impl(args, depth, stream);
}

int32_t mgs_profile_enable(int32_t on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  return MGS_OK;
}

int32_t mgs_profile_read(int32_t max_entries, char* names, float* total_ms, int32_t* launches) {
  if (max_entries < 0 || (max_entries > 0 && (!names || !total_ms || !launches)))
    return MGS_ERR_BAD_ARGUMENT;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int n = 0;
  for (ProfRec& r : g_prof) {
    (void)hipEventSynchronize(r.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
    int k = 0;
    for (; k < n; k++)
      if (strncmp(names + 32 * k, r.name, 31) == 0) break;
    if (k == n) {
      if (n >= max_entries) continue;
      strncpy(names + 32 * k, r.name, 31);
      names[32 * k + 31] = 0;
      total_ms[k] = 0.f;
      launches[k] = 0;
      n++;
    }
    total_ms[k] += ms;
    launches[k] += 1;
  }
  g_prof.clear();
  return n;
}

uint64_t mgs_knn_scratch_bytes(int32_t num_points) { return num_points < 1 ? 256 : knn_scratch_bytes(num_points); }

int32_t mgs_knn_dist2(const float* points, int32_t num_points, float* out, void* scratch,
                      void* stream) {
  if (!points || !out || !scratch || num_points < 1) return MGS_ERR_BAD_ARGUMENT;
  return launch_knn(points, num_points, out, scratch, (hipStream_t)stream);
}

}  // extern "C"
