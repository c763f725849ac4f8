// Scoring of a rendered view against its ground truth (utils/eval_utils.py:114-178): PSNR sums over the elements with
// gt > 0 (:150-152) and over all elements (image_utils.py:19-21), the L1 sum, the SSIM sum (loss_utils.py:61-101:
// 11x11 Gaussian window, sigma 1.5, per channel, ZERO padding, C1 = 0.01^2, C2 = 0.03^2) and the depth L1 sum over
// gt_depth > 0 - VALUE only, one launch, one record of a device table, nothing read on the host.
//
// With x = clamp(image, 0, 1) (after the optional exposure (|a| + eps) image + b, rounded as torch rounds it: a
// product, then a sum) and y the ground truth (a uint8 [H,W,3] image is divided by 255 in the tile load, the IEEE
// division the dataset does), one workgroup owns a 32x16 output tile of one channel:
//   stage   u = x - c1, v = y - c2 over the tile +-5 (42x26, zero outside the image); the staging thread of a tile
//           pixel also adds its (x - y)^2, |x - y| and mask terms (channel 0's workgroups: the depth terms of the pixel)
//   pass A  horizontal 11-tap filter of the five moment inputs (u, v, u^2, v^2, uv) over the tile's columns, rows +-5
//   pass B  vertical 11-tap filter -> the five moments at every pixel of the tile -> S, summed
// Both passes are register-blocked (4 columns / 2 rows per thread from one register window); the row strides are odd
// where lanes walk rows (stage -> pass A), pass B walks along rows.  The value needs no partial maps, so the LDS holds
// only the staged pair and the five horizontal planes.
//
// Precision: as k_ssim_loss (ssim_loss.hip) - the passes filter the moments of u, v about the tile-centre values c1, c2
// and recover the raw moments with the window mass W1 = G*1, so bright flat content does not cancel in fp32.
//
// Grid: at most 512 workgroups (two per CU), each walking tiles blockIdx.x, blockIdx.x + gridDim.x, ... with its sums in
// registers.  One workgroup per tile (1800 at 640x480, 4902 at 1200x680) was measured at 49.6 / 145.2 us: every
// workgroup ends in a release fence and a ticket, and without the fence the same grid took 37.5 / 80.6 us.  With the
// tile loop: 256 groups 32.0 / 72.7 us, 384: 28.3 / 62.4, 512: 27.0 / 53.2, 768: 28.3 / 50.5, 1024: 33.4 / 64.0.
//
// Reduction: seven fp32 partial sums per workgroup (sse, sse_all, abs, ssim, depth_abs, n_mask, n_depth; a count grows
// by at most 512 per tile and stays exact below 2^24, i.e. up to 32768 tiles per workgroup, 16 M tiles per image),
// each in a fixed order inside it; the workgroup that takes the last ticket (the int behind the 7 n partials: zero on
// entry, restored here) adds them in index order in double and writes the record.  No float atomics: two identical
// calls give bit-identical records.
//
// Resources, with the flags the library is built with (hipcc -O3 -fno-slp-vectorize --offload-arch=gfx950 -std=c++17,
// -Rpass-analysis=kernel-resource-usage; without -fno-slp-vectorize the same source takes 128 VGPRs and spills 17):
//   k_eval_score: 122 VGPRs (launch bounds ask for 4 waves/SIMD), 0 AGPRs, 0 VGPR spills (8 SGPRs spilled to lanes),
//   26640 B LDS -> 6 workgroups per CU by LDS, 4 by registers: "Occupancy [waves/SIMD]: 4".  k_ssim_loss, which keeps the
//   partial maps for the gradient, has 67200 B and 2.  Measured: profiles/eval_profile.txt.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/monogs_raster.h"
#include "launch.h"

namespace mgs {

namespace evs {
constexpr int kWin = 11, kR = 5;            // window, radius
constexpr int TX = 32, TY = 16;             // output tile
constexpr int kThreads = 256;
constexpr int IX = TX + 2 * kR, IY = TY + 2 * kR;      // staged inputs: tile +-5 (42 x 26)
constexpr int IXS = IX + 1;                 // odd row strides where lanes walk rows
constexpr int HXS = TX + 1;
constexpr int kIn = IY * IXS;               // one staged image
constexpr int kH = IY * HXS;                // one horizontal moment plane
constexpr int kLds = 2 * kIn + 5 * kH;      // floats
constexpr int RA = 4, NA = TX / RA;         // pass A: 4 columns per item, 8 runs per row
constexpr int RB = 2;                       // pass B: 2 rows per item
constexpr int kSums = 7;                    // partial sums per workgroup
constexpr int kMaxGroups = 512;             // workgroups of a launch (two per CU); each walks tiles in a grid-stride loop
constexpr int kStage = (IX * IY + kThreads - 1) / kThreads;      // staged items per thread
static_assert(NA * IY <= kThreads, "pass A: one round");
static_assert((TY / RB) * TX == kThreads, "pass B: one item per thread");
static_assert(4 * (kLds + 64) * (int)sizeof(float) <= 160 * 1024, "at least four workgroups per CU by LDS");

struct Weights { float g[kWin]; };

__global__ __launch_bounds__(kThreads, 4) void k_eval_score(mgs_eval_score_args A, Weights Wt) {
  __shared__ float smem[kLds];
  __shared__ float s_red[kSums][kThreads / 64];
  __shared__ float sWx[TX], sWy[TY];          // 1-D window mass over the image, per tile column / row
  float* sX = smem;
  float* sY = sX + kIn;
  float* sH = sY + kIn;                       // 5 planes [IY][HXS]: u, v, u^2, v^2, uv
  const int W = A.width, H = A.height;
  const size_t plane = (size_t)W * H;
  const int tid = threadIdx.x;
  float g[kWin];
#pragma unroll
  for (int k = 0; k < kWin; k++) g[k] = Wt.g[k];
  const bool expo = A.apply_exposure != 0;
  const float ea = expo ? __fadd_rn(fabsf(A.exposure_a[0]), A.exposure_eps) : 1.f;
  const float eb = expo ? A.exposure_b[0] : 0.f;
  const bool u8 = A.gt_format == MGS_EVAL_GT_U8_HWC;
  const int tiles_x = (W + TX - 1) / TX, tiles_xy = tiles_x * ((H + TY - 1) / TY);
  float sse = 0.f, sse_all = 0.f, abs_sum = 0.f, n_mask = 0.f, d_sum = 0.f, n_depth = 0.f, s_sum = 0.f;
  // a workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... (channel-major) and keeps its sums in registers
  for (int tile = blockIdx.x; tile < 3 * tiles_xy; tile += gridDim.x) {
    const int c = tile / tiles_xy, ty = (tile - c * tiles_xy) / tiles_x;
    const int x0 = (tile - c * tiles_xy - ty * tiles_x) * TX, y0 = ty * TY;
    const float* img = A.image + c * plane;
    const float* gtf = (const float*)A.gt + c * plane;
    const unsigned char* gtb = (const unsigned char*)A.gt + c;
    auto load_x = [&](size_t o) {
      float v = img[o];
      if (expo) v = __fadd_rn(__fmul_rn(ea, v), eb);
      return fminf(fmaxf(v, 0.f), 1.f);
    };
    auto load_y = [&](size_t o) { return u8 ? __fdiv_rn((float)gtb[3 * o], 255.f) : gtf[o]; };
    // the shift: values at the tile centre (clamped into the image; the same for every thread)
    const size_t oc = (size_t)min(y0 + TY / 2, H - 1) * W + min(x0 + TX / 2, W - 1);
    const float c1 = load_x(oc), c2 = load_y(oc);
    const bool with_depth = c == 0 && A.depth != nullptr;

    // ---- stage u = x - c1, v = y - c2 over the tile +-5, zero outside the image; the element sums; the window masses
    // Every load of a thread is issued before the first is used: the addresses are clamped into the image (and the item
    // into the staged region), so the loads need no branch and their latencies overlap; the flags select afterwards.
    float xs[kStage], ys[kStage], ds[kStage], gs[kStage];
#pragma unroll
    for (int rd = 0; rd < kStage; rd++) {
      const int i = min(tid + rd * kThreads, IX * IY - 1);
      const int r = i / IX, q = i - r * IX;
      const size_t o = (size_t)min(max(y0 - kR + r, 0), H - 1) * W + min(max(x0 - kR + q, 0), W - 1);
      xs[rd] = load_x(o);
      ys[rd] = load_y(o);
      ds[rd] = with_depth ? A.depth[o] : 0.f;
      gs[rd] = with_depth ? A.gt_depth[o] : 0.f;
    }
#pragma unroll
    for (int rd = 0; rd < kStage; rd++) {
      const int i = tid + rd * kThreads;
      if (i < IX * IY) {
        const int r = i / IX, q = i - r * IX;
        const int gx = x0 - kR + q, gy = y0 - kR + r;
        const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const float xv = xs[rd], yv = ys[rd];
        if (inside && q >= kR && q < kR + TX && r >= kR && r < kR + TY) {   // a pixel of this tile
          const float d = xv - yv, d2 = d * d;
          sse_all += d2;
          abs_sum += fabsf(d);
          if (yv > 0.f) { sse += d2; n_mask += 1.f; }
          if (gs[rd] > 0.f) { d_sum += fabsf(ds[rd] - gs[rd]); n_depth += 1.f; }
        }
        sX[r * IXS + q] = inside ? xv - c1 : 0.f;
        sY[r * IXS + q] = inside ? yv - c2 : 0.f;
      }
    }
    if (tid < TX + TY) {
      const bool is_col = tid < TX;
      const int j = is_col ? tid : tid - TX;
      const int base = (is_col ? x0 : y0) - kR + j, n = is_col ? W : H;
      float m = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; k++) m += (base + k >= 0 && base + k < n) ? g[k] : 0.f;
      (is_col ? sWx : sWy)[j] = m;
    }
    __syncthreads();

    // ---- pass A: horizontal moments over rows [0, IY) x tile columns [0, TX) (input column = tile column + k)
    if (tid < NA * IY) {
      const int r = tid % IY, c0 = (tid / IY) * RA;      // lanes walk rows (odd stride)
      float wx[RA + kWin - 1], wy[RA + kWin - 1];
#pragma unroll
      for (int k = 0; k < RA + kWin - 1; k++) {
        wx[k] = sX[r * IXS + c0 + k];
        wy[k] = sY[r * IXS + c0 + k];
      }
#pragma unroll
      for (int j = 0; j < RA; j++) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; k++) {
          const float xv = wx[j + k], yv = wy[j + k];
          a0 = fmaf(g[k], xv, a0);
          a1 = fmaf(g[k], yv, a1);
          a2 = fmaf(g[k], xv * xv, a2);
          a3 = fmaf(g[k], yv * yv, a3);
          a4 = fmaf(g[k], xv * yv, a4);
        }
        const int o = r * HXS + c0 + j;
        sH[o] = a0; sH[kH + o] = a1; sH[2 * kH + o] = a2; sH[3 * kH + o] = a3; sH[4 * kH + o] = a4;
      }
    }
    __syncthreads();

    // ---- pass B: vertical moments at the tile's pixels; S summed over those inside the image
    constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    {
      const int col = tid % TX, r0 = (tid / TX) * RB;    // lanes walk columns
      float m[5][RB];
#pragma unroll
      for (int t = 0; t < 5; t++) {
        float w[RB + kWin - 1];
#pragma unroll
        for (int k = 0; k < RB + kWin - 1; k++) w[k] = sH[t * kH + (r0 + k) * HXS + col];
#pragma unroll
        for (int j = 0; j < RB; j++) {
          float a = 0.f;
#pragma unroll
          for (int k = 0; k < kWin; k++) a = fmaf(g[k], w[j + k], a);
          m[t][j] = a;
        }
      }
      const float wxm = sWx[col];
#pragma unroll
      for (int j = 0; j < RB; j++) {
        const float W1 = wxm * sWy[r0 + j], w1c = 1.f - W1;
        const float mu_u = m[0][j], mu_v = m[1][j];
        const float mu1 = fmaf(c1, -w1c, mu_u) + c1, mu2 = fmaf(c2, -w1c, mu_v) + c2;
        const float s11 = m[2][j] - mu_u * mu_u + w1c * c1 * (2.f * mu_u + c1 * W1);
        const float s22 = m[3][j] - mu_v * mu_v + w1c * c2 * (2.f * mu_v + c2 * W1);
        const float s12 = m[4][j] - mu_u * mu_v + w1c * (c1 * mu_v + c2 * mu_u + c1 * c2 * W1);
        const float A1 = 2.f * mu1 * mu2 + C1, A2 = 2.f * s12 + C2;
        const float iB1 = 1.f / (mu1 * mu1 + mu2 * mu2 + C1), iB2 = 1.f / (s11 + s22 + C2);
        const float S = A1 * A2 * (iB1 * iB2);
        if (x0 + col < W && y0 + r0 + j < H) s_sum += S;
      }
    }
    __syncthreads();     // the planes are read: the next tile may be staged
  }

  // ---- per-workgroup partials, then the last workgroup's fixed-order sum
  // fixed order: butterfly inside the wave, then the wave totals in wave order - one barrier for all seven
  float tot[kSums];
  tot[MGS_EVAL_SSE] = sse; tot[MGS_EVAL_SSE_ALL] = sse_all; tot[MGS_EVAL_ABS] = abs_sum; tot[MGS_EVAL_SSIM] = s_sum;
  tot[MGS_EVAL_DEPTH_ABS] = d_sum; tot[MGS_EVAL_N_MASK] = n_mask; tot[MGS_EVAL_N_DEPTH] = n_depth;
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    for (int off = 32; off > 0; off >>= 1) tot[k] += __shfl_xor(tot[k], off);
    if ((tid & 63) == 0) s_red[k][tid >> 6] = tot[k];
  }
  __syncthreads();
  const int n = gridDim.x, blk = blockIdx.x;
  __shared__ int s_last;
  if (tid == 0) {   // write-through stores, then the ticket (as k_ssim_loss)
#pragma unroll
    for (int k = 0; k < kSums; k++) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < kThreads / 64; w++) t += s_red[k][w];
      __hip_atomic_store(&A.partial[(size_t)k * n + blk], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();
    int* ticket = reinterpret_cast<int*>(A.partial + (size_t)kSums * n);
    s_last = atomicAdd(ticket, 1) == n - 1;
    if (s_last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  // fixed order whatever workgroup is last: thread t sums partials t, t + 256, ... then the block sum
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; k++) acc[k] = 0.0;
  for (int i = tid; i < n; i += kThreads) {
#pragma unroll
    for (int k = 0; k < kSums; k++)
      acc[k] += (double)__hip_atomic_load(&A.partial[(size_t)k * n + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __shared__ double s_dred[kSums][kThreads / 64];
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
    if ((tid & 63) == 0) s_dred[k][tid >> 6] = acc[k];
  }
  __syncthreads();
  if (tid <= kSums) {
    double* rec = A.table + (size_t)A.row * MGS_EVAL_RECORD_DOUBLES;
    if (tid < kSums) {
      double s = 0.0;
      for (int w = 0; w < kThreads / 64; w++) s += s_dred[tid][w];
      rec[tid] = s;
    } else {
      rec[MGS_EVAL_PAIRS] = A.pair_count ? (double)A.pair_count[0] : 0.0;
    }
  }
}

static Weights weights() {
  // loss_utils.py:42-51: exp(-(x - 5)^2 / (2 sigma^2)) in double, stored as fp32, normalised in fp32
  Weights w;
  float sum = 0.f;
  for (int k = 0; k < kWin; k++) {
    w.g[k] = (float)exp(-(double)((k - kR) * (k - kR)) / (2.0 * 1.5 * 1.5));
    sum += w.g[k];
  }
  for (int k = 0; k < kWin; k++) w.g[k] = w.g[k] / sum;
  return w;
}

static int64_t tiles_of(int32_t H, int32_t W) { return 3 * (((int64_t)W + TX - 1) / TX) * (((int64_t)H + TY - 1) / TY); }
static int groups_of(int32_t H, int32_t W) { return (int)std::min<int64_t>(tiles_of(H, W), kMaxGroups); }

static int32_t score_status(const mgs_eval_score_args* a) {
  if (!a || !a->image || !a->gt || !a->partial || !a->table) return MGS_ERR_BAD_ARGUMENT;
  if ((a->depth == nullptr) != (a->gt_depth == nullptr)) return MGS_ERR_BAD_ARGUMENT;
  if (a->apply_exposure && (!a->exposure_a || !a->exposure_b)) return MGS_ERR_BAD_ARGUMENT;
  if (a->gt_format != MGS_EVAL_GT_F32_CHW && a->gt_format != MGS_EVAL_GT_U8_HWC) return MGS_ERR_BAD_ARGUMENT;
  if (a->row < 0 || a->row >= a->num_rows) return MGS_ERR_BAD_ARGUMENT;
  if (a->height < 1 || a->width < 1) return MGS_ERR_BAD_ARGUMENT;
  if (mgs_eval_score_partial_count(a->height, a->width) < 0) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}
}  // namespace evs

}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_eval_score_args_size(void) { return (int32_t)sizeof(mgs_eval_score_args); }
int32_t mgs_eval_view_args_size(void) { return (int32_t)sizeof(mgs_eval_view_args); }

int32_t mgs_eval_score_partial_count(int32_t height, int32_t width) {
  if (height < 1 || width < 1 || evs::tiles_of(height, width) > 0x7fffffff - evs::kMaxGroups) return -1;   // int tile index
  return (int32_t)(evs::kSums * evs::groups_of(height, width) + 1);
}

int32_t mgs_eval_score(const mgs_eval_score_args* a, void* stream) {
  const int32_t rc = evs::score_status(a);
  if (rc != MGS_OK) return rc;
  static const evs::Weights w = evs::weights();
  launch("eval_score", evs::k_eval_score, dim3((unsigned)evs::groups_of(a->height, a->width)), dim3(evs::kThreads),
         (hipStream_t)stream, *a, w);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_eval_view(const mgs_eval_view_args* args, void* stream) {
  if (!args || !args->T || !args->fwd.viewmatrix || !args->fwd.projmatrix || !args->fwd.projmatrix_raw || !args->fwd.geom ||
      !args->fwd.out_color || !args->fwd.out_depth || !args->fwd.out_opacity || !args->fwd.radii || !args->fwd.n_touched ||
      !args->fwd.bins || !args->fwd.means3D || !args->fwd.opacities || !args->fwd.campos || !args->fwd.bg ||
      (!args->fwd.cov3D_precomp && (!args->fwd.scales || !args->fwd.rotations)) ||
      (!args->fwd.shs && !args->fwd.colors_precomp) || args->fwd.shape.pair_capacity < 1)
    return MGS_ERR_BAD_ARGUMENT;
  if (args->score.height != args->fwd.shape.height || args->score.width != args->fwd.shape.width) return MGS_ERR_BAD_ARGUMENT;
  mgs_workspace_sizes ws;
  int32_t rc = mgs_raster_workspace_query(&args->fwd.shape, &ws);
  if (rc != MGS_OK) return rc;
  mgs_eval_score_args S = args->score;
  S.image = args->fwd.out_color;
  S.depth = S.gt_depth ? args->fwd.out_depth : nullptr;
  S.pair_count = (const int32_t*)((const char*)args->fwd.geom + ws.off_counters);
  if ((rc = evs::score_status(&S)) != MGS_OK) return rc;       // before the first launch
  if (!args->camera_matrices_valid) {
    rc = mgs_camera_from_pose(args->T, args->fwd.projmatrix_raw, const_cast<float*>(args->fwd.viewmatrix),
                              const_cast<float*>(args->fwd.projmatrix), stream);
    if (rc != MGS_OK) return rc;
  }
  if ((rc = mgs_raster_forward_project(&args->fwd, stream)) != MGS_OK) return rc;
  if ((rc = mgs_raster_forward_blend(&args->fwd, stream)) != MGS_OK) return rc;
  return mgs_eval_score(&S, stream);
}

}  // extern "C"
