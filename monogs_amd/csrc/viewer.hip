// Headless viewer: the last step from the forward's float planes to a finished uint8 [H,W,3] frame (what the
// reference's GUI does on the host: gui/slam_gui.py:544-653, gui/gui_utils.py:24-66, gl_render/shaders/gau_frag.glsl).
//
//   k_view_max / k_view_compose         float planes -> interleaved uint8: clamp * 255, or a 256-entry colour map of
//                                       (v - lo) / (max - lo); the maximum is a launch of its own (<= 64 block partials,
//                                       summed up again by every compose workgroup: no atomics, no host read)
//   k_view_first_hit                    the ellipsoid shader: nearest splat whose alpha exceeds a threshold, walked
//                                       front to back over the forward's per-tile sorted keys by one wave per 8x8 quadrant
//   k_view_id_range / k_view_time_colors  the time shader's tinted SH coefficients
//   k_view_overlay_project / _draw      frusta and free segments as 1-pixel lines: fp32 projection and clipping to
//                                       1/16-pixel integers, then integer-only stepping, highest segment index on top
//
// Every arithmetic step the torch mirror (monogs_amd/viewer.py) repeats bit for bit is a single rounding: rn_math.h for
// products, sums and differences, __fdiv_rn for quotients.
//
// Work-item shapes.  Compose: a thread owns FOUR consecutive pixels of the flat [H*W] order, i.e. 12 output bytes at a
// 4-byte aligned offset - three dword stores; its loads are float4 where the plane offset is 16-byte aligned (always for
// a single plane, for the colour planes when H*W is a multiple of 4) and scalar otherwise; only the last H*W mod 4
// pixels of the image take byte stores.  First hit: the quadrant wave of k_blend_fwd - 64 lanes hold the
// 8x8 pixels of a quadrant, stage 64 records at a time in LDS (3 KB per wave), walk the reachable ones by ballot mask and
// leave at the first splat after which no lane is still open.  Overlay: one thread per segment projects, one wave per
// segment draws (lane l takes steps l, l + 64, ...).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "raster_kernels.h"
#include "rn_math.h"

namespace mgs {

namespace vw {
constexpr int kThreads = 256;
constexpr int kRedBlocks = 64;          // workgroups of the two reduction launches: their partials fit one wave
constexpr float kDepthLo = 0.1f;        // slam_gui.py:582-584: min_value of the depth colour map
constexpr float kThrFlat = 0.22f, kThrGauss = 0.4f;   // gau_frag.glsl:30,33

__device__ __forceinline__ int lut_index(float t) {      // t is not NaN
  t = fminf(fmaxf(t, 0.f), 1.f);
  return min(255, (int)mul_rn(t, 256.f));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// ---- (a) compose -----------------------------------------------------------------------------------------------------
// Largest non-negative value of the plane (fmaxf passes over NaNs): one partial per workgroup.
__global__ __launch_bounds__(kThreads) void k_view_max(const float* __restrict__ src, int n, float* __restrict__ partial) {
  __shared__ float s_m[kThreads / 64];
  float m = 0.f;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) m = fmaxf(m, src[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; w++) m = fmaxf(m, s_m[w]);
    partial[blockIdx.x] = m;
  }
}

// four consecutive values of one plane: one 16-byte load where the address allows it
__device__ __forceinline__ void load4(const float* __restrict__ p, int cnt, float v[4]) {
  if (cnt == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = j < cnt ? p[j] : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void k_view_compose(mgs_view_compose_args A, int nblk) {
  __shared__ unsigned char s_lut[768];
  __shared__ float s_mx;
  const int tid = threadIdx.x;
  const int HW = A.width * A.height;
  const bool rgb = A.mode == MGS_VIEW_RGB;
  if (!rgb) {
    for (int i = tid; i < 768; i += kThreads) s_lut[i] = A.lut[i];
    if (tid < 64) {
      const float m = wave_max(tid < nblk ? reinterpret_cast<const float*>(A.scratch)[tid] : 0.f);
      if (tid == 0) s_mx = m;
    }
    __syncthreads();
  }
  const int p0 = 4 * (blockIdx.x * kThreads + tid);
  if (p0 >= HW) return;
  const int cnt = min(4, HW - p0);
  unsigned char b[12];
  if (rgb) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float v[4];
      load4(A.src + (size_t)c * HW + p0, cnt, v);
#pragma unroll
      for (int j = 0; j < 4; j++)       // fmaxf(NaN, 0) = 0: a NaN is black
        b[3 * j + c] = (unsigned char)(int)mul_rn(fminf(fmaxf(v[j], 0.f), 1.f), 255.f);
    }
  } else {
    const float lo = A.mode == MGS_VIEW_DEPTH ? kDepthLo : 0.f;
    const float mx = s_mx;
    const bool flat = !(mx > lo);
    const float den = sub_rn(mx, lo);
    float v[4];
    load4(A.src + p0, cnt, v);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float t = flat ? (v[j] != v[j] ? v[j] : 0.f) : __fdiv_rn(sub_rn(v[j], lo), den);
      const bool nan = t != t;
      const int i = 3 * lut_index(nan ? 0.f : t);
#pragma unroll
      for (int c = 0; c < 3; c++) b[3 * j + c] = nan ? (unsigned char)0 : s_lut[i + c];
    }
  }
  unsigned char* o = A.out + 3 * (size_t)p0;
  if (cnt == 4) {
    unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
#pragma unroll
    for (int d = 0; d < 3; d++)
      o4[d] = (unsigned int)b[4 * d] | ((unsigned int)b[4 * d + 1] << 8) | ((unsigned int)b[4 * d + 2] << 16) |
              ((unsigned int)b[4 * d + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 9; j++)                          // the last H*W mod 4 pixels of the image
      if (j < 3 * cnt) o[j] = b[j];
  }
}

// ---- (b) first hit ---------------------------------------------------------------------------------------------------
template <bool GAUSS>
__global__ __launch_bounds__(64) void k_view_first_hit(KP P, float thr, float* __restrict__ hit_color,
                                                       float* __restrict__ hit_depth) {
  // per staged splat 48 B: (x, y, A, B) (C, opacity, depth, -) (r, g, b, -)
  __shared__ float4 s_rec[kSeg * 3];
  const int item = xcd_remap<4>(blockIdx.x);
  if (item >= 4 * P.T) return;
  const int tile = item >> 2, quad = item & 3, lane = threadIdx.x;
  const int tx = tile % P.grid_x, ty = tile / P.grid_x;
  const int qx0 = tx * kTile + 8 * (quad & 1), qy0 = ty * kTile + 8 * (quad >> 1);
  if (qx0 >= P.W || qy0 >= P.H) return;
  const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
  const bool inside = px < P.W && py < P.H;
  const float fpx = (float)px, fpy = (float)py;
  int start = P.tile_offset[tile], end = P.tile_offset[tile + 1];
  start = min(start, P.cap); end = min(end, P.cap);
  const int n = end - start;
  const float bx0 = (float)qx0, by0 = (float)qy0;
  const float bx1 = fminf(bx0 + 7.f, (float)(P.W - 1)), by1 = fminf(by0 + 7.f, (float)(P.H - 1));
  bool open = inside;                     // no hit yet
  float h0 = P.bg[0], h1 = P.bg[1], h2 = P.bg[2], hd = 0.f;
  const unsigned int* key_lo = reinterpret_cast<const unsigned int*>(P.keys + start);
  for (int base = 0; base < n; base += kSeg) {
    const int k = base + lane;
    unsigned int id = k < n ? key_lo[2 * (size_t)k] : 0u;     // low key word = Gaussian id (<< kPackBits | pair index)
    if (P.pack) id >>= kPackBits;
    const float4* src = reinterpret_cast<const float4*>(P.rec + id);
    const float4 ra = src[0], rb = src[1], rc = src[2];       // (x, y, depth, o) (A, B, C, radius) (r, g, b, flags)
    // a hit needs o exp(power) > thr, i.e. the quadratic form below 2 ln(o / thr): the blend's conservative box test
    // with that bound drops the splats that cannot hit any pixel of this quadrant
    const bool reach = k < n && box_reachable(ra.x, ra.y, rb.x, rb.y, rb.z, 2.0f * logf(ra.w / thr), bx0, by0, bx1, by1);
    unsigned long long m = __builtin_amdgcn_ballot_w64(reach);
    if (m != 0ull) {
      __syncthreads();   // single-wave workgroup: orders the LDS traffic
      if (reach) {
        s_rec[3 * lane] = make_float4(ra.x, ra.y, rb.x, rb.y);
        s_rec[3 * lane + 1] = make_float4(rb.z, ra.w, ra.z, 0.f);
        s_rec[3 * lane + 2] = make_float4(rc.x, rc.y, rc.z, 0.f);
      }
      __syncthreads();
      while (m != 0ull) {
        const int j = __builtin_ctzll(m);
        m &= m - 1ull;
        const float4 u = s_rec[3 * j], v = s_rec[3 * j + 1], c = s_rec[3 * j + 2];
        const float dx = u.x - fpx, dy = u.y - fpy;
        const float power = -0.5f * (u.z * dx * dx + v.x * dy * dy) - u.w * dx * dy;
        const float G = __builtin_amdgcn_exp2f(power * 1.4426950408889634f);
        const float a = fminf(kAlphaMax, v.y * G);
        if (open && power <= 0.f && a >= kAlphaMin && a > thr) {
          h0 = GAUSS ? c.x * G : c.x; h1 = GAUSS ? c.y * G : c.y; h2 = GAUSS ? c.z * G : c.z;
          hd = v.z;
          open = false;
        }
        if (__builtin_amdgcn_ballot_w64(open) == 0ull) break;   // every pixel of the quadrant has its hit
      }
    }
    if (__builtin_amdgcn_ballot_w64(open) == 0ull) break;
  }
  if (inside) {
    const size_t HW = (size_t)P.W * P.H, pix = (size_t)py * P.W + px;
    hit_color[pix] = h0; hit_color[HW + pix] = h1; hit_color[2 * HW + pix] = h2;
    hit_depth[pix] = hd;
  }
}

// ---- (c) time shader -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_view_id_range(const int* __restrict__ ids, int n, int2* __restrict__ partial) {
  __shared__ int s_lo[kThreads / 64], s_hi[kThreads / 64];
  int lo = 0x7fffffff, hi = (int)0x80000000;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const int v = ids[i];
    lo = min(lo, v); hi = max(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_xor(lo, off)); hi = max(hi, __shfl_xor(hi, off)); }
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; w++) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
    partial[blockIdx.x] = make_int2(lo, hi);
  }
}

// one thread per coefficient: element e of [N,K,3] belongs to Gaussian e / (3 K), channel e % 3
__global__ __launch_bounds__(kThreads) void k_view_time_colors(mgs_view_time_colors_args A, int nblk) {
  __shared__ unsigned char s_lut[768];
  __shared__ int s_range[2];
  const int tid = threadIdx.x;
  for (int i = tid; i < 768; i += kThreads) s_lut[i] = A.lut[i];
  if (tid < 64) {
    int2 r = tid < nblk ? reinterpret_cast<const int2*>(A.scratch)[tid] : make_int2(0x7fffffff, (int)0x80000000);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { r.x = min(r.x, __shfl_xor(r.x, off)); r.y = max(r.y, __shfl_xor(r.y, off)); }
    if (tid == 0) { s_range[0] = r.x; s_range[1] = r.y; }
  }
  __syncthreads();
  const int e = blockIdx.x * kThreads + tid;
  const int row = 3 * A.sh_coeffs;
  if (e >= A.num_gaussians * row) return;
  const int g = e / row, c = e % 3;
  const long long span = (long long)s_range[1] - s_range[0];
  const float t = span > 0 ? __fdiv_rn((float)((long long)A.kf_ids[g] - s_range[0]), (float)span) : 0.f;
  const float tint = mul_rn(0.9f, __fdiv_rn((float)s_lut[3 * lut_index(t) + c], 255.f));
  A.out[e] = add_rn(mul_rn(0.1f, A.features[e]), tint);
}

// ---- (d) overlay -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool clip_edge(float p, float q, float& t0, float& t1) {     // Liang-Barsky
  if (p == 0.f) return q >= 0.f;
  const float r = q / p;
  if (p < 0.f) {
    if (r > t1) return false;
    if (r > t0) t0 = r;
  } else {
    if (r < t0) return false;
    if (r < t1) t1 = r;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void k_view_overlay_project(mgs_view_overlay_args A, int S) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= S) return;
  float w[2][3];
  if (s < 8 * A.num_poses) {
    const int pose = s >> 3, line = s & 7;
    const int e0 = line < 4 ? 0 : (line < 6 ? 1 : line - 4);                 // 0-1 0-2 0-3 0-4 1-2 1-3 2-4 3-4
    const int e1 = line < 4 ? line + 1 : (line == 4 ? 2 : (line == 5 ? 3 : 4));
    const float* Pm = A.poses + 16 * (size_t)pose;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int j = q ? e1 : e0;
      // (0,0,0), (1,-.5,2), (-1,-.5,2), (1,.5,2), (-1,.5,2) times size
      const float cx = j == 0 ? 0.f : ((j & 1) ? A.frustum_size : -A.frustum_size);
      const float cy = j == 0 ? 0.f : (j <= 2 ? -0.5f * A.frustum_size : 0.5f * A.frustum_size);
      const float cz = j == 0 ? 0.f : 2.f * A.frustum_size;
#pragma unroll
      for (int i = 0; i < 3; i++) w[q][i] = Pm[4 * i] * cx + Pm[4 * i + 1] * cy + Pm[4 * i + 2] * cz + Pm[4 * i + 3];
    }
  } else {
    const float* f = A.free_segments + 6 * (size_t)(s - 8 * A.num_poses);
#pragma unroll
    for (int i = 0; i < 3; i++) { w[0][i] = f[i]; w[1][i] = f[3 + i]; }
  }
  float v[2][3];
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int i = 0; i < 3; i++)
      v[q][i] = A.T_view[4 * i] * w[q][0] + A.T_view[4 * i + 1] * w[q][1] + A.T_view[4 * i + 2] * w[q][2] + A.T_view[4 * i + 3];
  int* out = A.endpoints + 5 * (size_t)s;
  bool valid = !(v[0][2] < A.near_z && v[1][2] < A.near_z);
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int i = 0; i < 3; i++) valid = valid && fabsf(v[q][i]) <= 3.0e38f;      // false for NaN and inf
  float x[2] = {0.f, 0.f}, y[2] = {0.f, 0.f};
  if (valid) {
#pragma unroll
    for (int q = 0; q < 2; q++) {      // the end point behind the near plane moves onto it
      if (v[q][2] < A.near_z) {
        const float t = (A.near_z - v[q][2]) / (v[1 - q][2] - v[q][2]);
        v[q][0] += t * (v[1 - q][0] - v[q][0]);
        v[q][1] += t * (v[1 - q][1] - v[q][1]);
        v[q][2] = A.near_z;
      }
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      x[q] = A.fx * v[q][0] / v[q][2] + A.cx;
      y[q] = A.fy * v[q][1] / v[q][2] + A.cy;
    }
    const float xmin = -0.5f * A.width, xmax = 1.5f * A.width, ymin = -0.5f * A.height, ymax = 1.5f * A.height;
    const float dx = x[1] - x[0], dy = y[1] - y[0];
    float t0 = 0.f, t1 = 1.f;
    valid = clip_edge(-dx, x[0] - xmin, t0, t1) && clip_edge(dx, xmax - x[0], t0, t1) &&
            clip_edge(-dy, y[0] - ymin, t0, t1) && clip_edge(dy, ymax - y[0], t0, t1);
    if (valid) {
      if (t1 < 1.f) { x[1] = x[0] + t1 * dx; y[1] = y[0] + t1 * dy; }
      if (t0 > 0.f) { x[0] = x[0] + t0 * dx; y[0] = y[0] + t0 * dy; }
      valid = fabsf(x[0]) <= 1.0e8f && fabsf(y[0]) <= 1.0e8f && fabsf(x[1]) <= 1.0e8f && fabsf(y[1]) <= 1.0e8f;
    }
  }
  out[0] = valid ? __float2int_rn(16.f * x[0]) : 0;
  out[1] = valid ? __float2int_rn(16.f * y[0]) : 0;
  out[2] = valid ? __float2int_rn(16.f * x[1]) : 0;
  out[3] = valid ? __float2int_rn(16.f * y[1]) : 0;
  out[4] = valid ? 1 : 0;
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {     // b > 0
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// PASS 0: owner[pixel] = max(owner, segment); PASS 1: the owner writes its colour
template <int PASS>
__global__ __launch_bounds__(64) void k_view_overlay_draw(mgs_view_overlay_args A) {
  const int s = blockIdx.x;
  const int* e = A.endpoints + 5 * (size_t)s;
  if (e[4] == 0) return;
  const long long X0 = e[0], Y0 = e[1], dx = (long long)e[2] - e[0], dy = (long long)e[3] - e[1];
  const long long mlen = max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy);
  const long long n = (mlen + 15) >> 4;
  if (n > 2ll * (A.width + A.height)) return;      // never taken: the project step's guard rectangle keeps n <= 2 max(W, H)
  int* owner = reinterpret_cast<int*>(A.scratch);
  const unsigned char* col = s < 8 * A.num_poses ? A.pose_colors + 3 * (size_t)(s >> 3)
                                                 : A.free_colors + 3 * (size_t)(s - 8 * A.num_poses);
  for (long long k = threadIdx.x; k <= n; k += 64) {
    const long long ox = n > 0 ? floor_div(2 * dx * k + n, 2 * n) : 0;
    const long long oy = n > 0 ? floor_div(2 * dy * k + n, 2 * n) : 0;
    const long long px = (X0 + ox + 8) >> 4, py = (Y0 + oy + 8) >> 4;
    if (px < 0 || px >= A.width || py < 0 || py >= A.height) continue;
    const size_t pix = (size_t)py * A.width + (size_t)px;
    if (PASS == 0) {
      atomicMax(&owner[pix], s);
    } else if (owner[pix] == s) {
      unsigned char* o = A.frame + 3 * pix;
      o[0] = col[0]; o[1] = col[1]; o[2] = col[2];
    }
  }
}

static int red_blocks(long long n) { return (int)std::min<long long>((n + kThreads - 1) / kThreads, kRedBlocks); }

static int32_t overlay_status(const mgs_view_overlay_args* a) {
  if (!a || a->width < 1 || a->height < 1 || a->num_poses < 0 || a->num_free < 0) return MGS_ERR_BAD_ARGUMENT;
  if (!a->endpoints || !a->frame || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  if ((a->num_poses > 0 && !a->pose_colors) || (a->num_free > 0 && !a->free_colors)) return MGS_ERR_BAD_ARGUMENT;
  if (!a->T_view || (a->num_poses > 0 && !a->poses) || (a->num_free > 0 && !a->free_segments) || !(a->near_z > 0.f))
    return MGS_ERR_BAD_ARGUMENT;
  if (mgs_view_overlay_scratch_bytes(a->width, a->height) == 0) return MGS_ERR_UNSUPPORTED;
  if (8ll * a->num_poses + a->num_free > (1 << 24)) return MGS_ERR_UNSUPPORTED;      // one workgroup per segment
  return MGS_OK;
}

static int32_t overlay_draw(const mgs_view_overlay_args* a, int S, hipStream_t st) {
  if (!hip_ok("memset(overlay owners)", hipMemsetAsync(a->scratch, 0xff, sizeof(int) * (size_t)a->width * a->height, st))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  launch("view_overlay_draw", k_view_overlay_draw<0>, dim3(S), dim3(64), st, *a);
  launch("view_overlay_draw", k_view_overlay_draw<1>, dim3(S), dim3(64), st, *a);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}
}  // namespace vw

int launch_view_first_hit(const KP& P, int mode, float* hit_color, float* hit_depth, hipStream_t st) {
  const dim3 grid(grid_pad(4 * P.T, 4));
  if (mode == MGS_VIEW_GAUSSIAN_BALL)
    launch("view_first_hit", vw::k_view_first_hit<true>, grid, dim3(64), st, P, vw::kThrGauss, hit_color, hit_depth);
  else
    launch("view_first_hit", vw::k_view_first_hit<false>, grid, dim3(64), st, P, vw::kThrFlat, hit_color, hit_depth);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_view_compose_args_size(void) { return (int32_t)sizeof(mgs_view_compose_args); }
int32_t mgs_view_time_colors_args_size(void) { return (int32_t)sizeof(mgs_view_time_colors_args); }
int32_t mgs_view_overlay_args_size(void) { return (int32_t)sizeof(mgs_view_overlay_args); }

uint64_t mgs_view_compose_scratch_bytes(void) { return sizeof(float) * vw::kRedBlocks; }
uint64_t mgs_view_time_colors_scratch_bytes(void) { return sizeof(int2) * vw::kRedBlocks; }
uint64_t mgs_view_overlay_scratch_bytes(int32_t width, int32_t height) {
  if (width < 1 || height < 1 || (int64_t)width * height * 3 > 0x7fffffff) return 0;
  return sizeof(int32_t) * (uint64_t)width * (uint64_t)height;
}

int32_t mgs_view_compose(const mgs_view_compose_args* a, void* stream) {
  if (!a || a->width < 1 || a->height < 1 || !a->src || !a->out) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode != MGS_VIEW_RGB && a->mode != MGS_VIEW_DEPTH && a->mode != MGS_VIEW_OPACITY) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode != MGS_VIEW_RGB && (!a->lut || !a->scratch)) return MGS_ERR_BAD_ARGUMENT;
  if ((int64_t)a->width * a->height * 3 > 0x7fffffff) return MGS_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(a->out) & 3) return MGS_ERR_UNSUPPORTED;             // dword stores
  const int HW = a->width * a->height;
  hipStream_t st = (hipStream_t)stream;
  int nblk = 0;
  if (a->mode != MGS_VIEW_RGB) {
    nblk = vw::red_blocks(HW);
    launch("view_max", vw::k_view_max, dim3(nblk), dim3(vw::kThreads), st, a->src, HW, reinterpret_cast<float*>(a->scratch));
  }
  const int groups = (HW + 3) / 4;
  launch("view_compose", vw::k_view_compose, dim3((groups + vw::kThreads - 1) / vw::kThreads), dim3(vw::kThreads), st, *a, nblk);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_view_time_colors(const mgs_view_time_colors_args* a, void* stream) {
  if (!a || a->num_gaussians < 1 || a->sh_coeffs < 1 || !a->features || !a->kf_ids || !a->lut || !a->out || !a->scratch)
    return MGS_ERR_BAD_ARGUMENT;
  const int64_t elems = (int64_t)a->num_gaussians * a->sh_coeffs * 3;
  if (elems > 0x7fffffff - vw::kThreads) return MGS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = vw::red_blocks(a->num_gaussians);
  launch("view_id_range", vw::k_view_id_range, dim3(nblk), dim3(vw::kThreads), st, a->kf_ids, a->num_gaussians,
         reinterpret_cast<int2*>(a->scratch));
  launch("view_time_colors", vw::k_view_time_colors, dim3((unsigned)((elems + vw::kThreads - 1) / vw::kThreads)),
         dim3(vw::kThreads), st, *a, nblk);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_view_overlay(const mgs_view_overlay_args* a, void* stream) {
  const int32_t rc = vw::overlay_status(a);
  if (rc != MGS_OK) return rc;
  const int S = 8 * a->num_poses + a->num_free;
  if (S == 0) return MGS_OK;
  hipStream_t st = (hipStream_t)stream;
  launch("view_overlay_project", vw::k_view_overlay_project, dim3((S + vw::kThreads - 1) / vw::kThreads), dim3(vw::kThreads),
         st, *a, S);
  return vw::overlay_draw(a, S, st);
}

}  // extern "C"
