// Frame-to-model ICP: point-to-plane alignment of a sensor depth plane against a model view, the whole coarse-to-fine
// schedule enqueued at once (DESIGN.md "Frame-to-model ICP"; the contract is in include/monogs_raster.h, the mirror is
// monogs_amd/icp.py: icp_rows_numpy, icp_solve_numpy, align_numpy).  Every fp32 / fp64 operation of the contract is a
// single rounding (rn_math.h) and every sum is an integer sum, so the device equals the mirror bit for bit.
//
//   k_icp_start   one thread: D_0 = T_model T_init^-1, T_w2c, the record cleared
//   k_icp_rows    a persistent grid, a wave per 8 x 8 tile of the stride grid (the ray cast's lane mapping, so the gathers
//                 into the model planes stay local), striding over the tiles.  A lane keeps the 28 fixed-point sums and
//                 the 7 counts in registers over its trips; shuffles across the wave, the four wave totals through LDS,
//                 ONE plain store of a row of 35 words per workgroup.  No atomics.
//   k_icp_solve   one workgroup: its four waves add the partial rows (integers: any order), thread 0 runs the LDL^T solve,
//                 the update of D, the status, the history row and T_w2c.
// RGB-D alignment (mgs_icp_align_rgbd; the header's "RGB-D alignment", the mirror is align_numpy(image=, photo_weight=)):
//   k_icp_intensity   a thread per pixel, one launch per image: luma and its central-difference gradient, [3,H,W]
//   k_icp_rows_rgbd   k_icp_rows' grid and lane mapping; a pixel that projects into the model view adds a photometric row
//                     lambda [J_I, r_I] beside its geometric row, into the same 28 sums; rows of 39 words
//   k_icp_solve_rgbd  k_icp_solve's body at the width of 39: the same solve, too few counts both kinds of rows
// mgs_icp_align launches what it launched before; k_icp_rows is not touched by any of this.
// The sensor normal is READ from the plane mgs_depth_normal wrote: it is formed once per frame and not once per iteration
// (19 in the default schedule), and the bits are those of depth_normal_torch by that kernel's own test.
//
// The bound that keeps the sums in int64 (the header states it): |n_a| <= 1 and |p_a| < 16 give |J_i| < 2^5, dist <= 8
// gives |r| < 2^5, a product is below 2^10, trunc(v 2^30) below 2^40, and at most 2^22 pixels add up to less than 2^62.
// A photometric row is gated to |w_i| < 16: its products are below 2^8, a pixel adds less than (2^10 + 2^8) 2^30 with both
// rows, and 2^22 pixels less than 1.25 * 2^62 < 2^63.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "rn_math.h"

namespace mgs {
namespace icp {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 8;
constexpr int kSums = MGS_ICP_SUMS;
constexpr int kProducts = 28;
constexpr float kIndexLimit = 8388608.f;      // 2^23: |rintf(u)| below it converts to int exactly
constexpr float kRange = 16.f;
constexpr double kFixed = 1073741824.0;       // 2^30
constexpr double kFixedInv = 1.0 / 1073741824.0;

enum { REC_COUNTS = 28, REC_X = 35, REC_PIVOTS = 41, REC_STATUS = 47, REC_LEVEL = 48, REC_ITER = 49, REC_RUN = 50, REC_DONE = 51 };
enum { ACCEPTED = 0, INVALID, RANGE, OUTSIDE, NO_MODEL, DISTANCE, NORMAL, kCounts };

using mgs::sub_rn;      // the fp32 one, beside the fp64 one here
__device__ __forceinline__ double sub_rn(double a, double b) { return add_rn(a, -b); }

// ---- rigid transforms in fp64: the header's "Rigid" ------------------------------------------------------------------
struct Rigid {
  double R[3][3], t[3];
};

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return add_rn(add_rn(mul_rn(a0, b0), mul_rn(a1, b1)), mul_rn(a2, b2));
}

__device__ __forceinline__ Rigid inverse(const Rigid& A) {
  Rigid B;
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) B.R[a][b] = A.R[b][a];
  }
#pragma unroll
  for (int a = 0; a < 3; a++) B.t[a] = -dot3(B.R[a][0], A.t[0], B.R[a][1], A.t[1], B.R[a][2], A.t[2]);
  return B;
}

__device__ __forceinline__ Rigid product(const Rigid& A, const Rigid& B) {
  Rigid C;
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) C.R[a][b] = dot3(A.R[a][0], B.R[0][b], A.R[a][1], B.R[1][b], A.R[a][2], B.R[2][b]);
    C.t[a] = add_rn(dot3(A.R[a][0], B.t[0], A.R[a][1], B.t[1], A.R[a][2], B.t[2]), A.t[a]);
  }
  return C;
}

__device__ __forceinline__ Rigid load_f32(const float* T) {
  Rigid A;
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) A.R[a][b] = (double)T[4 * a + b];
    A.t[a] = (double)T[4 * a + 3];
  }
  return A;
}

__device__ __forceinline__ Rigid load_f64(const double* D) {
  Rigid A;
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) A.R[a][b] = D[4 * a + b];
    A.t[a] = D[4 * a + 3];
  }
  return A;
}

__device__ __forceinline__ void store_f64(double* D, const Rigid& A) {
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) D[4 * a + b] = A.R[a][b];
    D[4 * a + 3] = A.t[a];
  }
}

// T_w2c = D^-1 T_model, rounded once
__device__ __forceinline__ void store_pose(float* T_w2c, const Rigid& D, const float* T_model) {
  const Rigid P = product(inverse(D), load_f32(T_model));
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) T_w2c[4 * a + b] = (float)P.R[a][b];
    T_w2c[4 * a + 3] = (float)P.t[a];
  }
  T_w2c[12] = 0.f; T_w2c[13] = 0.f; T_w2c[14] = 0.f; T_w2c[15] = 1.f;
}

__global__ __launch_bounds__(64) void k_icp_start(mgs_icp_args A) {
  if (threadIdx.x != 0) return;
  Rigid D;
  if (A.T_init) {
    D = product(load_f32(A.T_model), inverse(load_f32(A.T_init)));
  } else {
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int b = 0; b < 3; b++) D.R[a][b] = a == b ? 1.0 : 0.0;
      D.t[a] = 0.0;
    }
  }
  store_f64(A.D, D);
  store_pose(A.T_w2c, D, A.T_model);
  for (int i = 0; i < MGS_ICP_RECORD_WORDS; i++) A.record[i] = 0;
  A.record[REC_DONE] = -1;
}

// a launch of level `level` has nothing to do after a failure and once its level has converged
__device__ __forceinline__ bool idle(const int64_t* record, int level) {
  return record[REC_STATUS] >= MGS_ICP_TOO_FEW || record[REC_DONE] == level;
}

// ---- the rows ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_icp_rows(mgs_icp_args A, int level, int stride, int tiles_x, int tiles,
                                                       long long* __restrict__ partial) {
  __shared__ long long s_red[kWaves][kSums];
  if (idle(A.record, level)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int Ws = (A.width + stride - 1) / stride, Hs = (A.height + stride - 1) / stride;
  const size_t HW = (size_t)A.width * A.height, HWm = (size_t)A.model_width * A.model_height;
  float R[3][3], t[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) R[a][b] = (float)A.D[4 * a + b];
    t[a] = (float)A.D[4 * a + 3];
  }
  const float dist2 = mul_rn(A.dist, A.dist);
  long long acc[kProducts];
  int cnt[kCounts];
#pragma unroll
  for (int i = 0; i < kProducts; i++) acc[i] = 0;
#pragma unroll
  for (int i = 0; i < kCounts; i++) cnt[i] = 0;
  for (int tile = blockIdx.x * kWaves + wave; tile < tiles; tile += gridDim.x * kWaves) {      // wave-uniform
    const int gx = (tile % tiles_x) * kTile + (lane & 7), gy = (tile / tiles_x) * kTile + (lane >> 3);
    if (gx >= Ws || gy >= Hs) continue;
    const int u = gx * stride, v = gy * stride;
    const size_t pix = (size_t)v * A.width + u;
    const float d = A.depth[pix];
    const float ns[3] = {A.normal[pix], A.normal[HW + pix], A.normal[2 * HW + pix]};
    if (!(d > 0.f && d < __builtin_inff() && d <= A.depth_max && (ns[0] != 0.f || ns[1] != 0.f || ns[2] != 0.f))) {
      cnt[INVALID]++;
      continue;
    }
    const float rx = __fdiv_rn(sub_rn((float)u, A.cx), A.fx), ry = __fdiv_rn(sub_rn((float)v, A.cy), A.fy);
    const float X[3] = {mul_rn(rx, d), mul_rn(ry, d), d};
    float p[3], nr[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      p[a] = add_rn(add_rn(add_rn(mul_rn(R[a][0], X[0]), mul_rn(R[a][1], X[1])), mul_rn(R[a][2], X[2])), t[a]);
      nr[a] = add_rn(add_rn(mul_rn(R[a][0], ns[0]), mul_rn(R[a][1], ns[1])), mul_rn(R[a][2], ns[2]));
    }
    if (!(p[2] > 0.f && fabsf(p[0]) < kRange && fabsf(p[1]) < kRange && fabsf(p[2]) < kRange)) {
      cnt[RANGE]++;
      continue;
    }
    const float uf = rintf(add_rn(mul_rn(A.mfx, __fdiv_rn(p[0], p[2])), A.mcx));
    const float vf = rintf(add_rn(mul_rn(A.mfy, __fdiv_rn(p[1], p[2])), A.mcy));
    // in float first: a NaN or a huge value is no index; then the bounds, before any load
    bool inside = fabsf(uf) < kIndexLimit && fabsf(vf) < kIndexLimit;
    const int um = inside ? (int)uf : -1, vm = inside ? (int)vf : -1;
    inside = inside && um >= 0 && um < A.model_width && vm >= 0 && vm < A.model_height;
    if (!inside) {
      cnt[OUTSIDE]++;
      continue;
    }
    const size_t mp = (size_t)vm * A.model_width + um;
    const float dm = A.model_depth[mp];
    float n[3];
#pragma unroll
    for (int a = 0; a < 3; a++) n[a] = A.model_normal_chw ? A.model_normal[a * HWm + mp] : A.model_normal[3 * mp + a];
    if (!(dm > 0.f && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f) && fabsf(n[0]) <= 1.f && fabsf(n[1]) <= 1.f && fabsf(n[2]) <= 1.f)) {
      cnt[NO_MODEL]++;
      continue;
    }
    const float qx = mul_rn(__fdiv_rn(sub_rn(uf, A.mcx), A.mfx), dm), qy = mul_rn(__fdiv_rn(sub_rn(vf, A.mcy), A.mfy), dm);
    const float e[3] = {sub_rn(p[0], qx), sub_rn(p[1], qy), sub_rn(p[2], dm)};
    if (!(add_rn(add_rn(mul_rn(e[0], e[0]), mul_rn(e[1], e[1])), mul_rn(e[2], e[2])) <= dist2)) {
      cnt[DISTANCE]++;
      continue;
    }
    if (!(add_rn(add_rn(mul_rn(n[0], nr[0]), mul_rn(n[1], nr[1])), mul_rn(n[2], nr[2])) >= A.cos_min)) {
      cnt[NORMAL]++;
      continue;
    }
    cnt[ACCEPTED]++;
    float w[7];
    w[0] = n[0]; w[1] = n[1]; w[2] = n[2];
    w[3] = sub_rn(mul_rn(p[1], n[2]), mul_rn(p[2], n[1]));
    w[4] = sub_rn(mul_rn(p[2], n[0]), mul_rn(p[0], n[2]));
    w[5] = sub_rn(mul_rn(p[0], n[1]), mul_rn(p[1], n[0]));
    w[6] = add_rn(add_rn(mul_rn(n[0], e[0]), mul_rn(n[1], e[1])), mul_rn(n[2], e[2]));
    int k = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) {
#pragma unroll
      for (int j = i; j < 7; j++) acc[k++] += (long long)((double)mul_rn(w[i], w[j]) * kFixed);      // |v| 2^30 < 2^40: exact, truncated
    }
  }
  // integers: the order of these adds does not matter
#pragma unroll
  for (int i = 0; i < kSums; i++) {
    long long v = i < kProducts ? acc[i] : (long long)cnt[i - kProducts];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) s_red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += s_red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * kSums + threadIdx.x] = s;
  }
}

// ---- RGB-D: the intensity planes and the rows with a photometric row (the header's "RGB-D alignment") -----------------
constexpr int kSumsRgbd = MGS_ICP_RGBD_SUMS;
constexpr float kNoIntensity = -1.f, kNoGradient = 2.f;      // what no valid value is, as (0,0,0) is no normal
constexpr float kPhotoBound = 16.f;
constexpr float kFixedF = 1073741824.f;      // v 2^30 is exact in fp32 too (|v| < 2^10), and so is its truncation to int64
enum { PHOTO_ACCEPTED = 0, PHOTO_INVALID, PHOTO_BOUND, kPhotoCounts };
enum { REC_PHOTO = 52 };

// the luma of pixel (x, y), or kNoIntensity: outside the image, a channel outside [0, 1] (false for a NaN), validity off
__device__ __forceinline__ float luma_at(const mgs_icp_intensity_args& A, int x, int y) {
  if (x < 0 || x >= A.width || y < 0 || y >= A.height) return kNoIntensity;
  const size_t HW = (size_t)A.width * A.height, pix = (size_t)y * A.width + x;
  if (A.valid && !(A.valid[pix] > 0.f)) return kNoIntensity;
  const float r = A.chw ? A.rgb[pix] : A.rgb[3 * pix], g = A.chw ? A.rgb[HW + pix] : A.rgb[3 * pix + 1];
  const float b = A.chw ? A.rgb[2 * HW + pix] : A.rgb[3 * pix + 2];
  if (!(r >= 0.f && r <= 1.f && g >= 0.f && g <= 1.f && b >= 0.f && b <= 1.f)) return kNoIntensity;
  return add_rn(add_rn(mul_rn(0.299f, r), mul_rn(0.587f, g)), mul_rn(0.114f, b));
}

__global__ __launch_bounds__(kThreads) void k_icp_intensity(mgs_icp_intensity_args A) {
  const size_t HW = (size_t)A.width * A.height;
  const size_t pix = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (pix >= HW) return;
  const int y = (int)(pix / A.width), x = (int)(pix - (size_t)y * A.width);
  const float l = luma_at(A, x - 1, y), r = luma_at(A, x + 1, y), u = luma_at(A, x, y - 1), d = luma_at(A, x, y + 1);
  A.out[pix] = luma_at(A, x, y);
  A.out[HW + pix] = l >= 0.f && r >= 0.f ? mul_rn(0.5f, sub_rn(r, l)) : kNoGradient;
  A.out[2 * HW + pix] = u >= 0.f && d >= 0.f ? mul_rn(0.5f, sub_rn(d, u)) : kNoGradient;
}

// f00 + ax (f01 - f00) and the same below, then along y: the header's P2
__device__ __forceinline__ float bilinear(float f00, float f01, float f10, float f11, float ax, float ay) {
  const float top = add_rn(f00, mul_rn(ax, sub_rn(f01, f00))), bot = add_rn(f10, mul_rn(ax, sub_rn(f11, f10)));
  return add_rn(top, mul_rn(ay, sub_rn(bot, top)));
}

// k_icp_rows with the photometric row: a kernel of its own, so that k_icp_rows keeps its code and its registers.  Steps
// 1 - 4 and 5 - 9 are that kernel's lines; P1 - P5 stand between them and leave through `photo`, never through `continue`.
__global__ __launch_bounds__(kThreads) void k_icp_rows_rgbd(mgs_icp_args A, float lambda, const float* __restrict__ sensor_int,
                                                            const float* __restrict__ model_int, int level, int stride, int tiles_x,
                                                            int tiles, long long* __restrict__ partial) {
  __shared__ long long s_red[kWaves][kSumsRgbd];
  if (idle(A.record, level)) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int Ws = (A.width + stride - 1) / stride, Hs = (A.height + stride - 1) / stride;
  const size_t HW = (size_t)A.width * A.height, HWm = (size_t)A.model_width * A.model_height;
  float R[3][3], t[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int b = 0; b < 3; b++) R[a][b] = (float)A.D[4 * a + b];
    t[a] = (float)A.D[4 * a + 3];
  }
  const float dist2 = mul_rn(A.dist, A.dist);
  long long acc[kProducts], acc_ri2 = 0;
  int cnt[kCounts], pcnt[kPhotoCounts];
#pragma unroll
  for (int i = 0; i < kProducts; i++) acc[i] = 0;
#pragma unroll
  for (int i = 0; i < kCounts; i++) cnt[i] = 0;
#pragma unroll
  for (int i = 0; i < kPhotoCounts; i++) pcnt[i] = 0;
  for (int tile = blockIdx.x * kWaves + wave; tile < tiles; tile += gridDim.x * kWaves) {      // wave-uniform
    const int gx = (tile % tiles_x) * kTile + (lane & 7), gy = (tile / tiles_x) * kTile + (lane >> 3);
    if (gx >= Ws || gy >= Hs) continue;
    const int u = gx * stride, v = gy * stride;
    const size_t pix = (size_t)v * A.width + u;
    const float d = A.depth[pix];
    const float ns[3] = {A.normal[pix], A.normal[HW + pix], A.normal[2 * HW + pix]};
    if (!(d > 0.f && d < __builtin_inff() && d <= A.depth_max && (ns[0] != 0.f || ns[1] != 0.f || ns[2] != 0.f))) {
      cnt[INVALID]++;
      continue;
    }
    const float rx = __fdiv_rn(sub_rn((float)u, A.cx), A.fx), ry = __fdiv_rn(sub_rn((float)v, A.cy), A.fy);
    const float X[3] = {mul_rn(rx, d), mul_rn(ry, d), d};
    float p[3], nr[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      p[a] = add_rn(add_rn(add_rn(mul_rn(R[a][0], X[0]), mul_rn(R[a][1], X[1])), mul_rn(R[a][2], X[2])), t[a]);
      nr[a] = add_rn(add_rn(mul_rn(R[a][0], ns[0]), mul_rn(R[a][1], ns[1])), mul_rn(R[a][2], ns[2]));
    }
    if (!(p[2] > 0.f && fabsf(p[0]) < kRange && fabsf(p[1]) < kRange && fabsf(p[2]) < kRange)) {
      cnt[RANGE]++;
      continue;
    }
    const float xf = add_rn(mul_rn(A.mfx, __fdiv_rn(p[0], p[2])), A.mcx), yf = add_rn(mul_rn(A.mfy, __fdiv_rn(p[1], p[2])), A.mcy);
    const float uf = rintf(xf), vf = rintf(yf);
    // in float first: a NaN or a huge value is no index; then the bounds, before any load
    bool inside = fabsf(uf) < kIndexLimit && fabsf(vf) < kIndexLimit;
    const int um = inside ? (int)uf : -1, vm = inside ? (int)vf : -1;
    inside = inside && um >= 0 && um < A.model_width && vm >= 0 && vm < A.model_height;
    if (!inside) {
      cnt[OUTSIDE]++;
      continue;
    }
    // The two rows of the pixel take turns through ONE copy of the 28 products, in a loop that is kept rolled; `kind` is
    // uniform.  335 registers, one wave per SIMD - which is what the persistent grid of at most 256 workgroups places on
    // the 256 CUs anyway.  (Both rows unrolled: 426 registers.  Asking for two waves per SIMD spills 187 to scratch.)
#pragma unroll 1
    for (int kind = 0; kind < 2; kind++) {
    float w[7];
    bool on = false;
    if (kind == 0) {      // P1 - P5: the photometric row
      const float Is = sensor_int[pix];
      const float x0f = floorf(xf), y0f = floorf(yf);
      bool photo = Is >= 0.f && fabsf(x0f) < kIndexLimit && fabsf(y0f) < kIndexLimit;
      const int x0 = photo ? (int)x0f : -1, y0 = photo ? (int)y0f : -1;
      photo = photo && x0 >= 0 && x0 < A.model_width - 1 && y0 >= 0 && y0 < A.model_height - 1;
      float f[3][4];
      if (photo) {
        const size_t m00 = (size_t)y0 * A.model_width + x0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float* plane = model_int + c * HWm;
          f[c][0] = plane[m00]; f[c][1] = plane[m00 + 1]; f[c][2] = plane[m00 + A.model_width]; f[c][3] = plane[m00 + A.model_width + 1];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) photo = photo && f[0][k] >= 0.f && fabsf(f[1][k]) <= 1.f && fabsf(f[2][k]) <= 1.f;
      }
      if (!photo) {
        pcnt[PHOTO_INVALID]++;
      } else {
        const float ax = sub_rn(xf, x0f), ay = sub_rn(yf, y0f);
        const float Im = bilinear(f[0][0], f[0][1], f[0][2], f[0][3], ax, ay);
        const float gxm = bilinear(f[1][0], f[1][1], f[1][2], f[1][3], ax, ay);
        const float gym = bilinear(f[2][0], f[2][1], f[2][2], f[2][3], ax, ay);
        const float rI = sub_rn(Im, Is);
        const float a = mul_rn(gxm, A.mfx), b = mul_rn(gym, A.mfy);
        float J[6];
        J[0] = __fdiv_rn(a, p[2]);
        J[1] = __fdiv_rn(b, p[2]);
        J[2] = -__fdiv_rn(__fdiv_rn(add_rn(mul_rn(a, p[0]), mul_rn(b, p[1])), p[2]), p[2]);
        J[3] = sub_rn(mul_rn(p[1], J[2]), mul_rn(p[2], J[1]));
        J[4] = sub_rn(mul_rn(p[2], J[0]), mul_rn(p[0], J[2]));
        J[5] = sub_rn(mul_rn(p[0], J[1]), mul_rn(p[1], J[0]));
        bool bounded = true;
#pragma unroll
        for (int i = 0; i < 7; i++) {
          w[i] = mul_rn(lambda, i < 6 ? J[i] : rI);
          bounded = bounded && fabsf(w[i]) < kPhotoBound;      // false for a NaN
        }
        if (!bounded) {
          pcnt[PHOTO_BOUND]++;
        } else {
          pcnt[PHOTO_ACCEPTED]++;
          on = true;
          acc_ri2 += (long long)mul_rn(mul_rn(rI, rI), kFixedF);
        }
      }
    } else do {      // steps 5 - 9: the geometric row; a gate leaves through `break`
    const size_t mp = (size_t)vm * A.model_width + um;
    const float dm = A.model_depth[mp];
    float n[3];
#pragma unroll
    for (int a = 0; a < 3; a++) n[a] = A.model_normal_chw ? A.model_normal[a * HWm + mp] : A.model_normal[3 * mp + a];
    if (!(dm > 0.f && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f) && fabsf(n[0]) <= 1.f && fabsf(n[1]) <= 1.f && fabsf(n[2]) <= 1.f)) {
      cnt[NO_MODEL]++;
      break;
    }
    const float qx = mul_rn(__fdiv_rn(sub_rn(uf, A.mcx), A.mfx), dm), qy = mul_rn(__fdiv_rn(sub_rn(vf, A.mcy), A.mfy), dm);
    const float e[3] = {sub_rn(p[0], qx), sub_rn(p[1], qy), sub_rn(p[2], dm)};
    if (!(add_rn(add_rn(mul_rn(e[0], e[0]), mul_rn(e[1], e[1])), mul_rn(e[2], e[2])) <= dist2)) {
      cnt[DISTANCE]++;
      break;
    }
    if (!(add_rn(add_rn(mul_rn(n[0], nr[0]), mul_rn(n[1], nr[1])), mul_rn(n[2], nr[2])) >= A.cos_min)) {
      cnt[NORMAL]++;
      break;
    }
    cnt[ACCEPTED]++;
    on = true;
    w[0] = n[0]; w[1] = n[1]; w[2] = n[2];
    w[3] = sub_rn(mul_rn(p[1], n[2]), mul_rn(p[2], n[1]));
    w[4] = sub_rn(mul_rn(p[2], n[0]), mul_rn(p[0], n[2]));
    w[5] = sub_rn(mul_rn(p[0], n[1]), mul_rn(p[1], n[0]));
    w[6] = add_rn(add_rn(mul_rn(n[0], e[0]), mul_rn(n[1], e[1])), mul_rn(n[2], e[2]));
    } while (false);
    if (on) {      // integer adds: the order of the rows does not matter.  |v| 2^30 < 2^40: exact, truncated
      int k = 0;
#pragma unroll
      for (int i = 0; i < 7; i++) {
#pragma unroll
        for (int j = i; j < 7; j++) acc[k++] += (long long)mul_rn(mul_rn(w[i], w[j]), kFixedF);
      }
    }
    }
  }
  // integers: the order of these adds does not matter
#pragma unroll
  for (int i = 0; i < kSumsRgbd; i++) {
    long long v = i < kProducts ? acc[i] : i < kSums ? (long long)cnt[i - kProducts] : i < kSums + kPhotoCounts ? (long long)pcnt[i - kSums] : acc_ri2;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) s_red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSumsRgbd) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += s_red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * kSumsRgbd + threadIdx.x] = s;
  }
}

// ---- the solve --------------------------------------------------------------------------------------------------------
// The even Taylor series of a = sin(phi)/phi, b = (1 - cos(phi))/phi^2, c = (phi - sin(phi))/phi^3 in s = phi^2:
// a = sum (-s)^k / (2k+1)!, b = sum (-s)^k / (2k+2)!, c = sum (-s)^k / (2k+3)!.  They alternate with falling terms, so the
// error of k = 0 .. K-1 is below the first term left out, s^K / (2K+m)!.  At the largest s = 0.25, with K = 7:
//   a >= 0.95 in [0.5, 1):      ulp 2^-53 = 1.1e-16,  0.25^7 / 15! = 6.1e-5 / 1.31e12 = 4.7e-17   (K = 6: 3.9e-14)
//   b >= 0.48 in [0.25, 0.5):   ulp 2^-54 = 5.6e-17,  0.25^7 / 16! = 2.9e-18                      (K = 6: 2.8e-15)
//   c >= 0.16 in [0.125, 0.25): ulp 2^-55 = 2.8e-17,  0.25^7 / 17! = 1.7e-19                      (K = 6: 1.9e-16)
// so seven terms each.  The factorials up to 15! are exact in fp64 and each constant is ONE division.
constexpr int kTerms = MGS_ICP_EXP_TERMS;
__device__ const double kCoefA[kTerms] = {1.0, 1.0 / 6.0, 1.0 / 120.0, 1.0 / 5040.0, 1.0 / 362880.0, 1.0 / 39916800.0, 1.0 / 6227020800.0};
__device__ const double kCoefB[kTerms] = {1.0 / 2.0, 1.0 / 24.0, 1.0 / 720.0, 1.0 / 40320.0, 1.0 / 3628800.0, 1.0 / 479001600.0,
                                          1.0 / 87178291200.0};
__device__ const double kCoefC[kTerms] = {1.0 / 6.0, 1.0 / 120.0, 1.0 / 5040.0, 1.0 / 362880.0, 1.0 / 39916800.0, 1.0 / 6227020800.0,
                                          1.0 / 1307674368000.0};

__device__ __forceinline__ double horner(const double* c, double u) {
  double v = c[kTerms - 1];
#pragma unroll
  for (int k = kTerms - 2; k >= 0; k--) v = add_rn(c[k], mul_rn(u, v));
  return v;
}

// E = Exp([rho; theta]) for s = |theta|^2 <= 0.25
__device__ __forceinline__ Rigid se3_exp(const double x[6], double s) {
  const double a = horner(kCoefA, -s), b = horner(kCoefB, -s), c = horner(kCoefC, -s);
  const double th[3] = {x[3], x[4], x[5]};
  const double W[3][3] = {{0.0, -th[2], th[1]}, {th[2], 0.0, -th[0]}, {-th[1], th[0], 0.0}};
  Rigid E;
  double V[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double w2 = i == j ? sub_rn(mul_rn(th[i], th[j]), s) : mul_rn(th[i], th[j]);
      const double I = i == j ? 1.0 : 0.0;
      E.R[i][j] = add_rn(add_rn(I, mul_rn(a, W[i][j])), mul_rn(b, w2));
      V[i][j] = add_rn(add_rn(I, mul_rn(b, W[i][j])), mul_rn(c, w2));
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++) E.t[i] = dot3(V[i][0], x[0], V[i][1], x[1], V[i][2], x[2]);
  return E;
}

__device__ __forceinline__ int tri(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }      // (i, j), i <= j, of the 7 x 7 triangle

// One body for both widths of a partial row: kWidth = kSums is k_icp_solve as it always was, kWidth = kSumsRgbd also carries
// the photometric counts and the sum of r_I^2 into the record's words 52 .. 55 and the history row's word 7, and counts the
// photometric rows into the too-few test.  The arithmetic of the solve is the same lines.
template <int kWidth>
__device__ __forceinline__ void solve_body(const mgs_icp_args& A, int level, int iteration, int index, int last, int nblk,
                                           const long long* __restrict__ partial, int64_t* __restrict__ history) {
  constexpr bool kRgbd = kWidth > kSums;
  __shared__ long long s_part[kWaves][kWidth];
  __shared__ long long s_sum[kWidth];
  int64_t* row = history + (size_t)MGS_ICP_HISTORY_WORDS * index;
  if (idle(A.record, level)) {
    if (threadIdx.x == 0) {
      row[0] = 0; row[1] = 0; row[2] = 0; row[3] = A.record[REC_STATUS]; row[4] = 0; row[5] = level; row[6] = iteration; row[7] = 0;
    }
    return;
  }
  // wave w adds the rows w, w + 4, ...: four short chains of independent loads instead of one of nblk
  const int col = threadIdx.x & 63, part = threadIdx.x >> 6;
  if (col < kWidth) {
    long long s = 0;
#pragma unroll 8
    for (int b = part; b < nblk; b += kWaves) s += partial[(size_t)b * kWidth + col];
    s_part[part][col] = s;
  }
  __syncthreads();
  if (threadIdx.x < kWidth) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += s_part[w][threadIdx.x];
    s_sum[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int64_t* rec = A.record;
  for (int i = 0; i < kSums; i++) rec[i] = s_sum[i];
  if constexpr (kRgbd) {
    for (int i = kSums; i < kWidth; i++) rec[REC_PHOTO + i - kSums] = s_sum[i];
  }
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, piv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xx = 0.0;
  int status = MGS_ICP_ITERATING;
  if (s_sum[kProducts + ACCEPTED] + (kRgbd ? s_sum[kWidth - 4 + PHOTO_ACCEPTED] : 0) < (long long)A.min_pixels) {
    status = MGS_ICP_TOO_FEW;
  } else {
    double H[6][6], g[6], L[6][6], d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int j = i; j < 6; j++) H[i][j] = H[j][i] = mul_rn((double)s_sum[tri(i, j)], kFixedInv);
      g[i] = mul_rn((double)s_sum[tri(i, 6)], kFixedInv);
    }
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      H[i][i] = add_rn(H[i][i], A.damping);
      m = i == 0 || H[i][i] > m ? H[i][i] : m;
    }
    const double floor_ = mul_rn(A.min_pivot_ratio, m);
#pragma unroll
    for (int j = 0; j < 6; j++) {
      double tk[6], v = H[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) {
        tk[k] = mul_rn(L[j][k], d[k]);
        v = sub_rn(v, mul_rn(L[j][k], tk[k]));
      }
      piv[j] = v;
      const bool good = v > floor_;      // before any division by it; false for a NaN
      if (!good) status = MGS_ICP_DEGENERATE;
      d[j] = good ? v : 0.0;
#pragma unroll
      for (int i = j + 1; i < 6; i++) {
        double s = H[i][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = sub_rn(s, mul_rn(L[i][k], tk[k]));
        L[i][j] = good ? div_rn(s, v) : 0.0;
      }
    }
    if (status != MGS_ICP_DEGENERATE) {
      double y[6];
#pragma unroll
      for (int i = 0; i < 6; i++) {
        double v = -g[i];
#pragma unroll
        for (int k = 0; k < i; k++) v = sub_rn(v, mul_rn(L[i][k], y[k]));
        y[i] = v;
      }
#pragma unroll
      for (int i = 5; i >= 0; i--) {
        double v = div_rn(y[i], d[i]);
#pragma unroll
        for (int k = i + 1; k < 6; k++) v = sub_rn(v, mul_rn(L[k][i], x[k]));
        x[i] = v;
      }
      const double s = add_rn(add_rn(mul_rn(x[3], x[3]), mul_rn(x[4], x[4])), mul_rn(x[5], x[5]));
      xx = mul_rn(x[0], x[0]);
#pragma unroll
      for (int i = 1; i < 6; i++) xx = add_rn(xx, mul_rn(x[i], x[i]));
      if (!(s <= 0.25) || !(xx < __builtin_inf())) {
        status = MGS_ICP_STEP_TOO_LARGE;
      } else {
        const Rigid D = product(se3_exp(x, s), load_f64(A.D));
        store_f64(A.D, D);
        store_pose(A.T_w2c, D, A.T_model);
        if (xx < mul_rn(A.converged, A.converged)) {
          status = MGS_ICP_CONVERGED;
          rec[REC_DONE] = level;
        } else if (last) {
          status = MGS_ICP_MAX_ITERATIONS;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    rec[REC_X + i] = __double_as_longlong(x[i]);
    rec[REC_PIVOTS + i] = __double_as_longlong(piv[i]);
  }
  rec[REC_STATUS] = status;
  rec[REC_LEVEL] = level;
  rec[REC_ITER] = iteration;
  rec[REC_RUN] = rec[REC_RUN] + 1;
  row[0] = s_sum[kProducts + ACCEPTED]; row[1] = s_sum[tri(6, 6)]; row[2] = __double_as_longlong(xx); row[3] = status;
  row[4] = 1; row[5] = level; row[6] = iteration; row[7] = kRgbd ? s_sum[kWidth - 1] : 0;
}

__global__ __launch_bounds__(kThreads) void k_icp_solve(mgs_icp_args A, int level, int iteration, int index, int last, int nblk,
                                                        const long long* __restrict__ partial, int64_t* __restrict__ history) {
  solve_body<kSums>(A, level, iteration, index, last, nblk, partial, history);
}

__global__ __launch_bounds__(kThreads) void k_icp_solve_rgbd(mgs_icp_args A, int level, int iteration, int index, int last, int nblk,
                                                             const long long* __restrict__ partial, int64_t* __restrict__ history) {
  solve_body<kSumsRgbd>(A, level, iteration, index, last, nblk, partial, history);
}

static int total_iterations(const mgs_icp_args& a) {
  long long n = 0;
  for (int l = 0; l < a.num_levels; l++) n += a.iterations[l];
  return n > MGS_ICP_MAX_ITERATIONS_TOTAL ? -1 : (int)n;
}

static bool in_range(double v, double lo, double hi) { return v >= lo && v <= hi; }      // false for a NaN

}  // namespace icp
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_icp_args_size(void) { return (int32_t)sizeof(mgs_icp_args); }

uint64_t mgs_icp_scratch_bytes(int32_t max_iterations_total) {
  if (max_iterations_total < 0 || max_iterations_total > MGS_ICP_MAX_ITERATIONS_TOTAL) return 0;
  return 8ull * ((uint64_t)MGS_ICP_ROWS_BLOCKS * MGS_ICP_SUMS + (uint64_t)MGS_ICP_HISTORY_WORDS * (uint64_t)max_iterations_total);
}

// what both entries refuse: MGS_OK, or the error
static int32_t icp_check(const mgs_icp_args* a) {
  if (!a || !a->depth || !a->normal || !a->model_depth || !a->model_normal || !a->T_model || !a->scratch || !a->T_w2c || !a->D ||
      !a->record)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->width < 1 || a->height < 1 || a->model_width < 1 || a->model_height < 1) return MGS_ERR_BAD_ARGUMENT;
  if (!(a->fx > 0.f) || !(a->fy > 0.f) || !(a->mfx > 0.f) || !(a->mfy > 0.f) || !(a->cx == a->cx) || !(a->cy == a->cy) ||
      !(a->mcx == a->mcx) || !(a->mcy == a->mcy))
    return MGS_ERR_BAD_ARGUMENT;
  if (a->model_normal_chw < 0 || a->model_normal_chw > 1 || a->min_pixels < 0) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_levels < 1 || a->num_levels > MGS_ICP_MAX_LEVELS) return MGS_ERR_BAD_ARGUMENT;
  for (int l = 0; l < a->num_levels; l++)
    if (a->stride[l] < 1 || a->iterations[l] < 1) return MGS_ERR_BAD_ARGUMENT;
  const int total = icp::total_iterations(*a);
  if (total < 0) return MGS_ERR_BAD_ARGUMENT;
  if (!icp::in_range(a->dist, 0.0, 8.0) || !icp::in_range(a->cos_min, -1.0, 1.0) || !icp::in_range(a->depth_max, 0.0, 16.0) ||
      !icp::in_range(a->min_pivot_ratio, 0.0, 1.0) || !icp::in_range(a->damping, 0.0, 1.7e308) || !icp::in_range(a->converged, 0.0, 1.7e308))
    return MGS_ERR_BAD_ARGUMENT;
  if (((uintptr_t)a->scratch & 7) || ((uintptr_t)a->D & 7) || ((uintptr_t)a->record & 7)) return MGS_ERR_BAD_ARGUMENT;
  if ((int64_t)a->width * a->height > MGS_ICP_MAX_PIXELS) return MGS_ERR_UNSUPPORTED;
  if ((int64_t)a->model_width * a->model_height > 0x7fffffff / 3) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

// the schedule of either entry: `rgbd` null is mgs_icp_align's, launch for launch
static int32_t icp_enqueue(const mgs_icp_args* a, const mgs_icp_rgbd_args* rgbd, hipStream_t st) {
  const int total = icp::total_iterations(*a);
  long long* partial = static_cast<long long*>(a->scratch);
  int64_t* history = static_cast<int64_t*>(a->scratch) + (size_t)MGS_ICP_ROWS_BLOCKS * (rgbd ? MGS_ICP_RGBD_SUMS : MGS_ICP_SUMS);
  launch("icp_start", icp::k_icp_start, dim3(1), dim3(64), st, *a);
  int index = 0;
  for (int l = 0; l < a->num_levels; l++) {
    const int s = a->stride[l];
    const int Ws = (a->width + s - 1) / s, Hs = (a->height + s - 1) / s;
    const int tiles_x = (Ws + icp::kTile - 1) / icp::kTile, tiles = tiles_x * ((Hs + icp::kTile - 1) / icp::kTile);
    const int nblk = (tiles + icp::kWaves - 1) / icp::kWaves < MGS_ICP_ROWS_BLOCKS ? (tiles + icp::kWaves - 1) / icp::kWaves : MGS_ICP_ROWS_BLOCKS;
    for (int i = 0; i < a->iterations[l]; i++, index++) {
      if (rgbd) {
        launch("icp_rows_rgbd", icp::k_icp_rows_rgbd, dim3(nblk), dim3(icp::kThreads), st, *a, rgbd->photo_weight,
               (const float*)rgbd->intensity, (const float*)rgbd->model_intensity, l, s, tiles_x, tiles, partial);
        launch("icp_solve_rgbd", icp::k_icp_solve_rgbd, dim3(1), dim3(icp::kThreads), st, *a, l, i, index, (int)(index == total - 1), nblk,
               (const long long*)partial, history);
      } else {
        launch("icp_rows", icp::k_icp_rows, dim3(nblk), dim3(icp::kThreads), st, *a, l, s, tiles_x, tiles, partial);
        launch("icp_solve", icp::k_icp_solve, dim3(1), dim3(icp::kThreads), st, *a, l, i, index, (int)(index == total - 1), nblk,
               (const long long*)partial, history);
      }
    }
  }
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

static int32_t intensity_check(const mgs_icp_intensity_args* a) {
  if (!a || a->width < 1 || a->height < 1 || a->chw < 0 || a->chw > 1 || !a->rgb || !a->out) return MGS_ERR_BAD_ARGUMENT;
  if ((int64_t)a->width * a->height > 0x7fffffff / 3) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

static void intensity_enqueue(const mgs_icp_intensity_args& a, hipStream_t st) {
  const int HW = a.width * a.height;
  launch("icp_intensity", icp::k_icp_intensity, dim3((HW + icp::kThreads - 1) / icp::kThreads), dim3(icp::kThreads), st, a);
}

int32_t mgs_icp_align(const mgs_icp_args* a, void* stream) {
  const int32_t err = icp_check(a);
  return err != MGS_OK ? err : icp_enqueue(a, nullptr, (hipStream_t)stream);
}

int32_t mgs_icp_intensity_args_size(void) { return (int32_t)sizeof(mgs_icp_intensity_args); }

int32_t mgs_icp_rgbd_args_size(void) { return (int32_t)sizeof(mgs_icp_rgbd_args); }

uint64_t mgs_icp_rgbd_scratch_bytes(int32_t max_iterations_total) {
  if (max_iterations_total < 0 || max_iterations_total > MGS_ICP_MAX_ITERATIONS_TOTAL) return 0;
  return 8ull * ((uint64_t)MGS_ICP_ROWS_BLOCKS * MGS_ICP_RGBD_SUMS + (uint64_t)MGS_ICP_HISTORY_WORDS * (uint64_t)max_iterations_total);
}

int32_t mgs_icp_intensity(const mgs_icp_intensity_args* a, void* stream) {
  const int32_t err = intensity_check(a);
  if (err != MGS_OK) return err;
  intensity_enqueue(*a, (hipStream_t)stream);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_icp_align_rgbd(const mgs_icp_rgbd_args* r, void* stream) {
  if (!r) return MGS_ERR_BAD_ARGUMENT;
  const int32_t err = icp_check(&r->icp);
  if (err != MGS_OK) return err;
  if (!r->image || !r->model_color || !r->intensity || !r->model_intensity) return MGS_ERR_BAD_ARGUMENT;
  if (!(r->photo_weight >= 0.f && r->photo_weight <= MGS_ICP_PHOTO_WEIGHT_MAX)) return MGS_ERR_BAD_ARGUMENT;      // false for a NaN
  mgs_icp_intensity_args sensor = {r->icp.width, r->icp.height, r->image_chw, 0, r->image, nullptr, r->intensity};
  mgs_icp_intensity_args model = {r->icp.model_width, r->icp.model_height, r->model_color_chw, 0, r->model_color, r->icp.model_depth,
                                  r->model_intensity};
  const int32_t es = intensity_check(&sensor), em = intensity_check(&model);
  if (es != MGS_OK || em != MGS_OK) return es != MGS_OK ? es : em;
  hipStream_t st = (hipStream_t)stream;
  intensity_enqueue(sensor, st);
  intensity_enqueue(model, st);
  return icp_enqueue(&r->icp, r, st);
}

}  // extern "C"
