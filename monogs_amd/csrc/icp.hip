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
// The sensor normal is READ from the plane mgs_depth_normal wrote: it is formed once per frame and not once per iteration
// (19 in the default schedule), and the bits are those of depth_normal_torch by that kernel's own test.
//
// The bound that keeps the sums in int64 (the header states it): |n_a| <= 1 and |p_a| < 16 give |J_i| < 2^5, dist <= 8
// gives |r| < 2^5, a product is below 2^10, trunc(v 2^30) below 2^40, and at most 2^22 pixels add up to less than 2^62.
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

__global__ __launch_bounds__(kThreads) void k_icp_solve(mgs_icp_args A, int level, int iteration, int index, int last, int nblk,
                                                        const long long* __restrict__ partial, int64_t* __restrict__ history) {
  __shared__ long long s_part[kWaves][kSums];
  __shared__ long long s_sum[kSums];
  int64_t* row = history + (size_t)MGS_ICP_HISTORY_WORDS * index;
  if (idle(A.record, level)) {
    if (threadIdx.x == 0) {
      row[0] = 0; row[1] = 0; row[2] = 0; row[3] = A.record[REC_STATUS]; row[4] = 0; row[5] = level; row[6] = iteration; row[7] = 0;
    }
    return;
  }
  // wave w adds the rows w, w + 4, ...: four short chains of independent loads instead of one of nblk
  const int col = threadIdx.x & 63, part = threadIdx.x >> 6;
  if (col < kSums) {
    long long s = 0;
#pragma unroll 8
    for (int b = part; b < nblk; b += kWaves) s += partial[(size_t)b * kSums + col];
    s_part[part][col] = s;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) s += s_part[w][threadIdx.x];
    s_sum[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int64_t* rec = A.record;
  for (int i = 0; i < kSums; i++) rec[i] = s_sum[i];
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, piv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xx = 0.0;
  int status = MGS_ICP_ITERATING;
  if (s_sum[kProducts + ACCEPTED] < (long long)A.min_pixels) {
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
  row[4] = 1; row[5] = level; row[6] = iteration; row[7] = 0;
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

int32_t mgs_icp_align(const mgs_icp_args* a, void* stream) {
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
  hipStream_t st = (hipStream_t)stream;
  long long* partial = static_cast<long long*>(a->scratch);
  int64_t* history = static_cast<int64_t*>(a->scratch) + (size_t)MGS_ICP_ROWS_BLOCKS * MGS_ICP_SUMS;
  launch("icp_start", icp::k_icp_start, dim3(1), dim3(64), st, *a);
  int index = 0;
  for (int l = 0; l < a->num_levels; l++) {
    const int s = a->stride[l];
    const int Ws = (a->width + s - 1) / s, Hs = (a->height + s - 1) / s;
    const int tiles_x = (Ws + icp::kTile - 1) / icp::kTile, tiles = tiles_x * ((Hs + icp::kTile - 1) / icp::kTile);
    const int nblk = (tiles + icp::kWaves - 1) / icp::kWaves < MGS_ICP_ROWS_BLOCKS ? (tiles + icp::kWaves - 1) / icp::kWaves : MGS_ICP_ROWS_BLOCKS;
    for (int i = 0; i < a->iterations[l]; i++, index++) {
      launch("icp_rows", icp::k_icp_rows, dim3(nblk), dim3(icp::kThreads), st, *a, l, s, tiles_x, tiles, partial);
      launch("icp_solve", icp::k_icp_solve, dim3(1), dim3(icp::kThreads), st, *a, l, i, index, (int)(index == total - 1), nblk,
             (const long long*)partial, history);
    }
  }
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
