// Keyframe seeding on the device (mgs_keyframe_seed; DESIGN.md "Keyframe seeding on the device"): from a tracked frame
// (image, rendered or sensor depth, rendered opacity, camera) to the rows of its new Gaussians.  The reference does this
// in FrontEnd.add_new_keyframe (utils/slam_frontend.py:183-234) and GaussianModel.create_pcd_from_image_and_depth
// (gaussian_splatting/scene/gaussian_model.py:137-205) with open3d on the host.  Stream order:
//
//   memset            the call's state word block and its nine radix histograms
//   k_seed_prior<1-3> mode 0 only: three-level radix select of the lower median of the valid depths
//                     (depth > 0 && opacity > 0.95 && valid_rgb), as mgs_keyframe_decide's
//   k_seed_moments    mode 0 only: fp64 sums of (d - med), (d - med)^2 over the valid depths, one partial per workgroup
//   k_seed_prepare    std from the partials (fixed tree), the prepared depth map d (outliers -> med, noise, d = 0
//                     without image content except in mode 1), the sampling keys; level 1 of TWO selects: NumPy's median of all of d
//                     (on order-preserving keys) and the K-th smallest sampling key of the pixels with 0 < d <= trunc
//   k_seed_level<2,3> levels 2 and 3 of both selects
//   k_seed_count      per wave segment of the image: pixels below / at the key threshold, values <= the lower middle
//                     order statistic and the smallest value above it (for the mean of the two middle values)
//   k_seed_emit       scan of the segment counts, ballot compaction in ascending pixel order, back-projection, colour,
//                     rows; workgroup 0 writes the record
//   (host)            one copy of the record: K sizes the k-nn launcher's plan
//   k_knn_partial, k_knn_merge (knn.hip, unchanged), k_seed_scale
//
// A latency problem (1.2 MB per plane at 640x480): every launch is one resident round of workgroups.  Counting is
// integer, the float sums are fp64 over a fixed tree: two calls give bit-identical outputs.  Depth arithmetic that a
// torch mirror has to reproduce exactly goes through mul_rn / add_rn (no contraction into an fma).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "philox.h"
#include "radix_select.h"
#include "raster_kernels.h"
#include "rn_math.h"

namespace mgs {

namespace {

constexpr int kSeedThreads = 256;
constexpr int kSeedWaves = kSeedThreads / 64;
constexpr int kSeedMaxBlocks = 256;
constexpr int kSeedMaxSegments = kSeedMaxBlocks * kSeedWaves;   // one segment of the image per wave of count / emit
constexpr int kSeedStep = kSeedThreads * 4;                      // pixels per workgroup and step of the histogram passes
constexpr float kSH_C0 = 0.28209479177387814f;

// What the kernels hand each other (device; zeroed by the call's memset).
struct SeedState {
  float med, std;           // mode 0
  int n_valid;
  int n_outliers;           // integer atomics
  int prior_ok;             // mode 0: at least two valid pixels
  unsigned key_thr;         // the K-th smallest key
  int key_rank;             // pixels AT key_thr that are kept: the first key_rank + 1 in pixel order
  int K, n_depth;
  unsigned all_lo;          // order key of the lower middle order statistic of d
};

struct SeedScratch {
  SeedState* state;
  RadixHists prior, all, key;
  double* moments;          // [kSeedMaxBlocks][2]
  int4* seg;                // [kSeedMaxSegments] (below, at, <= all_lo, order key of the smallest value above all_lo)
  float* d;                 // [H*W] the prepared depth map (depth_out when the caller gave one)
  unsigned* keys;           // [H*W]
  float* dist2;             // [row_capacity]
  void* knn;
  int hb;                   // workgroups of the histogram passes
  int seg_len, n_seg;       // pixels per wave segment (a multiple of 64), segments
};

struct SeedLayout { uint64_t state, hists, zero_bytes, moments, seg, d, keys, dist2, knn, bytes; };

SeedLayout seed_layout(int num_pixels, int row_capacity) {
  SeedLayout L;
  uint64_t o = 0;
  L.state = o; o = align_up(o + sizeof(SeedState));
  L.hists = o; o = align_up(o + 3ull * kRadixHistInts * 4);
  L.zero_bytes = o;
  L.moments = o; o = align_up(o + (uint64_t)kSeedMaxBlocks * 2 * sizeof(double));
  L.seg = o; o = align_up(o + (uint64_t)kSeedMaxSegments * sizeof(int4));
  L.d = o; o = align_up(o + (uint64_t)num_pixels * 4);
  L.keys = o; o = align_up(o + (uint64_t)num_pixels * 4);
  L.dist2 = o; o = align_up(o + (uint64_t)row_capacity * 4);
  L.knn = o; o = align_up(o + knn_scratch_bytes(row_capacity));
  L.bytes = o;
  return L;
}

// ---- Philox-4x32-10 (philox.h), counter (pixel, 0, stream, 0), key = the two halves of the seed -------------------------
__device__ __forceinline__ float draw_normal(uint64_t seed, unsigned pixel) {
  const uint4 r = philox4x32_10(make_uint4(pixel, 0u, 0u, 0u), make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  // 24-bit uniforms strictly inside (0, 1): exact in fp32
  const float u1 = ((float)(r.x >> 8) + 0.5f) * 5.9604644775390625e-8f;
  const float u2 = ((float)(r.y >> 8) + 0.5f) * 5.9604644775390625e-8f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__device__ __forceinline__ unsigned draw_key(uint64_t seed, unsigned pixel) {
  return philox4x32_10(make_uint4(pixel, 0u, 1u, 0u), make_uint2((unsigned)seed, (unsigned)(seed >> 32))).x;
}

// ---- small block-wide helpers -------------------------------------------------------------------------------------
__device__ __forceinline__ bool valid_rgb(const mgs_keyframe_seed_args& A, int i, int HW) {
  return add_rn(add_rn(A.image[i], A.image[HW + i]), A.image[2 * (size_t)HW + i]) > A.rgb_boundary_threshold;
}

__device__ __forceinline__ bool prior_valid(float d, float o, bool rgb) { return d > 0.f && o > 0.95f && rgb; }

__device__ __forceinline__ bool depth_usable(float d, float trunc) { return d > 0.f && d <= trunc; }

// rank of the K-th smallest key, K = floor(n / downsample) as Python's int(n / downsample) (a double division)
struct SubsampleRank {
  float downsample;
  __device__ int count(int total) const { return (int)floor((double)total / (double)downsample); }
  __device__ int operator()(int total) const { return count(total) - 1; }
};

// ---- mode 0: the median of the valid depths -------------------------------------------------------------------------
template <int PASS>
__global__ __launch_bounds__(kSeedThreads) void k_seed_prior(const mgs_keyframe_seed_args A, const SeedScratch S) {
  __shared__ int s_hist[kRadixHist1];
  __shared__ int s_scan[kSeedWaves];
  __shared__ int s_sel[3];
  const int tid = threadIdx.x, HW = A.width * A.height;
  constexpr int nb = radix_level_buckets(PASS);
  for (int b = tid; b < nb; b += kSeedThreads) s_hist[b] = 0;
  RadixSelected sel{0u, 0, 0, true};
  if (PASS >= 2) sel = radix_select<kSeedThreads>(S.prior, PASS - 1, LowerMedianRank{}, s_scan, s_sel);   // ends in a barrier
  else __syncthreads();
  if (sel.any) {
    for (int base = blockIdx.x * kSeedStep; base < HW; base += gridDim.x * kSeedStep) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = base + j * kSeedThreads + tid;
        const bool in = i < HW;
        const float d = in ? A.depth[i] : 0.f;
        const bool ok = in && prior_valid(d, A.opacity[i], valid_rgb(A, i, HW));
        const RadixBucket rb = radix_level<PASS>(__float_as_uint(d), sel.prefix);
        if (PASS == 1) radix_hist_add_aggregated(s_hist, ok, rb.bucket);
        else if (ok && rb.counts) atomicAdd(&s_hist[rb.bucket], 1);
      }
    }
  }
  __syncthreads();
  radix_hist_flush<kSeedThreads>(s_hist, S.prior.level(PASS), nb);
}

// fp64 sums of (d - med) and (d - med)^2 over the valid depths: one partial per workgroup, summed lane tree -> wave
// order -> (in k_seed_prepare) workgroup tree.  Shifting by the median keeps the cancellation in S2 - S1^2 / n benign.
__global__ __launch_bounds__(kSeedThreads) void k_seed_moments(const mgs_keyframe_seed_args A, const SeedScratch S) {
  __shared__ int s_scan[kSeedWaves];
  __shared__ int s_sel[3];
  __shared__ double s_red[2][kSeedWaves];
  const int tid = threadIdx.x, HW = A.width * A.height;
  const RadixSelected sel = radix_select<kSeedThreads>(S.prior, 3, LowerMedianRank{}, s_scan, s_sel);
  const float med = sel.any ? __uint_as_float(sel.prefix) : __uint_as_float(0x7fc00000u);
  double s1 = 0.0, s2 = 0.0;
  if (sel.total >= 2) {
    for (int base = blockIdx.x * kSeedStep; base < HW; base += gridDim.x * kSeedStep) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = base + j * kSeedThreads + tid;
        if (i < HW) {
          const float d = A.depth[i];
          if (prior_valid(d, A.opacity[i], valid_rgb(A, i, HW))) {
            const double x = (double)d - (double)med;
            s1 += x;
            s2 += x * x;
          }
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
  }
  if ((tid & 63) == 0) { s_red[0][tid >> 6] = s1; s_red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < kSeedWaves; w++) { a += s_red[0][w]; b += s_red[1][w]; }
    S.moments[2 * blockIdx.x] = a;
    S.moments[2 * blockIdx.x + 1] = b;
    if (blockIdx.x == 0) {
      S.state->med = med;
      S.state->n_valid = sel.total;
      S.state->prior_ok = sel.total >= 2 ? 1 : 0;
    }
  }
}

// ---- the prepared depth map, the keys, level 1 of the two selects ---------------------------------------------------
__global__ __launch_bounds__(kSeedThreads) void k_seed_prepare(const mgs_keyframe_seed_args A, const SeedScratch S) {
  __shared__ int s_all[kRadixHist1];
  __shared__ int s_key[kRadixHist1];
  __shared__ double s_red[2][kSeedWaves];
  __shared__ int s_bad[kSeedWaves];
  __shared__ float s_std;
  const int tid = threadIdx.x, HW = A.width * A.height;
  for (int b = tid; b < kRadixHist1; b += kSeedThreads) { s_all[b] = 0; s_key[b] = 0; }
  __syncthreads();   // in every mode: no wave adds to a bucket that another wave has yet to clear
  float med = 0.f, std = 0.f;
  bool prior_ok = false;
  if (A.mode == 0) {
    // the moments' workgroup tree: thread t takes workgroup t's partial (hb <= 256), xor tree, waves in order
    double s1 = tid < S.hb ? S.moments[2 * tid] : 0.0, s2 = tid < S.hb ? S.moments[2 * tid + 1] : 0.0;
    for (int off = 32; off > 0; off >>= 1) {
      s1 += __shfl_xor(s1, off);
      s2 += __shfl_xor(s2, off);
    }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = s1; s_red[1][tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) {
      double a = 0.0, b = 0.0;
      for (int w = 0; w < kSeedWaves; w++) { a += s_red[0][w]; b += s_red[1][w]; }
      const double n = (double)S.state->n_valid;
      const double var = (b - a * a / n) / (n - 1.0);
      s_std = S.state->prior_ok ? (float)sqrt(var > 0.0 ? var : 0.0) : __uint_as_float(0x7fc00000u);
      if (blockIdx.x == 0) S.state->std = s_std;
    }
    __syncthreads();
    med = S.state->med;
    std = s_std;
    prior_ok = S.state->prior_ok != 0;
  }
  const float hi = add_rn(med, std), lo = sub_rn(med, std);
  const float sig_bad = mul_rn(std, 0.5f), sig_ok = mul_rn(std, 0.2f);
  int n_bad = 0;
  for (int base = blockIdx.x * kSeedStep; base < HW; base += gridDim.x * kSeedStep) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = base + j * kSeedThreads + tid;
      const bool in = i < HW;
      float d = 0.f;
      unsigned key = 0u;
      if (in) {
        const bool rgb = valid_rgb(A, i, HW);
        if (A.mode == 2) {
          d = A.depth[i];
        } else if (A.mode == 1) {
          const float nz = A.noise ? A.noise[i] : draw_normal(A.seed, (unsigned)i);
          d = add_rn(2.f, mul_rn(nz, 0.3f));
        } else if (!prior_ok) {
          d = 2.f;
        } else {
          const float nz = A.noise ? A.noise[i] : draw_normal(A.seed, (unsigned)i);
          d = A.depth[i];
          const bool bad = d > hi || d < lo || !prior_valid(d, A.opacity[i], rgb);
          n_bad += bad ? 1 : 0;
          d = add_rn(bad ? med : d, mul_rn(nz, bad ? sig_bad : sig_ok));
        }
        // no image content (add_new_keyframe's first-keyframe branch returns before that mask: mode 1 keeps every
        // pixel); a non-finite depth is no depth; -0 -> +0
        if ((!rgb && A.mode != 1) || !isfinite(d) || d == 0.f) d = 0.f;
        key = A.keys ? A.keys[i] : draw_key(A.seed, (unsigned)i);
        S.d[i] = d;
        S.keys[i] = key;
      }
      radix_hist_add_aggregated(s_all, in, radix_level<1>(float_order_key(d), 0u).bucket);
      if (in && depth_usable(d, A.depth_trunc)) atomicAdd(&s_key[radix_level<1>(key, 0u).bucket], 1);
    }
  }
  if (A.mode == 0) {
    for (int off = 32; off > 0; off >>= 1) n_bad += __shfl_xor(n_bad, off);
    if ((tid & 63) == 0) s_bad[tid >> 6] = n_bad;
  }
  __syncthreads();
  if (A.mode == 0 && tid == 0) {
    int t = 0;
    for (int w = 0; w < kSeedWaves; w++) t += s_bad[w];
    if (t) atomicAdd(&S.state->n_outliers, t);
  }
  radix_hist_flush<kSeedThreads>(s_all, S.all.h1, kRadixHist1);
  radix_hist_flush<kSeedThreads>(s_key, S.key.h1, kRadixHist1);
}

// Levels 2 and 3 of both selects: the rank (H*W - 1) / 2 of the depth map's order keys, the rank K - 1 of the
// sampling keys of the usable pixels.
template <int PASS>
__global__ __launch_bounds__(kSeedThreads) void k_seed_level(const mgs_keyframe_seed_args A, const SeedScratch S) {
  __shared__ int s_all[kRadixHist1];
  __shared__ int s_key[kRadixHist1];
  __shared__ int s_scan[kSeedWaves];
  __shared__ int s_sel[3];
  const int tid = threadIdx.x, HW = A.width * A.height;
  constexpr int nb = radix_level_buckets(PASS);
  for (int b = tid; b < nb; b += kSeedThreads) { s_all[b] = 0; s_key[b] = 0; }
  const RadixSelected sa = radix_select<kSeedThreads>(S.all, PASS - 1, LowerMedianRank{}, s_scan, s_sel);
  // ends in a barrier: both histograms are clear before any wave adds to them
  const RadixSelected sk = radix_select<kSeedThreads>(S.key, PASS - 1, SubsampleRank{A.downsample}, s_scan, s_sel);
  for (int base = blockIdx.x * kSeedStep; base < HW; base += gridDim.x * kSeedStep) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = base + j * kSeedThreads + tid;
      if (i >= HW) continue;
      const float d = S.d[i];
      const RadixBucket ba = radix_level<PASS>(float_order_key(d), sa.prefix);
      if (ba.counts) atomicAdd(&s_all[ba.bucket], 1);
      if (sk.any && depth_usable(d, A.depth_trunc)) {
        const RadixBucket bk = radix_level<PASS>(S.keys[i], sk.prefix);
        if (bk.counts) atomicAdd(&s_key[bk.bucket], 1);
      }
    }
  }
  __syncthreads();
  radix_hist_flush<kSeedThreads>(s_all, S.all.level(PASS), nb);
  radix_hist_flush<kSeedThreads>(s_key, S.key.level(PASS), nb);
}

// Per wave segment: how many usable pixels lie below / at the key threshold; how many values are <= the lower middle
// order statistic of d and the smallest order key above it.
__global__ __launch_bounds__(kSeedThreads) void k_seed_count(const mgs_keyframe_seed_args A, const SeedScratch S) {
  __shared__ int s_scan[kSeedWaves];
  __shared__ int s_sel[3];
  const int tid = threadIdx.x, lane = tid & 63, HW = A.width * A.height;
  const RadixSelected sa = radix_select<kSeedThreads>(S.all, 3, LowerMedianRank{}, s_scan, s_sel);
  const SubsampleRank sub{A.downsample};
  const RadixSelected sk = radix_select<kSeedThreads>(S.key, 3, sub, s_scan, s_sel);
  if (blockIdx.x == 0 && tid == 0) {
    S.state->all_lo = sa.prefix;
    S.state->key_thr = sk.any ? sk.prefix : 0u;
    S.state->key_rank = sk.any ? sk.rank : -1;
    S.state->n_depth = sk.total;
    S.state->K = sk.any ? sub.count(sk.total) : 0;
  }
  const int seg = blockIdx.x * kSeedWaves + (tid >> 6);
  if (seg >= S.n_seg) return;
  const int p0 = seg * S.seg_len, p1 = min(HW, p0 + S.seg_len);
  int below = 0, at = 0, le = 0;
  unsigned above = 0xffffffffu;
  for (int i0 = p0; i0 < p1; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < p1;
    const float d = in ? S.d[i] : 0.f;
    const unsigned k = in ? S.keys[i] : 0u;
    const unsigned m = float_order_key(d);
    const bool use = in && sk.any && depth_usable(d, A.depth_trunc);
    below += __popcll(__ballot(use && k < sk.prefix));
    at += __popcll(__ballot(use && k == sk.prefix));
    le += __popcll(__ballot(in && m <= sa.prefix));
    if (in && m > sa.prefix) above = min(above, m);
  }
  for (int off = 32; off > 0; off >>= 1) above = min(above, (unsigned)__shfl_xor((int)above, off));
  if (lane == 0) S.seg[seg] = make_int4(below, at, le, (int)above);
}

// Scan of the segment counts, then every wave compacts its segment in pixel order and writes its rows.
__global__ __launch_bounds__(kSeedThreads) void k_seed_emit(const mgs_keyframe_seed_args A, const SeedScratch S) {
  __shared__ int s_below[kSeedMaxSegments + 1];   // exclusive prefix per segment
  __shared__ int s_at[kSeedMaxSegments + 1];
  __shared__ int s_w[4][kSeedWaves];
  __shared__ float s_cam[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, HW = A.width * A.height;
  // thread t owns segments 4t .. 4t + 3 (n_seg <= 1024)
  int4 c[4];
  int sb = 0, sa = 0, sle = 0;
  unsigned above = 0xffffffffu;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int g = 4 * tid + j;
    c[j] = g < S.n_seg ? S.seg[g] : make_int4(0, 0, 0, -1);
    sb += c[j].x;
    sa += c[j].y;
    sle += c[j].z;
    above = min(above, (unsigned)c[j].w);
  }
  int ib = sb, ia = sa;
  for (int off = 1; off < 64; off <<= 1) {
    const int vb = __shfl_up(ib, off), va = __shfl_up(ia, off);
    if (lane >= off) { ib += vb; ia += va; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sle += __shfl_xor(sle, off);
    above = min(above, (unsigned)__shfl_xor((int)above, off));
  }
  if (lane == 63) { s_w[0][wv] = ib; s_w[1][wv] = ia; s_w[2][wv] = sle; s_w[3][wv] = (int)above; }
  if (tid < 16) s_cam[tid] = A.T[tid];
  __syncthreads();
  int base_b = 0, base_a = 0;
  for (int w = 0; w < wv; w++) { base_b += s_w[0][w]; base_a += s_w[1][w]; }
  int eb = base_b + ib - sb, ea = base_a + ia - sa;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    s_below[4 * tid + j] = eb;
    s_at[4 * tid + j] = ea;
    eb += c[j].x;
    ea += c[j].y;
  }
  __syncthreads();
  const SeedState st = *S.state;
  if (blockIdx.x == 0 && tid == 0) {
    int le = 0;
    unsigned ab = 0xffffffffu;
    for (int w = 0; w < kSeedWaves; w++) { le += s_w[2][w]; ab = min(ab, (unsigned)s_w[3][w]); }
    // NumPy's median: the lower middle order statistic, averaged (in fp32) with the next one when H*W is even
    const float v_lo = float_from_order_key(st.all_lo);
    float med_all = v_lo;
    if ((HW & 1) == 0) {
      const float v_hi = le > HW / 2 ? v_lo : float_from_order_key(ab);
      med_all = mul_rn(add_rn(v_lo, v_hi), 0.5f);
    }
    double ps = A.point_size;
    if (A.adaptive_pointsize) {
      ps = A.point_size * (double)med_all;
      ps = ps < 0.05 ? ps : 0.05;     // Python's min(0.05, x): a NaN x gives 0.05
    }
    mgs_keyframe_seed_result* R = static_cast<mgs_keyframe_seed_result*>(A.result);
    const float nan = __uint_as_float(0x7fc00000u);
    R->num_points = st.K;
    R->n_valid = A.mode == 0 ? st.n_valid : 0;
    R->n_outliers = A.mode == 0 ? st.n_outliers : 0;
    R->n_depth = st.n_depth;
    R->median_depth = A.mode == 0 ? st.med : nan;
    R->std_depth = A.mode == 0 ? st.std : nan;
    R->median_all = med_all;
    R->point_size = (float)ps;
  }
  const int seg = blockIdx.x * kSeedWaves + wv;
  if (seg >= S.n_seg || st.K <= 0) return;
  const int keep_at = st.key_rank + 1;
  int nb = s_below[seg], na = s_at[seg];
  const float ea_ = add_rn(fabsf(A.exposure_a[0]), A.exposure_eps), eb_ = A.exposure_b[0];
  const int p0 = seg * S.seg_len, p1 = min(HW, p0 + S.seg_len);
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int i0 = p0; i0 < p1; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < p1;
    const float z = in ? S.d[i] : 0.f;
    const unsigned k = in ? S.keys[i] : 0u;
    const bool use = in && depth_usable(z, A.depth_trunc);
    const bool below = use && k < st.key_thr, at = use && k == st.key_thr;
    const unsigned long long mb = __ballot(below), ma = __ballot(at);
    const int rank_at = na + __popcll(ma & lt);
    const bool keep = below || (at && rank_at < keep_at);
    const int row = nb + __popcll(mb & lt) + min(rank_at, keep_at);
    if (keep && row < A.row_capacity) {
      const float u = (float)(i % A.width), v = (float)(i / A.width);
      const float px = (u - A.cx) * z / A.fx - s_cam[3], py = (v - A.cy) * z / A.fy - s_cam[7], pz = z - s_cam[11];
#pragma unroll
      for (int cdim = 0; cdim < 3; cdim++) {
        A.xyz[3 * (size_t)row + cdim] = px * s_cam[cdim] + py * s_cam[4 + cdim] + pz * s_cam[8 + cdim];
        // as separate roundings: a contracted fma could move a value across floor()'s step
        const float img = add_rn(mul_rn(ea_, A.image[(size_t)cdim * HW + i]), eb_);
        const float col = floorf(mul_rn(fminf(fmaxf(img, 0.f), 1.f), 255.f)) / 255.f;
        A.features_dc[3 * (size_t)row + cdim] = (col - 0.5f) / kSH_C0;
      }
      A.rots[4 * (size_t)row] = 1.f;
      A.rots[4 * (size_t)row + 1] = 0.f;
      A.rots[4 * (size_t)row + 2] = 0.f;
      A.rots[4 * (size_t)row + 3] = 0.f;
      A.opacity_logit[row] = 0.f;      // inverse_sigmoid(0.5)
      if (A.pixel_index) A.pixel_index[row] = i;
    }
    nb += __popcll(mb);
    na += __popcll(ma);
  }
}

__global__ __launch_bounds__(kSeedThreads) void k_seed_scale(const float* __restrict__ dist2, int n, int dims,
                                                             const mgs_keyframe_seed_result* __restrict__ rec,
                                                             float* __restrict__ log_scales) {
  const int p = blockIdx.x * kSeedThreads + threadIdx.x;
  if (p >= n) return;
  const float s = logf(sqrtf(fmaxf(dist2[p], 1e-7f) * rec->point_size));
  for (int c = 0; c < dims; c++) log_scales[(size_t)p * dims + c] = s;
}

int hist_blocks(int num_pixels) {
  const int b = (num_pixels + kSeedStep - 1) / kSeedStep;
  return b < 1 ? 1 : (b > kSeedMaxBlocks ? kSeedMaxBlocks : b);
}

}  // namespace

uint64_t keyframe_seed_scratch_bytes(int num_pixels, int row_capacity) {
  return seed_layout(num_pixels, row_capacity).bytes;
}

int launch_keyframe_seed(const mgs_keyframe_seed_args& A, hipStream_t st) {
  const int HW = A.width * A.height;
  const SeedLayout L = seed_layout(HW, A.row_capacity);
  char* w = static_cast<char*>(A.scratch);
  SeedScratch S{};
  S.state = reinterpret_cast<SeedState*>(w + L.state);
  int* h = reinterpret_cast<int*>(w + L.hists);
  S.prior = radix_hists_at(h);
  S.all = radix_hists_at(h + kRadixHistInts);
  S.key = radix_hists_at(h + 2 * kRadixHistInts);
  S.moments = reinterpret_cast<double*>(w + L.moments);
  S.seg = reinterpret_cast<int4*>(w + L.seg);
  S.d = A.depth_out ? A.depth_out : reinterpret_cast<float*>(w + L.d);
  S.keys = reinterpret_cast<unsigned*>(w + L.keys);
  S.dist2 = reinterpret_cast<float*>(w + L.dist2);
  S.knn = w + L.knn;
  S.hb = hist_blocks(HW);
  S.seg_len = ((HW + kSeedMaxSegments - 1) / kSeedMaxSegments + 63) / 64 * 64;
  S.n_seg = (HW + S.seg_len - 1) / S.seg_len;
  const dim3 block(kSeedThreads), hgrid(S.hb), sgrid((S.n_seg + kSeedWaves - 1) / kSeedWaves);
  if (!hip_ok("keyframe seed memset", hipMemsetAsync(w, 0, L.zero_bytes, st))) { launches_ok(); return MGS_ERR_LAUNCH; }
  if (A.mode == 0) {
    launch("seed_prior1", k_seed_prior<1>, hgrid, block, st, A, S);
    launch("seed_prior2", k_seed_prior<2>, hgrid, block, st, A, S);
    launch("seed_prior3", k_seed_prior<3>, hgrid, block, st, A, S);
    launch("seed_moments", k_seed_moments, hgrid, block, st, A, S);
  }
  launch("seed_prepare", k_seed_prepare, hgrid, block, st, A, S);
  launch("seed_level2", k_seed_level<2>, hgrid, block, st, A, S);
  launch("seed_level3", k_seed_level<3>, hgrid, block, st, A, S);
  launch("seed_count", k_seed_count, sgrid, block, st, A, S);
  launch("seed_emit", k_seed_emit, sgrid, block, st, A, S);
  if (!launches_ok()) return MGS_ERR_LAUNCH;
  // the one host read: K sizes the k-nn launcher's kernel choice and slice plan (and the caller's append)
  mgs_keyframe_seed_result* host = A.result_host;
  if (!hip_ok("keyframe seed record copy", hipMemcpyAsync(host, A.result, sizeof(*host), hipMemcpyDeviceToHost, st)) ||
      !hip_ok("keyframe seed record sync", hipStreamSynchronize(st))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  const int K = host->num_points;
  if (K <= 0) return MGS_OK;
  if (K > A.row_capacity) return MGS_ERR_LAUNCH;   // cannot happen: K <= floor(H*W / downsample) <= row_capacity
  const int rc = launch_knn(A.xyz, K, S.dist2, S.knn, st);
  if (rc != MGS_OK) return rc;
  launch("seed_scale", k_seed_scale, dim3((K + kSeedThreads - 1) / kSeedThreads), block, st, (const float*)S.dist2, K,
         A.isotropic ? 1 : 3, (const mgs_keyframe_seed_result*)A.result, A.log_scales);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace mgs
