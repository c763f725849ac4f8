// Keyframe selection and window management on the device (mgs_keyframe_decide; DESIGN.md "Keyframe policy on the
// device").  The reference frontend's per-frame decision - is_keyframe (utils/slam_frontend.py:1692-1720),
// add_to_window (:1722-1783) and the run loop around them (:1914-1956) - with get_median_depth
// (utils/slam_utils.py:286-297) of the frame's final tracking render, in three stream-ordered launches:
//
//   k_kf_pass<1>  blocks [0, bp): level 1 of the radix select (radix_select.h) of the lower median of the valid depths
//                 (depth > 0 && opacity > 0.95; NaN fails both).  Blocks [bp, bp + bc): covisibility counts
//                 |cur|, |row_w|, |cur & row_w| over the N Gaussians (4 per lane and step: an int4 of n_touched, a
//                 uint32 of every row), one 33-int partial per workgroup.
//   k_kf_pass<2>  level 2: every workgroup repeats level 1's search, rank k = (n - 1) / 2.
//   k_kf_pass<3>  level 3; the workgroup that takes the last ticket selects the final bucket - the lower median's bit
//                 pattern, exactly torch.median's value - sums the count partials and evaluates the decision in one
//                 thread, in the reference's order of operations.
// No grid-wide barrier, no spinning, no float atomics: two calls give bit-identical records.  The scratch's histograms
// and ticket are zero on entry and are restored to zero by the last workgroup.
#include <hip/hip_runtime.h>
#include <math.h>

#include "launch.h"
#include "radix_select.h"
#include "raster_kernels.h"

namespace mgs {
namespace {

constexpr int kKfThreads = 256;
constexpr int kKfMaxBlocks = 256;
constexpr int kKfCounts = 1 + 2 * MGS_KF_MAX_WINDOW;   // |cur|, |row_w| x 16, |cur & row_w| x 16

__device__ __forceinline__ bool depth_valid(float d, float o) { return d > 0.f && o > 0.95f; }

// |translation of Ti Tj^-1|, both row-major world-to-camera rigid motions: Tj^-1 = [Rj^T | -Rj^T tj].
__device__ float rel_translation_norm(const float* Ti, const float* Tj) {
  float u[3];
#pragma unroll
  for (int c = 0; c < 3; c++) u[c] = Tj[0 * 4 + c] * Tj[3] + Tj[1 * 4 + c] * Tj[7] + Tj[2 * 4 + c] * Tj[11];
  float v[3];
#pragma unroll
  for (int r = 0; r < 3; r++) v[r] = Ti[r * 4 + 3] - (Ti[r * 4 + 0] * u[0] + Ti[r * 4 + 1] * u[1] + Ti[r * 4 + 2] * u[2]);
  return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

constexpr int kKfPoses = MGS_KF_MAX_WINDOW + 1;   // pose 0 = the current frame, 1 + w = window[w]

// The covisibility counts of one workgroup's share of the Gaussians -> partials[cb * kKfCounts + c].
__device__ void count_block(const mgs_keyframe_args& A, const KfScratch& S, int cb) {
  const int tid = threadIdx.x, N = A.num_gaussians, W = A.window_len;
  int c_cur = 0, c_row[MGS_KF_MAX_WINDOW], c_int[MGS_KF_MAX_WINDOW];
#pragma unroll
  for (int w = 0; w < MGS_KF_MAX_WINDOW; w++) { c_row[w] = 0; c_int[w] = 0; }
  const int n4 = (N + 3) >> 2;
  for (int q = cb * kKfThreads + tid; q < n4; q += S.bc * kKfThreads) {
    const bool whole = 4 * q + 3 < N;
    unsigned cm = 0;
    if (whole && S.vec_touched) {
      const int4 t = reinterpret_cast<const int4*>(A.n_touched)[q];
      cm = (unsigned)(t.x > 0) | (unsigned)(t.y > 0) << 1 | (unsigned)(t.z > 0) << 2 | (unsigned)(t.w > 0) << 3;
    } else {
      for (int j = 0; j < 4; j++)
        if (4 * q + j < N && A.n_touched[4 * q + j] > 0) cm |= 1u << j;
    }
    c_cur += __popc(cm);
#pragma unroll
    for (int w = 0; w < MGS_KF_MAX_WINDOW; w++) {
      if (w < W) {
        const uint8_t* row = A.visibility[w];
        unsigned rm = 0;
        if (whole && S.vec_rows) {
          const unsigned x = reinterpret_cast<const unsigned*>(row)[q];
          rm = (unsigned)((x & 0xffu) != 0) | (unsigned)((x & 0xff00u) != 0) << 1 |
               (unsigned)((x & 0xff0000u) != 0) << 2 | (unsigned)((x & 0xff000000u) != 0) << 3;
        } else {
          for (int j = 0; j < 4; j++)
            if (4 * q + j < N && row[4 * q + j] != 0) rm |= 1u << j;
        }
        c_row[w] += __popc(rm);
        c_int[w] += __popc(rm & cm);
      }
    }
  }
  __shared__ int s_red[kKfCounts][kKfThreads / 64];
  const int lane = tid & 63, wv = tid >> 6;
  auto wave_sum = [](int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
  };
  const int tc = wave_sum(c_cur);
  if (lane == 0) s_red[0][wv] = tc;
#pragma unroll
  for (int w = 0; w < MGS_KF_MAX_WINDOW; w++) {
    if (w < W) {
      const int r = wave_sum(c_row[w]), x = wave_sum(c_int[w]);
      if (lane == 0) { s_red[1 + w][wv] = r; s_red[1 + MGS_KF_MAX_WINDOW + w][wv] = x; }
    }
  }
  __syncthreads();
  if (tid < kKfCounts) {
    int s = 0;
    const bool used = tid == 0 || ((tid - 1) % MGS_KF_MAX_WINDOW) < W;
    if (used)
      for (int w = 0; w < kKfThreads / 64; w++) s += s_red[tid][w];
    S.partials[cb * kKfCounts + tid] = s;
  }
}

// The reference's decision from the exact counts, the median and the table of pose distances
// rel[i][j] = |t(T_i T_j^-1)| (0 = the current frame, 1 + w = window[w]); one thread, stores straight to *result.
__device__ void decide(const mgs_keyframe_args& A, const int* cnt, int n_valid, float med,
                       const float (*rel)[kKfPoses]) {
  mgs_keyframe_result* R = static_cast<mgs_keyframe_result*>(A.result);
  const int W = A.window_len;
  const int n_cur = cnt[0];
  float ss[MGS_KF_MAX_WINDOW];
  R->n_valid = n_valid;
  R->median_depth = med;
  R->window_len = W;
  R->n_cur = n_cur;
  for (int w = 0; w < MGS_KF_MAX_WINDOW; w++) {
    const int nr = w < W ? cnt[1 + w] : 0, ni = w < W ? cnt[1 + MGS_KF_MAX_WINDOW + w] : 0;
    R->n_row[w] = nr;
    R->n_inter[w] = ni;
    // szymkiewicz-simpson coefficient (:1735-1741): int / int true division in fp32 (exact: counts < 2^24)
    ss[w] = w < W ? (float)ni / (float)(n_cur < nr ? n_cur : nr) : 0.f;
    R->ss_ratio[w] = ss[w];
    R->score[w] = -1.0;
  }
  // is_keyframe (:1692-1720)
  const float dist = rel[0][1];
  const bool dist_check = dist > A.kf_translation * med;
  const bool dist_check2 = dist > A.kf_min_translation * med;
  const int n_row0 = cnt[1], n_int0 = cnt[1 + MGS_KF_MAX_WINDOW];
  const float overlap = (float)n_int0 / (float)(n_cur + n_row0 - n_int0);   // intersection / union
  const bool is_kf = (overlap < A.kf_overlap && dist_check2) || dist_check;
  R->dist = dist;
  R->overlap = overlap;
  R->flags = (dist_check ? 1 : 0) | (dist_check2 ? 2 : 0) | (is_kf ? 4 : 0);
  // the run loop (:1914-1938)
  bool create = is_kf;
  if (W < A.window_size) create = A.check_time && overlap < A.kf_overlap;
  if (A.single_thread) create = A.check_time && create;
  int cut = -1, evict = -1;
  if (create) {
    // add_to_window: window = [cur] + window; its positions >= 2 (input positions >= 1) are tested and the LAST one at
    // or below the cutoff is removed
    const float cut_off = A.initialized ? A.kf_cutoff : 0.4f;
#pragma unroll
    for (int w = 1; w < MGS_KF_MAX_WINDOW; w++)
      if (w < W && ss[w] <= cut_off) cut = w;
    const int len = 1 + W - (cut >= 0 ? 1 : 0);
    // input position of new-window position a >= 1
    auto at = [cut](int a) { return a - 1 + (cut >= 0 && a - 1 >= cut ? 1 : 0); };
    if (len > A.window_size) {
      // inverse-distance eviction over positions >= 2: fp32 norms, fp64 reciprocals / sums / products (.item())
      int best = -1;
      double best_s = 0.0;
      bool best_nan = false;
      for (int a = 2; a < len; a++) {
        const int i = 1 + at(a);
        double s = 0.0;
        for (int b = 2; b < len; b++) {
          if (b == a) continue;
          const float d = rel[i][1 + at(b)] + 1e-6f;
          s += 1.0 / (double)d;
        }
        const float k = sqrtf(rel[i][0]);
        const double sc = (double)k * s;
        R->score[at(a)] = sc;
        // np.argmax: the first maximum; a NaN wins (the first one)
        if (!best_nan && (best < 0 || isnan(sc) || sc > best_s)) { best = a; best_s = sc; best_nan = isnan(sc); }
      }
      evict = at(best);
    }
  }
  const int removed = evict >= 0 ? evict : cut;
  R->create_kf = create ? 1 : 0;
  R->removed_cutoff = cut;
  R->removed_evict = evict;
  R->removed = removed;
  R->reset = (create && A.monocular && !A.initialized && removed >= 0) ? 1 : 0;
}

template <int PASS>
__global__ __launch_bounds__(kKfThreads) void k_kf_pass(const mgs_keyframe_args A, const KfScratch S) {
  const int tid = threadIdx.x;
  if (PASS == 1 && (int)blockIdx.x >= S.bp) {
    count_block(A, S, blockIdx.x - S.bp);
    return;
  }
  __shared__ int s_hist[kRadixHist1];
  __shared__ int s_scan[kKfThreads / 64];
  __shared__ int s_sel[3];
  constexpr int nb = radix_level_buckets(PASS);
  for (int b = tid; b < nb; b += kKfThreads) s_hist[b] = 0;
  // prologue: the bucket (prefix) that holds the median rank
  RadixSelected sel{0u, 0, 0, true};
  if (PASS >= 2) sel = radix_select<kKfThreads>(S.hist, PASS - 1, LowerMedianRank{}, s_scan, s_sel);   // ends in a barrier
  else __syncthreads();
  if (sel.any) {
    const int HW = A.num_pixels, n4 = (HW + 3) >> 2;
    for (int q = blockIdx.x * kKfThreads + tid; q < n4; q += S.bp * kKfThreads) {
      float d[4], o[4];
      if (S.vec_pixels && 4 * q + 3 < HW) {
        const float4 dv = reinterpret_cast<const float4*>(A.depth)[q];
        const float4 ov = reinterpret_cast<const float4*>(A.opacity)[q];
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
        o[0] = ov.x; o[1] = ov.y; o[2] = ov.z; o[3] = ov.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const bool in = 4 * q + j < HW;
          d[j] = in ? A.depth[4 * q + j] : 0.f;
          o[j] = in ? A.opacity[4 * q + j] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool ok = depth_valid(d[j], o[j]);
        const RadixBucket rb = radix_level<PASS>(__float_as_uint(d[j]), sel.prefix);
        if (PASS == 1) radix_hist_add_aggregated(s_hist, ok, rb.bucket);
        else if (ok && rb.counts) atomicAdd(&s_hist[rb.bucket], 1);
      }
    }
  }
  __syncthreads();
  radix_hist_flush<kKfThreads>(s_hist, S.hist.level(PASS), nb);
  if (PASS != 3) return;
  // ---- the last workgroup: the median's last bits, the counts, the decision; then the scratch is zeroed again
  // the barrier orders every lane's increments before lane 0's agent-scope release and ticket (as k_ssim_loss); one
  // fence per workgroup, not per lane: an agent-scope fence writes back L2
  __syncthreads();
  __shared__ int s_last;
  if (tid == 0) {
    __threadfence();
    s_last = atomicAdd(S.ticket, 1) == (int)gridDim.x - 1;
    if (s_last) __threadfence();
  }
  __syncthreads();
  if (!s_last) return;
  const int n_valid = sel.total;
  float med = __uint_as_float(0x7fc00000u);   // NaN: torch.median of an empty selection
  if (sel.any) {
    block_select<kKfThreads, kRadixHist3 / kKfThreads>(S.hist.h3, sel.rank, s_scan, s_sel);
    med = __uint_as_float(sel.prefix << 10 | (unsigned)s_sel[0]);
  }
  // count partials: thread t loads workgroup t's 33 ints (independent loads, bc <= 256), then wave and block sums
  __shared__ int s_part[kKfCounts][kKfThreads / 64];
  __shared__ int s_cnt[kKfCounts];
  {
    int v[kKfCounts];
#pragma unroll
    for (int c = 0; c < kKfCounts; c++) v[c] = tid < S.bc ? S.partials[tid * kKfCounts + c] : 0;
#pragma unroll
    for (int c = 0; c < kKfCounts; c++) {
      int x = v[c];
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
      if ((tid & 63) == 0) s_part[c][tid >> 6] = x;
    }
  }
  __syncthreads();
  if (tid < kKfCounts) {
    int x = 0;
    for (int w = 0; w < kKfThreads / 64; w++) x += s_part[tid][w];
    s_cnt[tid] = x;
  }
  __syncthreads();
  // the poses, then every pairwise distance the decision can need, in parallel
  __shared__ float s_T[kKfPoses][16];
  __shared__ float s_rel[kKfPoses][kKfPoses];
  const int np = 1 + A.window_len;
  for (int e = tid; e < np * 16; e += kKfThreads) s_T[e / 16][e % 16] = (e < 16 ? A.T_cur : A.T_window[e / 16 - 1])[e % 16];
  __syncthreads();
  for (int e = tid; e < np * np; e += kKfThreads) s_rel[e / np][e % np] = rel_translation_norm(s_T[e / np], s_T[e % np]);
  __syncthreads();
  if (tid == 0) decide(A, s_cnt, n_valid, med, s_rel);
  for (int b = tid; b < kRadixHistInts; b += kKfThreads) S.hist.h1[b] = 0;   // the triple is contiguous
  if (tid == 0) *S.ticket = 0;
}

int blocks_for(int64_t n) {
  const int64_t b = (n + 4 * kKfThreads - 1) / (4 * kKfThreads);
  return (int)(b < 1 ? 1 : (b > kKfMaxBlocks ? kKfMaxBlocks : b));
}

}  // namespace

KfLayout kf_layout(int num_gaussians, int num_pixels) {
  KfLayout L;
  uint64_t o = 0;
  L.bp = blocks_for(num_pixels);
  L.bc = blocks_for(num_gaussians);
  L.hists = o; o = align_up(o + (uint64_t)kRadixHistInts * 4);
  L.ticket = o; o = align_up(o + 4);
  L.partials = o; o = align_up(o + (uint64_t)L.bc * kKfCounts * 4);
  L.bytes = o;
  return L;
}

int launch_keyframe_decide(const mgs_keyframe_args& A, hipStream_t st) {
  const KfLayout L = kf_layout(A.num_gaussians, A.num_pixels);
  char* w = static_cast<char*>(A.scratch);
  KfScratch S{};
  S.hist = radix_hists_at(w + L.hists);
  S.ticket = reinterpret_cast<int*>(w + L.ticket);
  S.partials = reinterpret_cast<int*>(w + L.partials);
  S.bp = L.bp;
  S.bc = L.bc;
  auto aligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
  S.vec_pixels = aligned(A.depth, 16) && aligned(A.opacity, 16);
  S.vec_touched = aligned(A.n_touched, 16);
  S.vec_rows = 1;
  for (int w2 = 0; w2 < A.window_len; w2++) S.vec_rows &= aligned(A.visibility[w2], 4) ? 1 : 0;
  launch("kf_pass1_counts", k_kf_pass<1>, dim3(S.bp + S.bc), dim3(kKfThreads), st, A, S);
  launch("kf_pass2", k_kf_pass<2>, dim3(S.bp), dim3(kKfThreads), st, A, S);
  launch("kf_pass3_decide", k_kf_pass<3>, dim3(S.bp), dim3(kKfThreads), st, A, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace mgs
