// The exact element of rank k of a plane of 32-bit keys: the one radix select of the library.  Its users:
//   keyframe_policy.hip  the median depth of mgs_keyframe_decide;
//   keyframe_seed.hip    the depth prior's median, NumPy's median of the prepared depth map and the K-th smallest
//                        sampling key of mgs_keyframe_seed;
//   frame_prepare.hip    the median gradient intensity of mgs_frame_prepare, over the image and per 32x32 patch.
//
// A select runs three histogram levels (bits 31..21, 20..10, 9..0: 2048 / 2048 / 1024 buckets, radix_level); every
// workgroup of the next level repeats the search of the earlier levels' histograms itself (radix_select), so no
// grid-wide barrier and no spinning is needed.  Positive fp32 values order like their uint32 bit patterns (+inf
// included); float_order_key() extends that order to negative values.
#pragma once
#include <hip/hip_runtime.h>

namespace mgs {

constexpr int kRadixHist1 = 2048, kRadixHist2 = 2048, kRadixHist3 = 1024;

// Block-wide search of `hist` (THREADS * PER buckets) for the bucket holding rank k = rank_of(total).  rank_of gets
// the histogram's own total and returns the wanted rank, or a negative value for "none".
// s_out = {bucket or -1, rank inside it, total}; s_scan holds THREADS / 64 ints.  All threads call it.
template <int THREADS, int PER, class RankOf>
__device__ void block_select_by(const int* hist, RankOf rank_of, int* s_scan, int* s_out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int h[PER];
  int local = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    h[j] = __hip_atomic_load(&hist[tid * PER + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    local += h[j];
  }
  int incl = local;   // inclusive scan inside the wave
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  if (lane == 63) s_scan[wv] = incl;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < THREADS / 64; w++) {
    if (w < wv) base += s_scan[w];
    total += s_scan[w];
  }
  const int k = rank_of(total);
  const int excl = base + incl - local;
  if (tid == 0) { s_out[0] = -1; s_out[1] = 0; s_out[2] = total; }
  __syncthreads();
  if (total > 0 && k >= excl && k < excl + local) {
    int c = excl;
#pragma unroll
    for (int j = 0; j < PER; j++) {
      if (k >= c && k < c + h[j]) { s_out[0] = tid * PER + j; s_out[1] = k - c; }
      c += h[j];
    }
  }
  __syncthreads();
}

// Rank k, or (k < 0) the lower-median rank (total - 1) / 2 of the histogram's own total - torch.median's element.
// total == 0: k = 0, no bucket holds it.
template <int THREADS, int PER>
__device__ void block_select(const int* hist, int k, int* s_scan, int* s_out) {
  block_select_by<THREADS, PER>(hist, [k](int total) { return k < 0 ? (total - 1) / 2 : k; }, s_scan, s_out);
}

// ---- the pieces of a three-level select over global histograms, for kernels of THREADS threads -------------------------
constexpr int kRadixHistInts = kRadixHist1 + kRadixHist2 + kRadixHist3;   // ints of one histogram triple

// The three histograms of one select: contiguous, h1 first (a memset or one loop over kRadixHistInts clears them).
struct RadixHists {
  int *h1, *h2, *h3;
  __host__ __device__ int* level(int l) const { return l == 1 ? h1 : (l == 2 ? h2 : h3); }
};
inline RadixHists radix_hists_at(void* base) {
  int* h = static_cast<int*>(base);
  return RadixHists{h, h + kRadixHist1, h + kRadixHist1 + kRadixHist2};
}
constexpr int radix_level_buckets(int level) { return level == 1 ? kRadixHist1 : (level == 2 ? kRadixHist2 : kRadixHist3); }

// Level LEVEL's rule for one key: does it count (its bits above the level equal the prefix selected so far) and in
// which bucket.  Level 1 counts every key.
struct RadixBucket { bool counts; unsigned bucket; };
template <int LEVEL>
__device__ __forceinline__ RadixBucket radix_level(unsigned key, unsigned prefix) {
  static_assert(LEVEL >= 1 && LEVEL <= 3, "three levels");
  if (LEVEL == 1) return RadixBucket{true, key >> 21};
  if (LEVEL == 2) return RadixBucket{(key >> 21) == prefix, (key >> 10) & 2047u};
  return RadixBucket{(key >> 10) == prefix, key & 1023u};
}

// torch.median's element: the lower-median rank of the histogram's own total (0 when it is empty).
struct LowerMedianRank {
  __device__ int operator()(int total) const { return (total - 1) / 2; }
};

// The first `levels` levels of the select of rank rank_of(level 1's total), repeated by every workgroup.  prefix = the
// selected key's top bits (11, 22 or all 32), rank = the rank left inside that bucket, total = level 1's total;
// any = false when no element has the rank (an empty histogram, a negative rank): prefix and rank mean nothing then.
// s_scan holds THREADS / 64 ints, s_sel 3.  All threads call it; it ends in a barrier.
struct RadixSelected { unsigned prefix; int rank, total; bool any; };
template <int THREADS, class RankOf>
__device__ RadixSelected radix_select(const RadixHists& H, int levels, RankOf rank_of, int* s_scan, int* s_sel) {
  RadixSelected r;
  block_select_by<THREADS, kRadixHist1 / THREADS>(H.h1, rank_of, s_scan, s_sel);
  r.total = s_sel[2];
  r.any = s_sel[0] >= 0;
  r.prefix = (unsigned)s_sel[0];
  r.rank = s_sel[1];
  if (levels >= 2 && r.any) {
    const int k2 = r.rank;
    __syncthreads();
    block_select<THREADS, kRadixHist2 / THREADS>(H.h2, k2, s_scan, s_sel);
    r.prefix = r.prefix << 11 | (unsigned)s_sel[0];
    r.rank = s_sel[1];
    if (levels >= 3) {
      const int k3 = r.rank;
      __syncthreads();
      block_select<THREADS, kRadixHist3 / THREADS>(H.h3, k3, s_scan, s_sel);
      r.prefix = r.prefix << 10 | (unsigned)s_sel[0];
      r.rank = s_sel[1];
    }
  }
  __syncthreads();
  return r;
}

// One LDS increment per distinct bucket and wave: depths and image statistics share a few top-bit buckets.  All lanes
// call it.
__device__ __forceinline__ void radix_hist_add_aggregated(int* s_hist, bool ok, unsigned b) {
  unsigned long long pending = __ballot(ok);
  while (pending) {
    const unsigned lb = (unsigned)__shfl((int)b, __ffsll((long long)pending) - 1);
    const unsigned long long same = __ballot(ok && b == lb) & pending;
    if (ok && b == lb && __ffsll((long long)same) - 1 == (int)(threadIdx.x & 63)) atomicAdd(&s_hist[lb], __popcll(same));
    pending &= ~same;
  }
}

// The workgroup's LDS histogram into the global one: integer atomics, so the sum does not depend on arrival order.
template <int THREADS>
__device__ __forceinline__ void radix_hist_flush(const int* s_hist, int* out, int nb) {
  for (int b = threadIdx.x; b < nb; b += THREADS) {
    const int v = s_hist[b];
    if (v) atomicAdd(&out[b], v);
  }
}

// uint32 keys in the order of the floats they came from (negative values below positive ones; -0 below +0).
__device__ __forceinline__ unsigned float_order_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_from_order_key(unsigned m) {
  return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
}

}  // namespace mgs
