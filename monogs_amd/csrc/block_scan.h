// Scans over a workgroup of 256 threads, and the ONE-workgroup scan of block totals built on them (tsdf.hip, mesh_eval.hip
// and, through compact_scan.h, mesh_clean.hip and mesh_render.hip).  Integer sums only: the result is a function of the
// input, not of an execution order.
#pragma once
#include <hip/hip_runtime.h>

namespace mgs {

constexpr int kCompactThreads = 256;                      // every user's workgroup
constexpr int kCompactScanPer = 4;                        // block totals per thread and trip of scan_block_totals

// exclusive scan of (v, f) over the workgroup's 256 threads; returns the totals in tv / tf
__device__ __forceinline__ void block_scan2(unsigned& v, unsigned& f, unsigned& tv, unsigned& tf, unsigned (*s_w)[2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned iv = v, jf = f;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned a = __shfl_up(iv, off), b = __shfl_up(jf, off);
    if (lane >= off) { iv += a; jf += b; }
  }
  __syncthreads();              // a previous trip's readers of s_w are done
  if (lane == 63) { s_w[wave][0] = iv; s_w[wave][1] = jf; }
  __syncthreads();
  unsigned bv = 0, bf = 0;
  tv = 0; tf = 0;
#pragma unroll
  for (int q = 0; q < kCompactThreads / 64; q++) {
    if (q < wave) { bv += s_w[q][0]; bf += s_w[q][1]; }
    tv += s_w[q][0]; tf += s_w[q][1];
  }
  v = bv + iv - v;
  f = bf + jf - f;
}

// inclusive scan of v over the workgroup's 256 threads; the total in `total`
__device__ __forceinline__ unsigned long long block_scan_incl(unsigned long long v, unsigned long long& total,
                                                              unsigned long long* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long a = __shfl_up(v, off);
    if (lane >= off) v += a;
  }
  __syncthreads();              // a previous trip's readers of s_w are done
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  unsigned long long base = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < kCompactThreads / 64; q++) {
    if (q < wave) base += s_w[q];
    total += s_w[q];
  }
  return base + v;
}

// the two as one overloaded exclusive scan, for scan_block_totals
__device__ __forceinline__ void block_scan_excl(uint2& v, uint2& total, unsigned (*s_w)[2]) {
  block_scan2(v.x, v.y, total.x, total.y, s_w);
}
__device__ __forceinline__ void block_scan_excl(unsigned long long& v, unsigned long long& total, unsigned long long* s_w) {
  v = block_scan_incl(v, total, s_w) - v;
}

// what scan_block_totals scans of a loaded block total: the value itself, or x and y of a uint4 whose z and w ride along
__device__ __forceinline__ uint2 scan_key(uint2 t) { return t; }
__device__ __forceinline__ uint2 scan_key(uint4 t) { return make_uint2(t.x, t.y); }
__device__ __forceinline__ unsigned long long scan_key(unsigned long long t) { return t; }

// One workgroup of 256 threads over n block totals, kCompactScanPer consecutive ones per thread, i.e. 1024 per trip:
// store(b, sum of scan_key(load(0 .. b - 1)), load(b)) for every b < n; returns the sum of all (in every thread).
// s_w: unsigned [4][2] for uint2 keys, unsigned long long [4] for uint64 ones.  A trip's loads are all issued before
// the first is used: load() only loads, whatever else is summed belongs into store().
template <class S, class Load, class Store>
__device__ __forceinline__ auto scan_block_totals(int n, S s_w, Load load, Store store) {
  using Item = decltype(load(0));
  using T = decltype(scan_key(load(0)));
  T carry = T();
  for (int b0 = 0; b0 < n; b0 += kCompactThreads * kCompactScanPer) {
    const int b = b0 + kCompactScanPer * threadIdx.x;
    Item t[kCompactScanPer];
    T v = T(), total;
#pragma unroll
    for (int q = 0; q < kCompactScanPer; q++) {
      t[q] = b + q < n ? load(b + q) : Item();
      v += scan_key(t[q]);
    }
    block_scan_excl(v, total, s_w);
    T run = carry + v;
#pragma unroll
    for (int q = 0; q < kCompactScanPer; q++) {
      if (b + q < n) store(b + q, run, t[q]);
      run += scan_key(t[q]);
    }
    carry += total;
  }
  return carry;
}

}  // namespace mgs
