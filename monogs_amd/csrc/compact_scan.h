// The stable compaction shared by mesh_clean.hip and mesh_render.hip: an exclusive scan of two flags over a workgroup,
// and the ONE-workgroup scan of the block totals that turns them into bases and grand totals.  Integer sums only: the
// result is a function of the flags, not of an execution order.
#pragma once
#include <hip/hip_runtime.h>

namespace mgs {

constexpr int kCompactThreads = 256;
constexpr int kCompactScanPer = 4;                        // block totals per thread and trip of k_compact_scan

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

// One workgroup, kCompactScanPer consecutive totals per thread, i.e. 1024 per trip: x and y become exclusive bases, z and
// w are summed.  counts (may be null): the totals of x, y, z, w.  (static: one copy per translation unit that includes it)
static __global__ __launch_bounds__(kCompactThreads) void k_compact_scan(uint4* __restrict__ base, int nblocks,
                                                                         int* __restrict__ counts) {
  __shared__ unsigned s_w[kCompactThreads / 64][2];
  unsigned cv = 0, cf = 0, cz = 0, cw = 0;
  for (int b0 = 0; b0 < nblocks; b0 += kCompactThreads * kCompactScanPer) {
    const int b = b0 + kCompactScanPer * threadIdx.x;
    uint4 t[kCompactScanPer];
    unsigned v = 0, f = 0, tv, tf;
#pragma unroll
    for (int q = 0; q < kCompactScanPer; q++) {
      t[q] = b + q < nblocks ? base[b + q] : make_uint4(0u, 0u, 0u, 0u);
      v += t[q].x; f += t[q].y;
      cz += t[q].z; cw += t[q].w;
    }
    block_scan2(v, f, tv, tf, s_w);
    unsigned rv = cv + v, rf = cf + f;
#pragma unroll
    for (int q = 0; q < kCompactScanPer; q++) {
      if (b + q < nblocks) { base[b + q].x = rv; base[b + q].y = rf; }
      rv += t[q].x; rf += t[q].y;
    }
    cv += tv; cf += tf;
  }
  if (!counts) return;
  unsigned tz, tw;
  block_scan2(cz, cw, tz, tw, s_w);      // used as the block's sum of z and w
  if (threadIdx.x == 0) {
    counts[0] = (int)cv; counts[1] = (int)cf; counts[2] = (int)tz; counts[3] = (int)tw;
  }
}

}  // namespace mgs
