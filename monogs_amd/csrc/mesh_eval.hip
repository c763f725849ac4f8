// Mesh evaluation: area-weighted surface sampling, exact nearest distance through a uniform grid, and the statistics of
// the distances (DESIGN.md "Mesh evaluation"; the mirrors in monogs_amd/mesh_eval.py are the contract).
//
// mgs_surface_sample
//   k_face_area      one thread per face: A = |(b - a) x (c - a)| as fp32 bits (0 when not finite or an index is bad);
//                    the block's integer maximum of the bits and its bad faces
//   k_area_max       ONE workgroup: the maximum and the bad faces of all blocks into the header (no atomics)
//   k_face_cdf       q = uint32(A * 2^(30 - E)) by an exact fp64 scaling, inclusive scan of q inside the block (uint64),
//                    the block's total
//   k_cdf_scan       ONE workgroup, 1024 block totals per trip with a carry (scan_block_totals, block_scan.h): inclusive
//                    block sums, T, the record
//   k_sample         one thread per sample: words, t = words mod T, block by binary search over the block sums, face by
//                    binary search inside the block, folded barycentric pair, point
// mgs_nearest_distance
//   k_nn_init        header: neutral box keys
//   k_nn_bbox        box of the finite reference points: integer min / max over order-preserving keys of the floats
//   k_nn_plan        ONE thread: cell size and grid dimensions from the box and Q, under the caps
//   k_nn_clear       cell counts = 0
//   k_nn_count       cell of every reference point (-1: not finite), integer histogram
//   k_nn_cellscan    exclusive scan of the counts inside blocks of 256 cells, block totals
//   k_nn_scan_totals ONE workgroup: the same scan_block_totals, exclusive, the total behind the last block
//   k_nn_cellstart   absolute start of every cell, and the end of the last
//   k_nn_scatter     points into their cells (x, y, z, original index); the place inside a cell is whatever the atomic
//                    gives - the query's (d2, index) rule makes the order invisible
//   k_nn_query       one query per lane over Chebyshev rings of cells; see "stopping bound" below
// mgs_mesh_eval_stats / _finish
//   k_eval_stats     kStatBlocks workgroups, grid stride: count, count below the threshold, max bits, fp64 sum; fixed tree
//   k_eval_finish    ONE workgroup: the kStatBlocks partials of both directions in a fixed order, the record
//
// Stopping bound.  The cell of a coordinate x on an axis is min(int(fl(fl(xc - lo) * inv_h)), dim - 1) with xc = x
// clamped to [lo, hi]: a monotone function of x.  Let qc be the query clamped to the box.  Every reference point p lies
// in the box, so |q - p|^2 >= |q - qc|^2 + |qc - p|^2 (qc is the projection of q onto a convex set).  After rings 0..k
// every point not yet seen lies in a cell that differs from the query's by more than k on some axis; by monotonicity the
// two values t = fl(fl(x - lo) * inv_h) differ by more than k there.  t carries two roundings and is at most dim <= 1024,
// so |qc - p| on that axis exceeds (k - 4 * 1025 * 2^-24) / inv_h, and inv_h = fl(1 / h): more than k h (1 - 2^-11) for
// k >= 1.  Squared that is k^2 h^2 (1 - 2^-10); the fp32 d2 of such a point is below its exact value by at most five
// roundings.  The lane stops when  best < (D0 + (k h)^2 (1 - 2^-9)) (1 - 2^-20),  D0 = fp32 |q - qc|^2: the factor 2^-9
// leaves 2^-10 for the roundings of (k h)^2 itself, 2^-20 = 16 ulp covers the roundings of D0, of the sum and of d2.
// With h < 1e-15 (squares near the subnormals) no lane stops early.  A lane that never stops ends after ring
// max(c, dim - 1 - c) over the axes, having seen every cell once: at most all cells plus all points.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/monogs_raster.h"
#include "block_scan.h"
#include "launch.h"
#include "philox.h"
#include "rn_math.h"
#include "scratch_carve.h"

namespace mgs {
namespace meval {

constexpr int kThreads = 256;
static_assert(kThreads == kCompactThreads, "block_scan_incl scans a workgroup of kCompactThreads");
constexpr int kMaxCells = MGS_NEAREST_MAX_CELLS;
constexpr int kMaxDim = MGS_NEAREST_MAX_DIM;
constexpr int kCellBlocks = kMaxCells / kThreads;         // 8192
constexpr int kStatBlocks = 256;

// ---- surface sampling --------------------------------------------------------------------------------------------------
struct SampleHeader {
  unsigned max_bits;            // bits of the largest finite area
  int bad;                      // faces with an index outside [0,V)
  unsigned long long total;     // T
};

struct SampleScratch {
  SampleHeader* hdr;
  unsigned* area;               // [F] bits of A, 0 when the face has no weight
  unsigned long long* local;    // [F] inclusive sum of q inside the face's block
  unsigned long long* bsum;     // [blocks(F)] inclusive sums of the block totals
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static SampleScratch sample_scratch_of(void* p, size_t F, size_t* bytes = nullptr) {
  Carver c(p);
  SampleScratch S;
  S.hdr = c.take<SampleHeader>();
  S.area = c.take<unsigned>(F);
  S.local = c.take<unsigned long long>(F);
  S.bsum = c.take<unsigned long long>((size_t)grid_of((long long)F));
  if (bytes) *bytes = c.bytes;
  return S;
}

__device__ __forceinline__ bool finite_bits(unsigned b) { return (b & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(kThreads) void k_face_area(const float* __restrict__ verts, const int* __restrict__ faces,
                                                        int V, int F, SampleScratch S) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  unsigned bits = 0;
  bool bad = false;
  if (f < F) {
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if ((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V) {
      float e[3], g[3];
#pragma unroll
      for (int ax = 0; ax < 3; ax++) {
        const float a = verts[3 * (size_t)ia + ax];
        e[ax] = sub_rn(verts[3 * (size_t)ib + ax], a);
        g[ax] = sub_rn(verts[3 * (size_t)ic + ax], a);
      }
      const float nx = sub_rn(mul_rn(e[1], g[2]), mul_rn(e[2], g[1]));
      const float ny = sub_rn(mul_rn(e[2], g[0]), mul_rn(e[0], g[2]));
      const float nz = sub_rn(mul_rn(e[0], g[1]), mul_rn(e[1], g[0]));
      // sqrtf is the correctly rounded root (surface.hip)
      const float A = sqrtf(add_rn(add_rn(mul_rn(nx, nx), mul_rn(ny, ny)), mul_rn(nz, nz)));
      const unsigned b = __float_as_uint(A);
      if (finite_bits(b)) bits = b;             // A >= 0; a NaN or an infinity has no weight
    } else {
      bad = true;
    }
    S.area[f] = bits;
  }
  // the block's largest bits and its bad faces, packed into the block's slot of bsum (k_face_cdf overwrites it later):
  // one atomic per wave on the header's word cost 194 us at a million faces (DESIGN.md "Mesh evaluation", Measured)
  __shared__ unsigned s_m[kThreads / 64], s_b[kThreads / 64];
  unsigned m = bits;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  const unsigned long long nb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_b[threadIdx.x >> 6] = (unsigned)__popcll(nb); }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned bm = 0, bb = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) { bm = max(bm, s_m[w]); bb += s_b[w]; }
    S.bsum[blockIdx.x] = ((unsigned long long)bb << 32) | bm;
  }
}

// One workgroup: the largest area bits and the bad faces of all blocks into the header.
__global__ __launch_bounds__(kThreads) void k_area_max(SampleScratch S, int nblocks) {
  __shared__ unsigned s_m[kThreads / 64], s_b[kThreads / 64];
  unsigned m = 0, bad = 0;
  for (int b = threadIdx.x; b < nblocks; b += kThreads) {
    const unsigned long long v = S.bsum[b];
    m = max(m, (unsigned)(v & 0xFFFFFFFFull));
    bad += (unsigned)(v >> 32);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    m = max(m, (unsigned)__shfl_xor((int)m, off));
    bad += (unsigned)__shfl_xor((int)bad, off);
  }
  if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_b[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned bm = 0, bb = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) { bm = max(bm, s_m[w]); bb += s_b[w]; }
    S.hdr->max_bits = bm;
    S.hdr->bad = (int)bb;
    S.hdr->total = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_face_cdf(int F, SampleScratch S) {
  __shared__ unsigned long long s_w[kThreads / 64];
  const int f = blockIdx.x * kThreads + threadIdx.x;
  const unsigned mb = S.hdr->max_bits;
  unsigned long long q = 0;
  if (f < F && mb) {
    const int E = ilogb((double)__uint_as_float(mb));
    q = (unsigned long long)(unsigned)ldexp((double)__uint_as_float(S.area[f]), 30 - E);       // exact scaling, truncation
  }
  unsigned long long total;
  const unsigned long long incl = block_scan_incl(q, total, s_w);
  if (f < F) S.local[f] = incl;
  if (threadIdx.x == 0) S.bsum[blockIdx.x] = total;
}

// The one-workgroup scan of the block totals (scan_block_totals): they become inclusive sums.
__global__ __launch_bounds__(kThreads) void k_cdf_scan(SampleScratch S, int nblocks, int* __restrict__ record) {
  __shared__ unsigned long long s_w[kThreads / 64];
  const unsigned long long carry = scan_block_totals(
      nblocks, s_w, [&](int b) { return S.bsum[b]; },
      [&](int b, unsigned long long run, unsigned long long own) { S.bsum[b] = run + own; });
  if (threadIdx.x == 0) {
    S.hdr->total = carry;
    record[0] = carry == 0 ? 1 : 0;
    record[1] = S.hdr->bad;
    record[2] = (int)(unsigned)(carry & 0xFFFFFFFFull);
    record[3] = (int)(unsigned)(carry >> 32);
  }
}

__global__ __launch_bounds__(kThreads) void k_sample(mgs_surface_sample_args A, SampleScratch S) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  const int n = A.num_samples, F = A.num_faces;
  if (j >= n) return;
  const unsigned long long T = S.hdr->total;
  if (T == 0 || F <= 0) {
    const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) A.points[3 * (size_t)j + ax] = nan;
    A.face_index[j] = -1;
    return;
  }
  uint4 w;
  if (A.randoms) {
    w = reinterpret_cast<const uint4*>(A.randoms)[j];
  } else {
    w = philox4x32_10(make_uint4((unsigned)j, 0u, 2u, 0u), make_uint2((unsigned)A.seed, (unsigned)(A.seed >> 32)));
  }
  const unsigned long long t = ((unsigned long long)w.x | ((unsigned long long)w.y << 32)) % T;
  // the smallest block whose inclusive sum exceeds t: it exists, the last sum is T > t
  const int nblocks = (F + kThreads - 1) / kThreads;
  int lo = 0, hi = nblocks - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.bsum[mid] > t) hi = mid; else lo = mid + 1;
  }
  const unsigned long long r = t - (lo ? S.bsum[lo - 1] : 0ull);
  const int first = lo * kThreads;
  int a0 = 0, a1 = min(kThreads, F - first) - 1;
  while (a0 < a1) {
    const int mid = (a0 + a1) >> 1;
    if (S.local[first + mid] > r) a1 = mid; else a0 = mid + 1;
  }
  const int f = first + a0;
  unsigned k1 = w.z >> 8, k2 = w.w >> 8;
  if (k1 + k2 > (1u << 24)) { k1 = (1u << 24) - k1; k2 = (1u << 24) - k2; }
  const float u1 = (float)k1 * 5.9604644775390625e-8f, u2 = (float)k2 * 5.9604644775390625e-8f;       // exact
  int ia = A.faces[3 * (size_t)f], ib = A.faces[3 * (size_t)f + 1], ic = A.faces[3 * (size_t)f + 2];
  const unsigned V = (unsigned)A.num_verts;
  if ((unsigned)ia >= V || (unsigned)ib >= V || (unsigned)ic >= V) ia = ib = ic = 0;   // only if the faces changed since the scan
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const float a = A.verts[3 * (size_t)ia + ax];
    const float e = sub_rn(A.verts[3 * (size_t)ib + ax], a), g = sub_rn(A.verts[3 * (size_t)ic + ax], a);
    A.points[3 * (size_t)j + ax] = add_rn(add_rn(a, mul_rn(u1, e)), mul_rn(u2, g));
  }
  A.face_index[j] = f;
}

// ---- nearest distance --------------------------------------------------------------------------------------------------
struct GridHeader {
  unsigned min_key[3], max_key[3];     // order-preserving keys of the box of the finite reference points
  int any_finite;
  float lo[3], hi[3];
  float h, inv_h;
  int dims[3];
  int ncells, nblocks;
};

struct GridScratch {
  GridHeader* hdr;
  int* count;        // [kMaxCells] points of the cell; counted down to 0 by the scatter
  int* cstart;       // [kMaxCells + 1] first point of the cell; [ncells] = the number of finite points
  int* btot;         // [kCellBlocks + 1] points of the earlier blocks of cells; [nblocks] = all
  int* cell;         // [Q] cell of the point, -1 when not finite
  float4* pts;       // [Q] (x, y, z, bits of the original index), by cell
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static GridScratch grid_scratch_of(void* p, size_t Q, size_t* bytes = nullptr) {
  Carver c(p);
  GridScratch S;
  S.hdr = c.take<GridHeader>();
  S.count = c.take<int>((size_t)kMaxCells);
  S.cstart = c.take<int>((size_t)kMaxCells + 1);
  S.btot = c.take<int>((size_t)kCellBlocks + 1);
  S.cell = c.take<int>(Q);
  S.pts = c.take<float4>(Q);
  if (bytes) *bytes = c.bytes;
  return S;
}

// unsigned order of the keys = order of the floats (no NaN reaches this)
__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float order_key_inv(unsigned k) {
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return finite_bits(__float_as_uint(x)) && finite_bits(__float_as_uint(y)) && finite_bits(__float_as_uint(z));
}

__global__ void k_nn_init(GridScratch S) {
  if (threadIdx.x < 3) {
    S.hdr->min_key[threadIdx.x] = 0xFFFFFFFFu;
    S.hdr->max_key[threadIdx.x] = 0u;
  }
}

__global__ __launch_bounds__(kThreads) void k_nn_bbox(const float* __restrict__ ref, int Q, GridScratch S) {
  __shared__ unsigned s_mn[kThreads / 64][3], s_mx[kThreads / 64][3];
  const int r = blockIdx.x * kThreads + threadIdx.x;
  unsigned mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  if (r < Q) {
    const float x = ref[3 * (size_t)r], y = ref[3 * (size_t)r + 1], z = ref[3 * (size_t)r + 2];
    if (finite3(x, y, z)) {
      mn[0] = mx[0] = order_key(x); mn[1] = mx[1] = order_key(y); mn[2] = mx[2] = order_key(z);
    }
  }
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn[ax] = min(mn[ax], (unsigned)__shfl_xor((int)mn[ax], off));
      mx[ax] = max(mx[ax], (unsigned)__shfl_xor((int)mx[ax], off));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) { s_mn[threadIdx.x >> 6][ax] = mn[ax]; s_mx[threadIdx.x >> 6][ax] = mx[ax]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int ax = threadIdx.x;
    unsigned lo = s_mn[0][ax], hi = s_mx[0][ax];
#pragma unroll
    for (int w = 1; w < kThreads / 64; w++) { lo = min(lo, s_mn[w][ax]); hi = max(hi, s_mx[w][ax]); }
    // the box only grows, so a stale read of it is an inner bound: a block inside it has nothing to add (a block without
    // a finite point holds the neutral keys and never passes).  One atomic per wave on these six words cost 252 us.
    if (lo < __hip_atomic_load(&S.hdr->min_key[ax], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&S.hdr->min_key[ax], lo);
    if (hi > __hip_atomic_load(&S.hdr->max_key[ax], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&S.hdr->max_key[ax], hi);
  }
}

// One thread.  Chosen cell size: about eight cells per reference point (DESIGN.md "Mesh evaluation", Measured), over the axes on which the box is at least one cell
// wide (a plane or a line of points gets a 2-D or 1-D grid); then h is raised until no axis has more than kMaxDim cells
// and the grid no more than kMaxCells.
__global__ void k_nn_plan(GridScratch S, int Q, float cell_size) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  GridHeader& H = *S.hdr;
  const int n = H.min_key[0] != 0xFFFFFFFFu ? 1 : 0;     // no finite float has the neutral key
  H.any_finite = n;
  double ext[3], emax = 0.0;
  for (int ax = 0; ax < 3; ax++) {
    H.lo[ax] = n > 0 ? order_key_inv(H.min_key[ax]) : 0.f;
    H.hi[ax] = n > 0 ? order_key_inv(H.max_key[ax]) : 0.f;
    ext[ax] = (double)H.hi[ax] - (double)H.lo[ax];
    emax = fmax(emax, ext[ax]);
  }
  double h = (double)cell_size;
  if (!(h > 0.0)) {
    const double target = fmin((double)kMaxCells, fmax(1.0, 8.0 * (double)Q));
    bool active[3] = {ext[0] > 0.0, ext[1] > 0.0, ext[2] > 0.0};
    h = 1.0;
    for (int pass = 0; pass < 3; pass++) {
      int m = 0;
      double prod = 1.0;
      for (int ax = 0; ax < 3; ax++) if (active[ax]) { m++; prod *= ext[ax]; }
      if (m == 0) break;
      h = pow(prod / target, 1.0 / m);
      bool dropped = false;
      for (int ax = 0; ax < 3; ax++) if (active[ax] && ext[ax] < h) { active[ax] = false; dropped = true; }
      if (!dropped) break;
    }
  }
  if (!(h >= 1e-30)) h = 1e-30;              // also a NaN
  if (h > 1e30) h = 1e30;
  h = fmax(h, emax / (double)(kMaxDim - 1));
  float hf = (float)h;
  int dims[3] = {1, 1, 1};
  for (int it = 0; it < 96; it++) {
    long long cells = 1;
    bool fits = true;
    for (int ax = 0; ax < 3; ax++) {
      const double d = floor(ext[ax] / (double)hf) + 1.0;
      if (!(d <= (double)kMaxDim)) { fits = false; break; }
      dims[ax] = (int)d;
      cells *= dims[ax];
    }
    if (fits && cells <= kMaxCells) break;
    dims[0] = dims[1] = dims[2] = 1;         // what stays if the loop runs out (it cannot: 1.1^96 > 2^13)
    hf *= 1.1f;
  }
  H.h = hf;
  H.inv_h = 1.f / hf;
  for (int ax = 0; ax < 3; ax++) H.dims[ax] = dims[ax];
  H.ncells = dims[0] * dims[1] * dims[2];
  H.nblocks = (H.ncells + kThreads - 1) / kThreads;
}

// cell of coordinate x on axis ax: monotone in x (the file's head); xc is x clamped to the box
__device__ __forceinline__ int cell_of(const GridHeader& H, int ax, float x) {
  const float xc = fminf(fmaxf(x, H.lo[ax]), H.hi[ax]);
  const float t = mul_rn(sub_rn(xc, H.lo[ax]), H.inv_h);
  return min((int)fminf(t, (float)kMaxDim), H.dims[ax] - 1);
}

__global__ __launch_bounds__(kThreads) void k_nn_clear(GridScratch S) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c < S.hdr->ncells && c < kMaxCells) S.count[c] = 0;
}

__global__ __launch_bounds__(kThreads) void k_nn_count(const float* __restrict__ ref, int Q, GridScratch S) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= Q) return;
  const GridHeader& H = *S.hdr;
  const float x = ref[3 * (size_t)r], y = ref[3 * (size_t)r + 1], z = ref[3 * (size_t)r + 2];
  int c = -1;
  if (finite3(x, y, z)) {
    c = (cell_of(H, 2, z) * H.dims[1] + cell_of(H, 1, y)) * H.dims[0] + cell_of(H, 0, x);
    if ((unsigned)c < (unsigned)H.ncells && c < kMaxCells) atomicAdd(&S.count[c], 1); else c = -1;
  }
  S.cell[r] = c;
}

__global__ __launch_bounds__(kThreads) void k_nn_cellscan(GridScratch S) {
  __shared__ unsigned long long s_w[kThreads / 64];
  const int ncells = min(S.hdr->ncells, kMaxCells);
  if (blockIdx.x * kThreads >= ncells) return;            // uniform
  const int c = blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long v = c < ncells ? (unsigned long long)S.count[c] : 0ull;
  unsigned long long total;
  const unsigned long long incl = block_scan_incl(v, total, s_w);
  if (c < ncells) S.cstart[c] = (int)(incl - v);
  if (threadIdx.x == 0) S.btot[blockIdx.x] = (int)total;
}

__global__ __launch_bounds__(kThreads) void k_nn_scan_totals(GridScratch S) {
  __shared__ unsigned long long s_w[kThreads / 64];
  const int nblocks = min(S.hdr->nblocks, kCellBlocks);
  const unsigned long long carry = scan_block_totals(
      nblocks, s_w, [&](int b) { return (unsigned long long)S.btot[b]; },
      [&](int b, unsigned long long run, unsigned long long) { S.btot[b] = (int)run; });
  if (threadIdx.x == 0) S.btot[nblocks] = (int)carry;
}

__global__ __launch_bounds__(kThreads) void k_nn_cellstart(GridScratch S) {
  const int ncells = min(S.hdr->ncells, kMaxCells);
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c < ncells) S.cstart[c] += S.btot[c / kThreads];
  else if (c == ncells) S.cstart[c] = S.btot[min(S.hdr->nblocks, kCellBlocks)];
}

__global__ __launch_bounds__(kThreads) void k_nn_scatter(const float* __restrict__ ref, int Q, GridScratch S) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= Q) return;
  const int c = S.cell[r];
  if (c < 0) return;
  const int pos = S.cstart[c] + atomicSub(&S.count[c], 1) - 1;
  if ((unsigned)pos < (unsigned)Q)
    S.pts[pos] = make_float4(ref[3 * (size_t)r], ref[3 * (size_t)r + 1], ref[3 * (size_t)r + 2], __int_as_float(r));
}

__global__ __launch_bounds__(kThreads) void k_nn_query(mgs_nearest_args A, GridScratch S) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.num_query) return;
  const GridHeader& H = *S.hdr;
  const float inf = __builtin_inff();
  const float qx = A.query[3 * (size_t)i], qy = A.query[3 * (size_t)i + 1], qz = A.query[3 * (size_t)i + 2];
  float best = inf;
  int bi = 0x7FFFFFFF;
  if (finite3(qx, qy, qz) && H.any_finite) {
    const int nx = H.dims[0], ny = H.dims[1], nz = H.dims[2];
    const int Q = A.num_ref;
    const float h = H.h;
    const bool use_bound = h >= 1e-15f;
    const int cx = cell_of(H, 0, qx), cy = cell_of(H, 1, qy), cz = cell_of(H, 2, qz);
    const float ox = sub_rn(qx, fminf(fmaxf(qx, H.lo[0]), H.hi[0]));
    const float oy = sub_rn(qy, fminf(fmaxf(qy, H.lo[1]), H.hi[1]));
    const float oz = sub_rn(qz, fminf(fmaxf(qz, H.lo[2]), H.hi[2]));
    const float D0 = add_rn(add_rn(mul_rn(ox, ox), mul_rn(oy, oy)), mul_rn(oz, oz));
    const int kmax = max(max(max(cx, nx - 1 - cx), max(cy, ny - 1 - cy)), max(cz, nz - 1 - cz));

    auto scan = [&](int row, int xa, int xb) {            // the points of cells [xa, xb] of one row: contiguous
      const int s = max(S.cstart[row + xa], 0), e = min(S.cstart[row + xb + 1], Q);
      for (int p = s; p < e; p++) {
        const float4 r = S.pts[p];
        const float dx = sub_rn(qx, r.x), dy = sub_rn(qy, r.y), dz = sub_rn(qz, r.z);
        const float d2 = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
        const int id = __float_as_int(r.w);
        if (d2 < best || (d2 == best && id < bi)) { best = d2; bi = id; }
      }
    };

    for (int k = 0; k <= kmax; k++) {
      const int z0 = max(cz - k, 0), z1 = min(cz + k, nz - 1);
      const int y0 = max(cy - k, 0), y1 = min(cy + k, ny - 1);
      const int xa = max(cx - k, 0), xb = min(cx + k, nx - 1);
      for (int z = z0; z <= z1; z++) {
        const bool zface = z - cz == k || cz - z == k;
        for (int y = y0; y <= y1; y++) {
          const int row = (z * ny + y) * nx;
          if (zface || y - cy == k || cy - y == k) {
            scan(row, xa, xb);
          } else {
            if (cx - k >= 0) scan(row, cx - k, cx - k);
            if (cx + k <= nx - 1) scan(row, cx + k, cx + k);
          }
        }
      }
      if (use_bound) {
        const float rb = mul_rn((float)k, h);
        const float lb = mul_rn(add_rn(D0, mul_rn(mul_rn(rb, rb), 0.998046875f)), 0.99999904632568359375f);
        if (best < lb) break;
      }
    }
  }
  A.d2[i] = best;
  A.index[i] = bi == 0x7FFFFFFF ? -1 : bi;
}

// ---- statistics --------------------------------------------------------------------------------------------------------
struct StatPartial {
  double sum;
  unsigned long long n, below;
  unsigned max_bits, pad;
};

__device__ __forceinline__ void stat_merge(StatPartial& a, const StatPartial& b) {
  a.sum += b.sum; a.n += b.n; a.below += b.below; a.max_bits = max(a.max_bits, b.max_bits);
}

// the workgroup's partial in thread 0: a fixed tree over the lanes, then the waves in order
__device__ __forceinline__ StatPartial stat_block_reduce(StatPartial p, StatPartial* s_p) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    StatPartial o;
    o.sum = __shfl_down(p.sum, off);
    o.n = __shfl_down(p.n, off);
    o.below = __shfl_down(p.below, off);
    o.max_bits = (unsigned)__shfl_down((int)p.max_bits, off);
    stat_merge(p, o);
  }
  if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kThreads / 64; w++) stat_merge(p, s_p[w]);
  return p;
}

__global__ __launch_bounds__(kThreads) void k_eval_stats(const float* __restrict__ d2, int n, float threshold,
                                                         StatPartial* __restrict__ out) {
  __shared__ StatPartial s_p[kThreads / 64];
  StatPartial p{0.0, 0ull, 0ull, 0u, 0u};
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)kStatBlocks * kThreads) {
    const float v = d2[i];
    if (finite_bits(__float_as_uint(v)) && v >= 0.f) {
      const float d = sqrtf(v);
      p.sum += (double)d;
      p.n++;
      if (d < threshold) p.below++;
      p.max_bits = max(p.max_bits, __float_as_uint(d));
    }
  }
  p = stat_block_reduce(p, s_p);
  if (threadIdx.x == 0) out[blockIdx.x] = p;
}

__global__ __launch_bounds__(kThreads) void k_eval_finish(const StatPartial* __restrict__ parts, mgs_mesh_eval_args A) {
  __shared__ StatPartial s_p[kThreads / 64];
  for (int dir = 0; dir < 2; dir++) {
    StatPartial p = parts[dir * kStatBlocks + threadIdx.x];          // kStatBlocks == kThreads
    __syncthreads();                                                 // the previous direction's readers of s_p are done
    p = stat_block_reduce(p, s_p);
    if (threadIdx.x == 0) {
      A.record[4 * dir + 0] = (double)p.n;
      A.record[4 * dir + 1] = (double)p.below;
      A.record[4 * dir + 2] = (double)__uint_as_float(p.max_bits);
      A.record[4 * dir + 3] = p.sum;
      const int* sr = A.sample_record[dir];
      A.record[8 + 2 * dir] = sr ? (double)sr[0] : 0.0;
      A.record[9 + 2 * dir] = sr ? (double)sr[1] : 0.0;
    }
  }
}

static_assert(kStatBlocks == kThreads, "k_eval_finish takes one partial per thread");

}  // namespace meval
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_surface_sample_args_size(void) { return (int32_t)sizeof(mgs_surface_sample_args); }
int32_t mgs_nearest_args_size(void) { return (int32_t)sizeof(mgs_nearest_args); }
int32_t mgs_mesh_eval_args_size(void) { return (int32_t)sizeof(mgs_mesh_eval_args); }

uint64_t mgs_surface_sample_scratch_bytes(int32_t num_faces) {
  if (num_faces < 0 || num_faces > kMaxItems) return 0;
  return carved_bytes(meval::sample_scratch_of, (size_t)num_faces);
}

uint64_t mgs_nearest_scratch_bytes(int32_t num_ref) {
  if (num_ref < 0 || num_ref > kMaxItems) return 0;
  return carved_bytes(meval::grid_scratch_of, (size_t)num_ref);
}

uint64_t mgs_mesh_eval_scratch_bytes(void) { return 2 * (uint64_t)meval::kStatBlocks * sizeof(meval::StatPartial); }

int32_t mgs_surface_sample(const mgs_surface_sample_args* a, void* stream) {
  if (!a || a->num_verts < 0 || a->num_faces < 0 || a->num_samples < 0 || !a->scratch || !a->record)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->num_faces > 0 && (!a->faces || (a->num_verts > 0 && !a->verts))) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_samples > 0 && (!a->points || !a->face_index)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > kMaxItems || a->num_faces > kMaxItems || a->num_samples > kMaxItems)
    return MGS_ERR_UNSUPPORTED;
  const int V = a->num_verts, F = a->num_faces, n = a->num_samples;
  const meval::SampleScratch S = meval::sample_scratch_of(a->scratch, (size_t)F);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(meval::kThreads);
  const int blocks = grid_of(F);
  if (F > 0) launch("face_area", meval::k_face_area, dim3(blocks), th, st, a->verts, a->faces, V, F, S);
  launch("area_max", meval::k_area_max, dim3(1), th, st, S, blocks);
  if (F > 0) launch("face_cdf", meval::k_face_cdf, dim3(blocks), th, st, F, S);
  launch("cdf_scan", meval::k_cdf_scan, dim3(1), th, st, S, blocks, a->record);
  if (n > 0) launch("sample", meval::k_sample, dim3(grid_of(n)), th, st, *a, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_nearest_distance(const mgs_nearest_args* a, void* stream) {
  if (!a || a->num_query < 0 || a->num_ref < 0 || !a->scratch || !(a->cell_size >= 0.f)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_ref > 0 && !a->ref) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_query > 0 && (!a->query || !a->d2 || !a->index)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_query > kMaxItems || a->num_ref > kMaxItems) return MGS_ERR_UNSUPPORTED;
  const int P = a->num_query, Q = a->num_ref;
  if (P == 0) return MGS_OK;
  const meval::GridScratch S = meval::grid_scratch_of(a->scratch, (size_t)Q);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(meval::kThreads), cells(meval::kCellBlocks);
  launch("nn_init", meval::k_nn_init, dim3(1), dim3(64), st, S);
  if (Q > 0) launch("nn_bbox", meval::k_nn_bbox, dim3(grid_of(Q)), th, st, a->ref, Q, S);
  launch("nn_plan", meval::k_nn_plan, dim3(1), dim3(64), st, S, Q, a->cell_size);
  launch("nn_clear", meval::k_nn_clear, cells, th, st, S);
  if (Q > 0) launch("nn_count", meval::k_nn_count, dim3(grid_of(Q)), th, st, a->ref, Q, S);
  launch("nn_cellscan", meval::k_nn_cellscan, cells, th, st, S);
  launch("nn_scan_totals", meval::k_nn_scan_totals, dim3(1), th, st, S);
  launch("nn_cellstart", meval::k_nn_cellstart, dim3(meval::kCellBlocks + 1), th, st, S);
  if (Q > 0) launch("nn_scatter", meval::k_nn_scatter, dim3(grid_of(Q)), th, st, a->ref, Q, S);
  launch("nn_query", meval::k_nn_query, dim3(grid_of(P)), th, st, *a, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

static int32_t eval_status(const mgs_mesh_eval_args* a) {
  if (!a || a->num < 0 || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  if (a->num > kMaxItems) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

int32_t mgs_mesh_eval_stats(const mgs_mesh_eval_args* a, void* stream) {
  const int32_t rc = eval_status(a);
  if (rc != MGS_OK) return rc;
  if (a->direction < 0 || a->direction > 1 || !(a->threshold >= 0.f) || (a->num > 0 && !a->d2)) return MGS_ERR_BAD_ARGUMENT;
  meval::StatPartial* parts = static_cast<meval::StatPartial*>(a->scratch) + a->direction * meval::kStatBlocks;
  launch("eval_stats", meval::k_eval_stats, dim3(meval::kStatBlocks), dim3(meval::kThreads), (hipStream_t)stream, a->d2,
         a->num, a->threshold, parts);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_eval_finish(const mgs_mesh_eval_args* a, void* stream) {
  const int32_t rc = eval_status(a);
  if (rc != MGS_OK) return rc;
  if (!a->record) return MGS_ERR_BAD_ARGUMENT;
  launch("eval_finish", meval::k_eval_finish, dim3(1), dim3(meval::kThreads), (hipStream_t)stream,
         static_cast<const meval::StatPartial*>(a->scratch), *a);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
