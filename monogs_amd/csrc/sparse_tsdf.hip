// Sparse TSDF volume: the dense lattice of tsdf.hip without its box - bricks of 8 x 8 x 8 points in a pool, found through
// a hash map of 64-bit brick keys (DESIGN.md "Sparse TSDF volume"; mirrors in monogs_amd/sparse_tsdf.py).  A sparse
// volume IS the dense volume of the same origin and voxel size in which every point of an unallocated brick has weight 0.
//
// Allocation of one view (mgs_sparse_tsdf_allocate), five launches behind one fill of the view's set table:
//   k_alloc_candidates   one thread per (pixel, sample): the keys of its eight corner bricks to cand_key; a key the map
//                        already holds, one out of range (counted) or one an earlier corner of the same thread has is
//                        written as kNoKey
//   k_alloc_insert       min_index_set.h: per key the smallest candidate index (a set per block in LDS, then its
//                        representatives into the view's table)
//   k_alloc_flag         the representatives, their rank inside a block of 256 candidates, the block totals
//   k_alloc_scan         ONE workgroup (scan_block_totals): bases; state: count, dropped, the view's base id
//   k_alloc_commit       representative r -> brick id base + r: its coordinates, its map entry
// The map is written by k_alloc_commit only (one thread per new key, CAS on the key plane, the value stored plainly) and
// read by later launches only; the set table is touched by agent-scope atomics in k_alloc_insert and read plainly in
// k_alloc_flag.  Nothing else crosses workgroups inside a launch.
//
//   k_sparse_integrate   one workgroup of 128 threads per brick of the POOL (workgroups past the count leave at once: no
//                        host read), a thread owns four consecutive points of an x row; tsdf.hip's cull and update
//   k_sparse_neighbors   the [bricks,27] table of brick ids (-1 absent), one map lookup per entry
//   k_sparse_classify    one workgroup per brick, an LDS tile of 10^3 flags filled through the table; codes as tsdf.hip's
//   k_sparse_prefix / k_sparse_scan / k_sparse_emit   tsdf.hip's three-launch form over bricks * 512 virtual points
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/monogs_raster.h"
#include "block_scan.h"
#include "launch.h"
#include "min_index_set.h"
#include "pinhole.h"
#include "rn_math.h"
#include "scratch_carve.h"
#include "sparse_tsdf_map.h"

namespace mgs {
namespace sparse {

static_assert(kThreads == kCompactThreads, "block_scan2 scans a workgroup of kCompactThreads");
constexpr int kH = kB + 2, kC = kB + 1;                    // flag tile with its halo; cells with base corner -1 .. 7
constexpr int kIntThreads = kBP / 4;                       // integration: four points per thread
constexpr unsigned short kNoRank = 0xFFFFu;
constexpr int kLocalSlots = 2 * kThreads;                  // a block's own set in k_alloc_insert: twice its candidates

__device__ __constant__ signed char c_slot_of[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
__device__ __constant__ unsigned char c_slot_code[7] = {1, 2, 4, 3, 5, 6, 7};
__device__ __constant__ unsigned char c_tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7},
                                                     {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__device__ __constant__ unsigned char c_tet_flip[6] = {0, 1, 1, 0, 0, 1};
// The sign cases of tsdf.hip, restated (tests/test_cpu_sparse_tsdf.py compares this text with tsdf.py:_tet_table()).
// TET_TABLE_BEGIN
__device__ __constant__ unsigned char c_tet_ntri[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__device__ __constant__ unsigned char c_tet_tri[16][6] = {
    {0, 0, 0, 0, 0, 0}, {0, 1, 2, 0, 0, 0}, {0, 4, 3, 0, 0, 0}, {1, 2, 4, 1, 4, 3},
    {1, 3, 5, 0, 0, 0}, {0, 5, 2, 0, 3, 5}, {0, 4, 5, 0, 5, 1}, {2, 4, 5, 0, 0, 0},
    {2, 5, 4, 0, 0, 0}, {0, 1, 5, 0, 5, 4}, {0, 5, 3, 0, 2, 5}, {1, 5, 3, 0, 0, 0},
    {1, 3, 4, 1, 4, 2}, {0, 3, 4, 0, 0, 0}, {0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
// TET_TABLE_END
__device__ __constant__ unsigned char c_tet_edge[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

// ---- the write side of the persistent map (sparse_tsdf_map.h has the keys and the read side) ------------------------
// `key` (which no other thread of this launch inserts and the map does not hold) takes the first free slot of its
// probe sequence; at most max_bricks <= table_size / 2 keys are ever inserted, so a free slot is met
__device__ __forceinline__ void map_insert(unsigned long long* __restrict__ keys, int* __restrict__ vals, unsigned mask,
                                           unsigned long long key, int id) {
  unsigned slot = (unsigned)mix64(key) & mask;
  for (unsigned probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
    unsigned long long cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kNoKey) {
      cur = atomicCAS(keys + slot, kNoKey, key);
      if (cur == kNoKey) {
        vals[slot] = id;
        return;
      }
    }
    if (cur == key) return;      // a caller's duplicate: the first holder keeps the key
  }
}

// ---- allocation ------------------------------------------------------------------------------------------------------
struct AllocScratch {
  unsigned long long* cand_key;   // [n] brick key of the candidate, kNoKey: none
  unsigned* table;                // [table] the view's set of candidate indices (min_index_set.h)
  unsigned short* rel;            // [n] rank of a representative among its block's, kNoRank otherwise
  uint2* base;                    // [blocks] x: representatives of the block, then of the earlier blocks
  int* view_base;                 // [1] state[0] before this view
};

static AllocScratch alloc_scratch_of(void* p, size_t n, size_t table, size_t* bytes = nullptr) {
  Carver c(p);
  AllocScratch s;
  s.cand_key = c.take<unsigned long long>(n);
  s.table = c.take<unsigned>(table);
  s.rel = c.take<unsigned short>(n);
  s.base = c.take<uint2>((size_t)grid_of((long long)n));
  s.view_base = c.take<int>();
  if (bytes) *bytes = c.bytes;
  return s;
}

__global__ __launch_bounds__(kThreads) void k_alloc_candidates(mgs_sparse_tsdf_view_args A, unsigned long long* __restrict__ cand_key,
                                                               unsigned map_mask) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int S = A.samples;
  if (t >= (long long)A.width * A.height * S) return;
  const int pix = (int)(t / S), s = (int)(t - (long long)pix * S);
  unsigned long long key[8];
#pragma unroll
  for (int c = 0; c < 8; c++) key[c] = kNoKey;
  int out_of_range = 0;
  do {
    float d = A.depth[pix];
    if (A.opacity) {
      const float o = A.opacity[pix];
      if (o < A.min_opacity) break;
      if (A.normalize) d = __fdiv_rn(d, o);
    }
    if (!(d > A.depth_min && d <= A.depth_max)) break;
    const float z = add_rn(sub_rn(d, A.trunc), mul_rn((float)s, mul_rn(4.f, A.vol.voxel_size)));
    if (!(z > A.z_near)) break;
    const int x = pix % A.width, y = pix / A.width;
    const float xn = __fdiv_rn(sub_rn((float)x, A.cx), A.fx), yn = __fdiv_rn(sub_rn((float)y, A.cy), A.fy);
    const float q[3] = {sub_rn(mul_rn(xn, z), A.T[3]), sub_rn(mul_rn(yn, z), A.T[7]), sub_rn(z, A.T[11])};
    float lo[3], hi[3];
    bool lo_ok[3], hi_ok[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float p = add_rn(add_rn(mul_rn(A.T[a], q[0]), mul_rn(A.T[4 + a], q[1])), mul_rn(A.T[8 + a], q[2]));
      const float l = __fdiv_rn(sub_rn(p, A.vol.origin[a]), A.vol.voxel_size);
      lo[a] = floorf(mul_rn(sub_rn(l, 4.f), 0.125f));
      hi[a] = floorf(mul_rn(add_rn(l, 4.f), 0.125f));
      lo_ok[a] = lo[a] >= (float)-kBias && lo[a] < (float)kBias;      // in float: a NaN or a huge value is no index
      hi_ok[a] = hi[a] >= (float)-kBias && hi[a] < (float)kBias;
    }
#pragma unroll
    for (int c = 0; c < 8; c++) {
      bool ok = true, again = false;
      int b[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const bool up = (c >> a) & 1;
        ok = ok && (up ? hi_ok[a] : lo_ok[a]);
        b[a] = ok ? (int)(up ? hi[a] : lo[a]) : 0;
        again = again || (up && hi[a] == lo[a]);     // corner c without bit a has the same brick and a smaller index
      }
      if (!ok) { out_of_range++; continue; }
      if (again) continue;
      const unsigned long long k = key_of(b[0], b[1], b[2]);
      if (map_find(keys_of(A.vol), A.vol.map_vals, map_mask, k) < 0) key[c] = k;
    }
  } while (false);
#pragma unroll
  for (int c = 0; c < 8; c++) cand_key[8 * t + c] = key[c];
  if (out_of_range) atomicAdd(A.vol.state + 2, out_of_range);
}

__global__ __launch_bounds__(kThreads) void k_alloc_insert(const unsigned long long* __restrict__ cand_key, unsigned n,
                                                           unsigned* __restrict__ table, unsigned mask) {
  // The 256 candidates of a block - some ten neighbouring pixels - name few bricks: a set of the block's own in LDS
  // first, then only its representatives (the block's smallest index of each key) go to the view's table.  The
  // smallest index of a key over the view is the smallest of its blocks' smallest: the table ends as it would with
  // every candidate inserted, without millions of atomics on the few hundred slots a view's new bricks take (a view
  // of 7.4 M candidates and 368 new bricks: 514 us with every candidate inserted).
  __shared__ unsigned s_table[kLocalSlots];
  const auto same = [&](unsigned a, unsigned b) { return cand_key[a] == cand_key[b]; };
  for (int e = threadIdx.x; e < kLocalSlots; e += kThreads) s_table[e] = kSetEmpty;
  __syncthreads();
  const unsigned c = blockIdx.x * kThreads + threadIdx.x;
  if (c < n) {
    const unsigned long long key = cand_key[c];
    if (key != kNoKey) set_insert(s_table, (unsigned)kLocalSlots - 1, (unsigned)(mix64(key) >> 32), c, same);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kLocalSlots; e += kThreads) {
    const unsigned i = s_table[e];
    if (i != kSetEmpty) set_insert(table, mask, (unsigned)mix64(cand_key[i]), i, same);
  }
}

__global__ __launch_bounds__(kThreads) void k_alloc_flag(AllocScratch S, unsigned n, unsigned mask) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const unsigned c = blockIdx.x * kThreads + threadIdx.x;
  bool rep = false;
  if (c < n) {
    const unsigned long long key = S.cand_key[c];
    if (key != kNoKey)
      rep = set_find(S.table, mask, (unsigned)mix64(key), c,
                     [&](unsigned a, unsigned b) { return S.cand_key[a] == S.cand_key[b]; }) == c;
  }
  unsigned v = rep ? 1u : 0u, f = 0u, tv, tf;
  block_scan2(v, f, tv, tf, s_w);
  if (c < n) S.rel[c] = rep ? (unsigned short)v : kNoRank;
  if (threadIdx.x == 0) S.base[blockIdx.x] = make_uint2(tv, 0u);
}

__global__ __launch_bounds__(kThreads) void k_alloc_scan(AllocScratch S, int nblocks, int* __restrict__ state, int cap) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const uint2 c = scan_block_totals(
      nblocks, s_w, [&](int b) { return S.base[b]; }, [&](int b, uint2 run, uint2) { S.base[b] = run; });
  if (threadIdx.x == 0) {
    const int old = min(max(state[0], 0), cap);
    const long long want = (long long)c.x;
    const long long kept = min(want, (long long)(cap - old));
    *S.view_base = old;
    state[0] = old + (int)kept;
    state[1] = (int)min((long long)state[1] + (want - kept), 0x7fffffffll);
    state[3] = (int)min(want, 0x7fffffffll);
  }
}

__global__ __launch_bounds__(kThreads) void k_alloc_commit(AllocScratch S, unsigned n, mgs_sparse_tsdf_volume V, unsigned map_mask) {
  const unsigned c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  const unsigned short r = S.rel[c];
  if (r == kNoRank) return;
  const long long id = (long long)*S.view_base + S.base[blockIdx.x].x + r;
  if (id >= V.max_bricks) return;
  const unsigned long long key = S.cand_key[c];
  int b[3];
  coords_of(key, b);
#pragma unroll
  for (int a = 0; a < 3; a++) V.brick_coords[3 * id + a] = b[a];
  map_insert(keys_of(V), V.map_vals, map_mask, key, (int)id);
}

__global__ __launch_bounds__(kThreads) void k_sparse_register(mgs_sparse_tsdf_volume V, int first, int count, unsigned map_mask) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e == 0) V.state[0] = first + count;
  if (e >= count) return;
  const int id = first + e;
  const int* b = V.brick_coords + 3 * (size_t)id;
  if (!coord_ok(b[0]) || !coord_ok(b[1]) || !coord_ok(b[2])) return;
  map_insert(keys_of(V), V.map_vals, map_mask, key_of(b[0], b[1], b[2]), id);
}

// ---- integration (tsdf.hip's k_tsdf_integrate on the points of one brick) --------------------------------------------
__device__ __forceinline__ void load4(const float* __restrict__ p, bool vec, float v[4]) {
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = p[e];
  }
}

__device__ __forceinline__ void store4(float* __restrict__ p, bool vec, const float v[4], const bool upd[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);      // lanes without an update hold what was loaded
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (upd[e]) p[e] = v[e];
  }
}

__global__ __launch_bounds__(kIntThreads) void k_sparse_integrate(mgs_sparse_tsdf_view_args A, int vec_i) {
  const bool vec = vec_i != 0;
  const int brick = blockIdx.x;
  if (brick >= min(A.vol.state[0], A.vol.max_bricks)) return;
  const int i0 = kB * A.vol.brick_coords[3 * brick], j0 = kB * A.vol.brick_coords[3 * brick + 1],
            k0 = kB * A.vol.brick_coords[3 * brick + 2];
  const Pinhole cam = pinhole_of(A.T, A.fx, A.fy, A.cx, A.cy, A.z_near);
  const float vs = A.vol.voxel_size;
  const float* origin = A.vol.origin;
  const float fW = (float)A.width, fH = (float)A.height;
  {  // ---- brick culling: the same for every thread of the workgroup
    const int i1 = i0 + kB - 1, j1 = j0 + kB - 1, k1 = k0 + kB - 1;
    float m = 0.f, zmin = INFINITY, zmax = -INFINITY;
    float gl = -INFINITY, gr = INFINITY, gt = -INFINITY, gb = INFINITY;       // max of left / top, min of right / bottom
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const float px = lattice(origin[0], (c & 1) ? i1 : i0, vs), py = lattice(origin[1], (c & 2) ? j1 : j0, vs),
                  pz = lattice(origin[2], (c & 4) ? k1 : k0, vs);
      const float xc = cam_row(cam, 0, px, py, pz), yc = cam_row(cam, 1, px, py, pz), zc = cam_row(cam, 2, px, py, pz);
#pragma unroll
      for (int r = 0; r < 3; r++)
        m = fmaxf(m, fabsf(cam.r[r][0] * px) + fabsf(cam.r[r][1] * py) + fabsf(cam.r[r][2] * pz) + fabsf(cam.r[r][3]));
      finite = finite && fabsf(xc) <= 3.0e38f && fabsf(yc) <= 3.0e38f && fabsf(zc) <= 3.0e38f;
      zmin = fminf(zmin, zc); zmax = fmaxf(zmax, zc);
      gl = fmaxf(gl, A.fx * xc + (A.cx + 0.5f) * zc);
      gr = fminf(gr, A.fx * xc + (A.cx + 0.5f - fW) * zc);
      gt = fmaxf(gt, A.fy * yc + (A.cy + 0.5f) * zc);
      gb = fminf(gb, A.fy * yc + (A.cy + 0.5f - fH) * zc);
    }
    if (finite && m <= 1.0e30f) {
      const float E = 1.0e-5f * m;
      const float M = 2.f * (A.fx + A.fy + fabsf(A.cx) + fabsf(A.cy) + fW + fH + 2.f) * E;
      bool cull = zmax < A.z_near - E;
      if (A.depth_max >= 0.f && A.depth_max <= 3.0e38f) cull = cull || zmin > A.depth_max + A.trunc + E;
      if (A.z_near >= 0.f) cull = cull || gl < -M || gr > M || gt < -M || gb > M;
      if (cull) return;
    }
  }
  const int tid = threadIdx.x;
  const int li = 4 * (tid & 1), lj = (tid >> 1) & 7, lk = tid >> 4;
  const int i = i0 + li, j = j0 + lj, k = k0 + lk;
  const float py = lattice(origin[1], j, vs), pz = lattice(origin[2], k, vs);
  int pix[4];
  float zc4[4];
  bool any = false;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    pix[e] = -1;
    zc4[e] = 0.f;
    const float px = lattice(origin[0], i + e, vs);
    float u, v, zc;
    int x, y;
    if (!project(cam, px, py, pz, u, v, zc)) continue;
    if (!round_to_pixel(u, v, fW, fH, x, y)) continue;
    pix[e] = y * A.width + x;
    zc4[e] = zc;
    any = true;
  }
  if (!any) return;
  const float w = A.view_weight;
  float tn[4];
  bool upd[4];
  any = false;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    upd[e] = false;
    tn[e] = 0.f;
    if (pix[e] < 0) continue;
    float d = A.depth[pix[e]];
    if (A.opacity) {
      const float o = A.opacity[pix[e]];
      if (o < A.min_opacity) continue;
      if (A.normalize) d = __fdiv_rn(d, o);
    }
    if (!(d > A.depth_min && d <= A.depth_max)) continue;
    const float sdf = sub_rn(d, zc4[e]);
    if (sdf < -A.trunc) continue;
    tn[e] = fminf(1.f, __fdiv_rn(sdf, A.trunc));
    upd[e] = true;
    any = true;
  }
  if (!any) return;
  const size_t base = (size_t)brick * kBP + (size_t)((lk * kB + lj) * kB + li);
  const size_t n = (size_t)A.vol.max_bricks * kBP;
  float D[4], W[4], W1[4];
  load4(A.vol.tsdf + base, vec, D);
  load4(A.vol.weight + base, vec, W);
#pragma unroll
  for (int e = 0; e < 4; e++) W1[e] = add_rn(W[e], w);
  if (A.image) {
    const size_t HW = (size_t)A.width * A.height;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float Cc[4];
      load4(A.vol.color + c * n + base, vec, Cc);
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (upd[e]) Cc[e] = __fdiv_rn(add_rn(mul_rn(W[e], Cc[e]), mul_rn(w, A.image[c * HW + pix[e]])), W1[e]);
      store4(A.vol.color + c * n + base, vec, Cc, upd);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; e++) {
    if (!upd[e]) continue;
    D[e] = __fdiv_rn(add_rn(mul_rn(W[e], D[e]), mul_rn(w, tn[e])), W1[e]);
    W[e] = fminf(W1[e], A.max_weight);
  }
  store4(A.vol.tsdf + base, vec, D, upd);
  store4(A.vol.weight + base, vec, W, upd);
}

// ---- extraction ------------------------------------------------------------------------------------------------------
struct MeshScratch {
  int* nbr;                // [bricks,27] brick id of the neighbour (dx + 1) + 3 (dy + 1) + 9 (dz + 1), -1: absent
  unsigned short* code;    // [n] bits 0-6: owned edges with a vertex, bits 8-11: triangles of the owned cell
  unsigned short* vrel;    // [n] vertices of the block's earlier points
  unsigned short* frel;    // [n] faces of the block's earlier points
  uint2* base;             // [blocks] totals, then exclusive bases: x vertices, y faces
};

static MeshScratch mesh_scratch_of(void* p, size_t bricks, size_t* bytes = nullptr) {
  Carver c(p);
  MeshScratch s;
  const size_t n = bricks * kBP;
  s.nbr = c.take<int>(27 * bricks);
  s.code = c.take<unsigned short>(n);
  s.vrel = c.take<unsigned short>(n);
  s.frel = c.take<unsigned short>(n);
  s.base = c.take<uint2>((size_t)grid_of((long long)n));
  if (bytes) *bytes = c.bytes;
  return s;
}

__global__ __launch_bounds__(kThreads) void k_sparse_neighbors(mgs_sparse_tsdf_volume V, int bricks, int* __restrict__ nbr,
                                                               unsigned map_mask) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= 27 * bricks) return;
  const int id = neighbor_find(V, e, map_mask);
  nbr[e] = id < bricks ? id : -1;      // a brick past the count the caller read does not exist for this extraction
}

// the virtual index of the point (li, lj, lk) of `brick`, each coordinate in [-1, 8]; -1 in an absent brick
__device__ __forceinline__ int virtual_index(const int* __restrict__ nbr, int brick, int li, int lj, int lk) {
  const int q = ((li + kB) >> 3) + 3 * ((lj + kB) >> 3) + 9 * ((lk + kB) >> 3);      // (l + 8) >> 3: 0, 1, 2
  const int id = q == 13 ? brick : nbr[27 * (size_t)brick + q];
  if (id < 0) return -1;
  return id * kBP + (((lk & 7) * kB + (lj & 7)) * kB + (li & 7));
}

__global__ __launch_bounds__(kThreads) void k_sparse_classify(mgs_sparse_tsdf_mesh_args A, MeshScratch S) {
  __shared__ unsigned char s_flag[kH][kH][kH];      // bit 0 inside, bit 1 weight >= min_weight; 0 in an absent brick
  __shared__ unsigned char s_cell[kC][kC][kC];      // cell valid, for base corners -1 .. 7
  const int brick = blockIdx.x, tid = threadIdx.x;
  int in_or = 0, in_and = 1;
  for (int e = tid; e < kH * kH * kH; e += kThreads) {
    const int x = e % kH, y = (e / kH) % kH, z = e / (kH * kH);
    const int p = virtual_index(S.nbr, brick, x - 1, y - 1, z - 1);
    unsigned char f = 0;
    if (p >= 0) f = (A.vol.tsdf[p] < 0.f ? 1 : 0) | (A.vol.weight[p] >= A.min_weight ? 2 : 0);
    s_flag[z][y][x] = f;
    in_or |= f & 1;
    in_and &= f & 1;
  }
  // (both are barriers) a tile whose points and halo all have one sign holds no crossing edge and no triangle
  const int any_in = __syncthreads_or(in_or), all_in = __syncthreads_and(in_and);
  unsigned short* code = S.code + (size_t)brick * kBP;
  if (!any_in || all_in) {
    code[tid] = 0;
    code[tid + kThreads] = 0;
    return;
  }
  for (int e = tid; e < kC * kC * kC; e += kThreads) {
    const int x = e % kC, y = (e / kC) % kC, z = e / (kC * kC);
    unsigned char a = 2;
#pragma unroll
    for (int c = 0; c < 8; c++) a &= s_flag[z + (c >> 2)][y + ((c >> 1) & 1)][x + (c & 1)];
    s_cell[z][y][x] = a >> 1;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < kBP / kThreads; h++) {
    const int lp = tid + h * kThreads;
    const int tx = lp & 7, ty = (lp >> 3) & 7, tz = lp >> 6;
    // flags of the point are at [tz + 1][ty + 1][tx + 1]; the cell with base corner a - d at s_cell[tz + 1 - dz]...
    const int in_a = s_flag[tz + 1][ty + 1][tx + 1] & 1;
    unsigned mask = 0;
#pragma unroll
    for (int s = 0; s < 7; s++) {
      const int o = c_slot_code[s];
      const int ox = o & 1, oy = (o >> 1) & 1, oz = o >> 2;
      const int in_b = s_flag[tz + 1 + oz][ty + 1 + oy][tx + 1 + ox] & 1;
      if (in_a == in_b) continue;
      unsigned any = 0;
#pragma unroll
      for (int d = 0; d < 8; d++) {
        if ((d & o) != 0) continue;
        any |= s_cell[tz + 1 - (d >> 2)][ty + 1 - ((d >> 1) & 1)][tx + 1 - (d & 1)];
      }
      if (any) mask |= 1u << s;
    }
    unsigned nt = 0;
    if (s_cell[tz + 1][ty + 1][tx + 1]) {
      unsigned in8 = 0;
#pragma unroll
      for (int c = 0; c < 8; c++) in8 |= (unsigned)(s_flag[tz + 1 + (c >> 2)][ty + 1 + ((c >> 1) & 1)][tx + 1 + (c & 1)] & 1) << c;
#pragma unroll
      for (int t = 0; t < 6; t++) {
        unsigned cs = 0;
#pragma unroll
        for (int p = 0; p < 4; p++) cs |= ((in8 >> c_tet[t][p]) & 1u) << p;
        nt += c_tet_ntri[cs];
      }
    }
    code[lp] = (unsigned short)(mask | (nt << 8));
  }
}

__global__ __launch_bounds__(kThreads) void k_sparse_prefix(MeshScratch S, int n) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const int p = blockIdx.x * kThreads + threadIdx.x;
  const unsigned c = p < n ? S.code[p] : 0u;
  unsigned v = __popc(c & 0x7fu), f = c >> 8, tv, tf;
  block_scan2(v, f, tv, tf, s_w);
  if (p < n) { S.vrel[p] = (unsigned short)v; S.frel[p] = (unsigned short)f; }
  if (threadIdx.x == 0) S.base[blockIdx.x] = make_uint2(tv, tf);
}

__global__ __launch_bounds__(kThreads) void k_sparse_scan(uint2* __restrict__ base, int nblocks, int* __restrict__ counts) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const uint2 c = scan_block_totals(
      nblocks, s_w, [&](int b) { return base[b]; }, [&](int b, uint2 run, uint2) { base[b] = run; });
  if (threadIdx.x == 0) {
    counts[0] = (int)min(c.x, 0x7fffffffu);
    counts[1] = (int)min(c.y, 0x7fffffffu);
  }
}

__device__ __forceinline__ unsigned vertex_id(const MeshScratch& S, size_t p, int slot) {
  return S.base[p / kThreads].x + S.vrel[p] + __popc((unsigned)S.code[p] & ((1u << slot) - 1u));
}

__global__ __launch_bounds__(kThreads) void k_sparse_emit(mgs_sparse_tsdf_mesh_args A, MeshScratch S, int n) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const unsigned c = S.code[p];
  const unsigned mask = c & 0x7fu, nt = c >> 8;
  if (c == 0u) return;
  const uint2 bb = S.base[blockIdx.x];
  const int brick = p / kBP, lp = p % kBP;
  const int li = lp & 7, lj = (lp >> 3) & 7, lk = lp >> 6;
  const int i = kB * A.vol.brick_coords[3 * brick] + li, j = kB * A.vol.brick_coords[3 * brick + 1] + lj,
            k = kB * A.vol.brick_coords[3 * brick + 2] + lk;
  const float vs = A.vol.voxel_size;
  const float* origin = A.vol.origin;
  const float* tsdf = A.vol.tsdf;
  const float* color = A.vol.color;
  if (mask) {
    unsigned id = bb.x + S.vrel[p];
    const float ta = tsdf[p];
    const float pa[3] = {lattice(origin[0], i, vs), lattice(origin[1], j, vs), lattice(origin[2], k, vs)};
    const size_t np = (size_t)A.vol.max_bricks * kBP;
    float ca[3] = {0.f, 0.f, 0.f};
    if (color && A.colors) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) ca[ch] = color[ch * np + p];
    }
#pragma unroll
    for (int s = 0; s < 7; s++) {
      if (!((mask >> s) & 1u)) continue;
      const int o = c_slot_code[s];
      const int ox = o & 1, oy = (o >> 1) & 1, oz = o >> 2;
      const int q = virtual_index(S.nbr, brick, li + ox, lj + oy, lk + oz);
      if (q >= 0 && id < (unsigned)A.num_verts) {      // q < 0 only if the planes changed since the count
        const float tb = tsdf[q];
        const float f = __fdiv_rn(ta, sub_rn(ta, tb));
        const float pb[3] = {lattice(origin[0], i + ox, vs), lattice(origin[1], j + oy, vs), lattice(origin[2], k + oz, vs)};
#pragma unroll
        for (int ax = 0; ax < 3; ax++) A.verts[3 * (size_t)id + ax] = add_rn(pa[ax], mul_rn(f, sub_rn(pb[ax], pa[ax])));
        if (color && A.colors) {
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            const float cb = color[ch * np + q];
            A.colors[3 * (size_t)id + ch] = add_rn(ca[ch], mul_rn(f, sub_rn(cb, ca[ch])));
          }
        }
      }
      id++;
    }
  }
  if (nt) {      // the owned cell is valid: its eight corners lie in allocated bricks (k_sparse_classify)
    unsigned fid = bb.y + S.frel[p];
    int corner[8];
    unsigned in8 = 0;
    bool whole = true;
#pragma unroll
    for (int cc = 0; cc < 8; cc++) {
      corner[cc] = virtual_index(S.nbr, brick, li + (cc & 1), lj + ((cc >> 1) & 1), lk + (cc >> 2));
      whole = whole && corner[cc] >= 0;
      if (corner[cc] >= 0) in8 |= (tsdf[corner[cc]] < 0.f ? 1u : 0u) << cc;
    }
    if (!whole) return;
    for (int t = 0; t < 6; t++) {
      unsigned cs = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) cs |= ((in8 >> c_tet[t][q]) & 1u) << q;
      const int ntri = c_tet_ntri[cs];
      for (int r = 0; r < ntri; r++) {
        int vid[3];
#pragma unroll
        for (int e = 0; e < 3; e++) {
          const int le = c_tet_tri[cs][3 * r + e];
          const int ca = c_tet[t][c_tet_edge[le][0]], cb = c_tet[t][c_tet_edge[le][1]];     // ca is a subset of cb
          vid[e] = (int)vertex_id(S, (size_t)corner[ca], c_slot_of[ca ^ cb]);
        }
        if (c_tet_flip[t]) { const int x = vid[1]; vid[1] = vid[2]; vid[2] = x; }
        if (fid < (unsigned)A.num_faces) {
          A.faces[3 * (size_t)fid] = vid[0]; A.faces[3 * (size_t)fid + 1] = vid[1]; A.faces[3 * (size_t)fid + 2] = vid[2];
        }
        fid++;
      }
    }
  }
}

// ---- host checks -----------------------------------------------------------------------------------------------------
static int32_t view_status(const mgs_sparse_tsdf_view_args* a) {
  if (!a) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rc = volume_status(&a->vol);
  if (rc == MGS_ERR_BAD_ARGUMENT) return rc;
  if (a->width < 1 || a->height < 1 || !a->T || !a->depth) return MGS_ERR_BAD_ARGUMENT;
  if (!(a->trunc > 0.f) || !(a->fx > 0.f) || !(a->fy > 0.f)) return MGS_ERR_BAD_ARGUMENT;
  if (rc != MGS_OK) return rc;
  if ((int64_t)a->width * a->height > 0x7fffffff) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

static long long candidates(int width, int height, int samples) { return (long long)width * height * 8 * samples; }

static int32_t mesh_status(const mgs_sparse_tsdf_mesh_args* a) {
  if (!a) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rc = volume_status(&a->vol);
  if (rc != MGS_OK) return rc;
  if (a->num_bricks < 1 || a->num_bricks > a->vol.max_bricks || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  return MGS_OK;
}

}  // namespace sparse
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_sparse_tsdf_volume_size(void) { return (int32_t)sizeof(mgs_sparse_tsdf_volume); }
int32_t mgs_sparse_tsdf_view_args_size(void) { return (int32_t)sizeof(mgs_sparse_tsdf_view_args); }
int32_t mgs_sparse_tsdf_mesh_args_size(void) { return (int32_t)sizeof(mgs_sparse_tsdf_mesh_args); }

uint64_t mgs_sparse_tsdf_table_size(int32_t max_bricks) {
  return sparse::bricks_ok(max_bricks) ? set_table_size((unsigned long long)max_bricks) : 0;
}

uint64_t mgs_sparse_tsdf_allocate_scratch_bytes(int32_t width, int32_t height, int32_t samples) {
  if (width < 1 || height < 1 || samples < 1) return 0;
  if ((int64_t)width * height > 0x7fffffff) return 0;
  const long long n = sparse::candidates(width, height, samples);
  if (n / samples / 8 != (long long)width * height || n > 0x7fffffffll) return 0;
  return carved_bytes(sparse::alloc_scratch_of, (size_t)n, (size_t)set_table_size((unsigned long long)n));
}

int32_t mgs_sparse_tsdf_allocate(const mgs_sparse_tsdf_view_args* a, void* stream) {
  const int32_t rc = sparse::view_status(a);
  if (rc != MGS_OK) return rc;
  if (a->samples < 1 || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  if ((long long)a->samples > 0x7fffffffll / 8 / ((long long)a->width * a->height)) return MGS_ERR_UNSUPPORTED;
  const long long n = sparse::candidates(a->width, a->height, a->samples);
  const size_t table = (size_t)set_table_size((unsigned long long)n);
  const sparse::AllocScratch S = sparse::alloc_scratch_of(a->scratch, (size_t)n, table);
  const unsigned mask = (unsigned)(table - 1), map_mask = sparse::map_mask_of(a->vol);
  hipStream_t st = (hipStream_t)stream;
  if (!hip_ok("sparse_alloc_fill", hipMemsetAsync(S.table, 0xFF, table * sizeof(unsigned), st))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  const int blocks = grid_of(n);
  launch("sparse_alloc_candidates", sparse::k_alloc_candidates, dim3(grid_of(n / 8)), dim3(sparse::kThreads), st, *a, S.cand_key,
         map_mask);
  launch("sparse_alloc_insert", sparse::k_alloc_insert, dim3(blocks), dim3(sparse::kThreads), st,
         (const unsigned long long*)S.cand_key, (unsigned)n, S.table, mask);
  launch("sparse_alloc_flag", sparse::k_alloc_flag, dim3(blocks), dim3(sparse::kThreads), st, S, (unsigned)n, mask);
  launch("sparse_alloc_scan", sparse::k_alloc_scan, dim3(1), dim3(sparse::kThreads), st, S, blocks, a->vol.state, a->vol.max_bricks);
  launch("sparse_alloc_commit", sparse::k_alloc_commit, dim3(blocks), dim3(sparse::kThreads), st, S, (unsigned)n, a->vol, map_mask);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_sparse_tsdf_integrate(const mgs_sparse_tsdf_view_args* a, void* stream) {
  const int32_t rc = sparse::view_status(a);
  if (rc != MGS_OK) return rc;
  if (!(a->view_weight > 0.f) || !(a->max_weight > 0.f) || (a->image && !a->vol.color)) return MGS_ERR_BAD_ARGUMENT;
  uintptr_t al = reinterpret_cast<uintptr_t>(a->vol.tsdf) | reinterpret_cast<uintptr_t>(a->vol.weight);
  if (a->image) al |= reinterpret_cast<uintptr_t>(a->vol.color);
  const int vec = (al & 15) == 0 ? 1 : 0;      // the planes are multiples of 512 floats apart
  launch("sparse_integrate", sparse::k_sparse_integrate, dim3((unsigned)a->vol.max_bricks), dim3(sparse::kIntThreads),
         (hipStream_t)stream, *a, vec);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_sparse_tsdf_register(const mgs_sparse_tsdf_volume* v, int32_t first, int32_t count, void* stream) {
  const int32_t rc = sparse::volume_status(v);
  if (rc != MGS_OK) return rc;
  if (first < 0 || count < 1 || first > v->max_bricks || count > v->max_bricks - first) return MGS_ERR_BAD_ARGUMENT;
  launch("sparse_register", sparse::k_sparse_register, dim3(grid_of(count)), dim3(sparse::kThreads), (hipStream_t)stream, *v,
         first, count, sparse::map_mask_of(*v));
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

uint64_t mgs_sparse_tsdf_mesh_scratch_bytes(int32_t num_bricks) {
  if (!sparse::bricks_ok(num_bricks)) return 0;
  return carved_bytes(sparse::mesh_scratch_of, (size_t)num_bricks);
}

int32_t mgs_sparse_tsdf_mesh_count(const mgs_sparse_tsdf_mesh_args* a, void* stream) {
  const int32_t rc = sparse::mesh_status(a);
  if (rc != MGS_OK) return rc;
  if (!a->counts) return MGS_ERR_BAD_ARGUMENT;
  const int bricks = a->num_bricks, n = bricks * sparse::kBP;
  const sparse::MeshScratch S = sparse::mesh_scratch_of(a->scratch, (size_t)bricks);
  const int blocks = grid_of(n);
  hipStream_t st = (hipStream_t)stream;
  launch("sparse_neighbors", sparse::k_sparse_neighbors, dim3(grid_of(27ll * bricks)), dim3(sparse::kThreads), st, a->vol, bricks,
         S.nbr, sparse::map_mask_of(a->vol));
  launch("sparse_classify", sparse::k_sparse_classify, dim3((unsigned)bricks), dim3(sparse::kThreads), st, *a, S);
  launch("sparse_prefix", sparse::k_sparse_prefix, dim3(blocks), dim3(sparse::kThreads), st, S, n);
  launch("sparse_scan", sparse::k_sparse_scan, dim3(1), dim3(sparse::kThreads), st, S.base, blocks, a->counts);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_sparse_tsdf_mesh_emit(const mgs_sparse_tsdf_mesh_args* a, void* stream) {
  const int32_t rc = sparse::mesh_status(a);
  if (rc != MGS_OK) return rc;
  if (a->num_verts < 0 || a->num_faces < 0) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts == 0x7fffffff || a->num_faces > 0x7fffffff / 3) return MGS_ERR_UNSUPPORTED;      // saturated counts
  if (a->num_verts == 0 && a->num_faces == 0) return MGS_OK;
  if ((a->num_verts > 0 && !a->verts) || (a->num_faces > 0 && !a->faces)) return MGS_ERR_BAD_ARGUMENT;
  const int n = a->num_bricks * sparse::kBP;
  const sparse::MeshScratch S = sparse::mesh_scratch_of(a->scratch, (size_t)a->num_bricks);
  launch("sparse_emit", sparse::k_sparse_emit, dim3(grid_of(n)), dim3(sparse::kThreads), (hipStream_t)stream, *a, S, n);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
