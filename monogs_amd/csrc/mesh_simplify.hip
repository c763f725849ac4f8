// Mesh simplification by vertex clustering: the vertices of one grid cell become one vertex at their mean, faces that
// collapse or repeat are dropped (DESIGN.md "Mesh simplification"; the NumPy mirror mesh_simplify.simplify_mesh_numpy
// is the contract).
//
// mgs_mesh_simplify_count
//   k_sp_init     both hash tables to kSetEmpty, the box keys to neutral, the counts record to 0
//   k_sp_box      (origin from the vertices) per-axis minimum of the finite vertices: integer min over order-preserving
//                 keys of the floats, one atomicMin per workgroup, axis and improvement (mesh_eval.hip's k_nn_bbox)
//   k_sp_keys     one lane per vertex: its 63-bit cell key (bad: all ones, counted), its accumulator row and flag cleared
//   k_sp_vinsert  one lane per good vertex into the min-index set of the cell keys (min_index_set.h); a lane whose
//                 predecessor in the wave has its key leaves the insert to it
//   k_sp_label    one lane per good vertex: label = find(), then 64-bit integer adds of its fixed-point fraction and
//                 colour and of 1 into the label's row; a wave whose lanes all have one label adds once
//   k_sp_finsert  one lane per face: bad (counted), collapsed, or inserted into the min-index set of the sorted label
//                 triples
//   k_sp_fkeep    one lane per inserted face: kept iff find() is its own index; a kept face marks its three labels
//   k_sp_ranks    in-block ranks of the marked labels and of the kept faces, block totals; clusters, collapsed faces
//   k_compact_scan  (compact_scan.h) ONE workgroup, 1024 block totals per trip: bases, grand totals to the counts record
// mgs_mesh_simplify_emit
//   k_sp_emit     a marked label writes its mean position and colour at base + rank, a kept face base + rank of its
//                 three labels; every store bounded by the counts the host passed
//
// Order.  The tables end in a state that is a function of the keys alone (min_index_set.h), the sums are integer sums
// below 2^55, the flags are stores of the one value 1, the compaction is a stable scan: two calls give the same bytes.
// Visibility.  Whatever a launch reads plainly was written by an earlier launch; within the insert launches the tables
// are touched by agent-scope atomics only; the accumulators only by atomic adds.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/monogs_raster.h"
#include "compact_scan.h"
#include "launch.h"
#include "min_index_set.h"
#include "rn_math.h"

namespace mgs {
namespace msimp {

constexpr int kThreads = 256;
static_assert(kThreads == kCompactThreads, "block_scan2 scans a workgroup of kCompactThreads");

constexpr unsigned long long kBadKey = ~0ull;
constexpr float kCellLimit = 1048576.f;                 // 2^20: cells lie in [-2^20, 2^20)
constexpr float kFixedOne = 16777216.f;                 // 2^24: the fixed point of fractions and colours
enum { kFaceDropped = 0, kFaceKept = 1, kFaceCollapsed = 2, kFaceDuplicate = 3 };
enum { kCountDuplicates = 4, kCountBadVerts = 5, kCountBadFaces = 6 };      // counts[0..3]: k_compact_scan's totals

struct Scratch {
  unsigned* box;              // [3] order-preserving keys of the per-axis minimum (origin from the vertices)
  unsigned long long* vkey;   // [V] cell key, kBadKey for a bad vertex
  int* label;                 // [V] smallest index of the vertex's cluster, -1 for a bad vertex
  int* cnt;                   // [V] vertices of the cluster, at its label
  long long* sum;             // [3 V] fixed-point sums of the fractions, at the label
  long long* csum;            // [3 V] the same of the colours
  int* vrel;                  // [V] 1 when a kept face names the label; after k_sp_ranks the in-block rank, -1 when dropped
  int* frel;                  // [F] kFace*; after k_sp_ranks the in-block rank, -1 when dropped
  uint4* base;                // [blocks(max(V,F))] x: emitted vertices, y: kept faces of the earlier blocks (z, w: clusters, collapsed)
  unsigned* vtab;             // [set_table_size(V)]
  unsigned* ftab;             // [set_table_size(F)]
  unsigned vmask, fmask;
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static Scratch scratch_of(void* p, size_t V, size_t F, size_t* bytes = nullptr) {
  Carver c(p);
  Scratch S{};
  S.box = c.take<unsigned>(3);
  S.vkey = c.take<unsigned long long>(V);
  S.label = c.take<int>(V);
  S.cnt = c.take<int>(V);
  S.sum = c.take<long long>(3 * V);
  S.csum = c.take<long long>(3 * V);
  S.vrel = c.take<int>(V);
  S.frel = c.take<int>(F);
  S.base = c.take<uint4>((size_t)grid_of((long long)(V > F ? V : F)));
  const size_t tv = (size_t)set_table_size(V), tf = (size_t)set_table_size(F);
  S.vtab = c.take<unsigned>(tv);
  S.ftab = c.take<unsigned>(tf);
  S.vmask = (unsigned)(tv - 1);
  S.fmask = (unsigned)(tf - 1);
  if (bytes) *bytes = c.bytes;
  return S;
}

__device__ __forceinline__ bool finite_bits(unsigned b) { return (b & 0x7F800000u) != 0x7F800000u; }

// unsigned order of the keys = order of the floats (mesh_eval.hip's)
__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float order_key_inv(unsigned k) {
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// the origin of the cells on axis ax: the caller's, or the minimum k_sp_box found (NaN when no vertex is finite)
__device__ __forceinline__ float origin_of(const mgs_mesh_simplify_args& A, const Scratch& S, int ax) {
  return A.origin_from_verts ? order_key_inv(S.box[ax]) : A.origin[ax];
}

// cell c (as a float) and fraction fr of coordinate v: t = (v - o) / cell, c = floor(t), fr = t - c, one rounding each
__device__ __forceinline__ void cell_of(float v, float o, float cell, float& c, float& fr) {
  const float t = __fdiv_rn(sub_rn(v, o), cell);
  c = floorf(t);
  fr = sub_rn(t, c);
}

__device__ __forceinline__ unsigned home_of_key(unsigned long long key) { return (unsigned)mix64(key); }
// a <= b <= c, each below 2^31
__device__ __forceinline__ unsigned home_of_triple(int a, int b, int c) {
  return (unsigned)mix64(mix64(((unsigned long long)(unsigned)a << 32) | (unsigned)b) ^ (unsigned long long)(unsigned)c);
}

__device__ __forceinline__ void sort3(int& a, int& b, int& c) {
  int t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
}

// the sorted labels of face f; false when an index lies outside [0,V) or names a bad vertex
__device__ __forceinline__ bool face_labels(const int* __restrict__ faces, const int* __restrict__ label, int V, int f,
                                            int& a, int& b, int& c) {
  const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
  if (!((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V)) return false;
  a = label[ia]; b = label[ib]; c = label[ic];
  if (a < 0 || b < 0 || c < 0) return false;
  sort3(a, b, c);
  return true;
}

// record[k] += the wave's lanes with `flag`: one add per wave that has any
__device__ __forceinline__ void count_lanes(bool flag, int* __restrict__ counter) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, __popcll(m));
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void add64(long long* p, long long v) {
  if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ---- count ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sp_init(Scratch S, int* __restrict__ counts) {
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i <= S.vmask; i += stride) S.vtab[i] = kSetEmpty;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i <= S.fmask; i += stride) S.ftab[i] = kSetEmpty;
  if (blockIdx.x == 0) {
    if (threadIdx.x < 3) S.box[threadIdx.x] = 0xFFFFFFFFu;
    if (threadIdx.x < MGS_MESH_SIMPLIFY_COUNTS) counts[threadIdx.x] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_sp_box(const float* __restrict__ verts, int V, Scratch S) {
  __shared__ unsigned s_mn[kThreads / 64][3];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  unsigned mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  if (i < V) {
    const float x = verts[3 * (size_t)i], y = verts[3 * (size_t)i + 1], z = verts[3 * (size_t)i + 2];
    if (finite_bits(__float_as_uint(x)) && finite_bits(__float_as_uint(y)) && finite_bits(__float_as_uint(z))) {
      mn[0] = order_key(x); mn[1] = order_key(y); mn[2] = order_key(z);
    }
  }
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mn[ax] = min(mn[ax], (unsigned)__shfl_xor((int)mn[ax], off));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) s_mn[threadIdx.x >> 6][ax] = mn[ax];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int ax = threadIdx.x;
    unsigned lo = s_mn[0][ax];
#pragma unroll
    for (int w = 1; w < kThreads / 64; w++) lo = min(lo, s_mn[w][ax]);
    // the word only falls: a stale (larger) read only costs an atomic that changes nothing
    if (lo < __hip_atomic_load(&S.box[ax], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&S.box[ax], lo);
  }
}

__global__ __launch_bounds__(kThreads) void k_sp_keys(mgs_mesh_simplify_args A, Scratch S) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  bool bad = false;
  if (i < A.num_verts) {
    unsigned long long key = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      const float v = A.verts[3 * (size_t)i + ax];
      float c, fr;
      cell_of(v, origin_of(A, S, ax), A.cell, c, fr);
      // a NaN c fails both comparisons
      if (!finite_bits(__float_as_uint(v)) || !(c >= -kCellLimit && c < kCellLimit)) bad = true;
      else key = (key << 21) | (unsigned long long)((int)c + (1 << 20));
      S.sum[3 * (size_t)i + ax] = 0;
      S.csum[3 * (size_t)i + ax] = 0;
    }
    S.vkey[i] = bad ? kBadKey : key;
    S.label[i] = -1;
    S.cnt[i] = 0;
    S.vrel[i] = 0;
  }
  count_lanes(bad, A.counts + kCountBadVerts);
}

__global__ __launch_bounds__(kThreads) void k_sp_vinsert(int V, Scratch S) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long key = i < V ? S.vkey[i] : kBadKey;
  // A lane whose predecessor in the wave has its key has nothing to add: the first lane of such a run has the run's
  // smallest index and inserts.  Extracted meshes list the vertices of a cell close together, and a million vertices
  // in ONE cell otherwise meet at one slot (5.5 ms; 0.1 ms with this; 38 -> 14 us on the 530 k-vertex lattice).
  const unsigned long long before = __shfl_up(key, 1);
  if (key == kBadKey || ((threadIdx.x & 63) != 0 && before == key)) return;
  const unsigned long long* vkey = S.vkey;
  set_insert(S.vtab, S.vmask, home_of_key(key), (unsigned)i, [&](unsigned j, unsigned) { return vkey[j] == key; });
}

__global__ __launch_bounds__(kThreads) void k_sp_label(mgs_mesh_simplify_args A, Scratch S) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  int l = -1;
  long long q[3] = {0, 0, 0}, qc[3] = {0, 0, 0};
  if (i < A.num_verts) {
    const unsigned long long key = S.vkey[i];
    if (key != kBadKey) {
      const unsigned long long* vkey = S.vkey;
      const unsigned r = set_find(S.vtab, S.vmask, home_of_key(key), (unsigned)i, [&](unsigned j, unsigned) { return vkey[j] == key; });
      l = r == kSetEmpty ? -1 : (int)r;
      S.label[i] = l;
    }
  }
  const bool ok = l >= 0;
  if (ok) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      float c, fr;
      cell_of(A.verts[3 * (size_t)i + ax], origin_of(A, S, ax), A.cell, c, fr);
      q[ax] = (long long)mul_rn(fr, kFixedOne);                       // exact scaling, truncation; 0 <= q <= 2^24
      if (A.colors) qc[ax] = (long long)mul_rn(fminf(fmaxf(A.colors[3 * (size_t)i + ax], 0.f), 1.f), kFixedOne);
    }
  }
  // one cell may hold every vertex: a wave whose lanes share ONE label adds their sums once
  const unsigned long long active = __ballot(ok);
  if (!active) return;                                                // uniform
  const int lead = __shfl(l, __ffsll((long long)active) - 1);
  if (__ballot(ok && l != lead) == 0 && __popcll(active) > 1) {
    long long s[3], sc[3];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) { s[ax] = wave_sum(q[ax]); sc[ax] = wave_sum(qc[ax]); }
    if ((int)(threadIdx.x & 63) == __ffsll((long long)active) - 1) {
      atomicAdd(&S.cnt[lead], __popcll(active));
#pragma unroll
      for (int ax = 0; ax < 3; ax++) { add64(&S.sum[3 * (size_t)lead + ax], s[ax]); add64(&S.csum[3 * (size_t)lead + ax], sc[ax]); }
    }
    return;
  }
  if (!ok) return;
  atomicAdd(&S.cnt[l], 1);
#pragma unroll
  for (int ax = 0; ax < 3; ax++) { add64(&S.sum[3 * (size_t)l + ax], q[ax]); add64(&S.csum[3 * (size_t)l + ax], qc[ax]); }
}

// do faces j and (a, b, c) have one sorted label triple; j was inserted, so its labels are good
struct SameTriple {
  const int* faces;
  const int* label;
  int a, b, c;
  __device__ bool operator()(unsigned j, unsigned) const {
    int x = label[faces[3 * (size_t)j]], y = label[faces[3 * (size_t)j + 1]], z = label[faces[3 * (size_t)j + 2]];
    sort3(x, y, z);
    return x == a && y == b && z == c;
  }
};

__global__ __launch_bounds__(kThreads) void k_sp_finsert(mgs_mesh_simplify_args A, Scratch S) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  bool bad = false;
  if (f < A.num_faces) {
    const int V = A.num_verts;
    const int ia = A.faces[3 * (size_t)f], ib = A.faces[3 * (size_t)f + 1], ic = A.faces[3 * (size_t)f + 2];
    bad = !((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V);
    int a, b, c, code = kFaceDropped;
    if (!bad && face_labels(A.faces, S.label, V, f, a, b, c)) {
      if (a == b || b == c) {
        code = kFaceCollapsed;
      } else {
        code = kFaceKept;                                             // until k_sp_fkeep finds a smaller equal
        set_insert(S.ftab, S.fmask, home_of_triple(a, b, c), (unsigned)f, SameTriple{A.faces, S.label, a, b, c});
      }
    }
    S.frel[f] = code;
  }
  count_lanes(bad, A.counts + kCountBadFaces);
}

__global__ __launch_bounds__(kThreads) void k_sp_fkeep(mgs_mesh_simplify_args A, Scratch S) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= A.num_faces || S.frel[f] != kFaceKept) return;
  int a, b, c;
  if (!face_labels(A.faces, S.label, A.num_verts, f, a, b, c)) return;      // held in k_sp_finsert
  const unsigned first = set_find(S.ftab, S.fmask, home_of_triple(a, b, c), (unsigned)f, SameTriple{A.faces, S.label, a, b, c});
  if (first == (unsigned)f) {
    S.vrel[a] = 1; S.vrel[b] = 1; S.vrel[c] = 1;                      // the one value, whoever writes it
  } else {
    S.frel[f] = kFaceDuplicate;
  }
}

__global__ __launch_bounds__(kThreads) void k_sp_ranks(int V, int F, Scratch S, int* __restrict__ counts) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool kv = i < V && S.vrel[i] == 1, root = i < V && S.label[i] == i;
  const int code = i < F ? S.frel[i] : kFaceDropped;
  const bool kf = code == kFaceKept;
  const unsigned clusters = (unsigned)__syncthreads_count(root), collapsed = (unsigned)__syncthreads_count(code == kFaceCollapsed);
  count_lanes(code == kFaceDuplicate, counts + kCountDuplicates);
  unsigned v = kv ? 1u : 0u, f = kf ? 1u : 0u, tv, tf;
  block_scan2(v, f, tv, tf, s_w);
  if (i < V) S.vrel[i] = kv ? (int)v : -1;
  if (i < F) S.frel[i] = kf ? (int)f : -1;
  if (threadIdx.x == 0) S.base[blockIdx.x] = make_uint4(tv, tf, clusters, collapsed);
}

// ---- emit -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sp_emit(mgs_mesh_simplify_args A, Scratch S) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int V = A.num_verts, F = A.num_faces;
  if (i < V) {
    const int r = S.vrel[i];
    if (r >= 0) {
      const unsigned id = S.base[i / kThreads].x + (unsigned)r;
      if (id < (unsigned)A.out_num_verts) {
        const double den = mul_rn((double)S.cnt[i], (double)kFixedOne);
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
          const float o = origin_of(A, S, ax);
          float c, fr;
          cell_of(A.verts[3 * (size_t)i + ax], o, A.cell, c, fr);          // the label is a vertex of its own cell
          const double m = div_rn((double)S.sum[3 * (size_t)i + ax], den);
          A.out_verts[3 * (size_t)id + ax] = (float)add_rn((double)o, mul_rn(add_rn((double)c, m), (double)A.cell));
          if (A.colors && A.out_colors) A.out_colors[3 * (size_t)id + ax] = (float)div_rn((double)S.csum[3 * (size_t)i + ax], den);
        }
      }
    }
  }
  if (i < F) {
    const int r = S.frel[i];
    if (r >= 0) {
      const unsigned fid = S.base[i / kThreads].y + (unsigned)r;
      if (fid < (unsigned)A.out_num_faces) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
          const int v = A.faces[3 * (size_t)i + e];
          int id = -1;                                  // only if the faces changed since the count
          if ((unsigned)v < (unsigned)V) {
            const int l = S.label[v];
            if (l >= 0 && S.vrel[l] >= 0) id = (int)S.base[l / kThreads].x + S.vrel[l];
          }
          A.out_faces[3 * (size_t)fid + e] = id;
        }
      }
    }
  }
}

static int32_t simplify_status(const mgs_mesh_simplify_args* a) {
  const int32_t rc = mesh_sizes_status(a);
  if (rc != MGS_OK) return rc;
  if (a->num_verts > 0 && !a->verts) return MGS_ERR_BAD_ARGUMENT;
  if (!(a->cell > 0.f) || !std::isfinite(a->cell)) return MGS_ERR_BAD_ARGUMENT;
  if (!a->origin_from_verts && !(std::isfinite(a->origin[0]) && std::isfinite(a->origin[1]) && std::isfinite(a->origin[2])))
    return MGS_ERR_BAD_ARGUMENT;
  return MGS_OK;
}

}  // namespace msimp
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_mesh_simplify_args_size(void) { return (int32_t)sizeof(mgs_mesh_simplify_args); }

uint64_t mgs_mesh_simplify_scratch_bytes(int32_t num_verts, int32_t num_faces) {
  if (num_verts < 0 || num_faces < 0 || num_verts > kMaxItems || num_faces > kMaxItems) return 0;
  return carved_bytes(msimp::scratch_of, (size_t)num_verts, (size_t)num_faces);
}

int32_t mgs_mesh_simplify_count(const mgs_mesh_simplify_args* a, void* stream) {
  const int32_t rc = msimp::simplify_status(a);
  if (rc != MGS_OK) return rc;
  if (!a->counts) return MGS_ERR_BAD_ARGUMENT;
  const int V = a->num_verts, F = a->num_faces;
  const msimp::Scratch S = msimp::scratch_of(a->scratch, (size_t)V, (size_t)F);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(msimp::kThreads);
  const int vblocks = grid_of(V), fblocks = grid_of(F), blocks = vblocks > fblocks ? vblocks : fblocks;
  // the tables hold at most 4 entries per item; a grid-stride fill, four entries per lane and trip at the usual sizes
  const long long entries = (long long)(S.vmask > S.fmask ? S.vmask : S.fmask) + 1;
  const int init_blocks = (int)(entries / (4 * msimp::kThreads) < 1 ? 1 : (entries / (4 * msimp::kThreads) > 65536 ? 65536 : entries / (4 * msimp::kThreads)));
  launch("sp_init", msimp::k_sp_init, dim3(init_blocks), th, st, S, a->counts);
  if (V > 0) {
    if (a->origin_from_verts) launch("sp_box", msimp::k_sp_box, dim3(vblocks), th, st, a->verts, V, S);
    launch("sp_keys", msimp::k_sp_keys, dim3(vblocks), th, st, *a, S);
    launch("sp_vinsert", msimp::k_sp_vinsert, dim3(vblocks), th, st, V, S);
    launch("sp_label", msimp::k_sp_label, dim3(vblocks), th, st, *a, S);
  }
  if (F > 0) {
    launch("sp_finsert", msimp::k_sp_finsert, dim3(fblocks), th, st, *a, S);
    launch("sp_fkeep", msimp::k_sp_fkeep, dim3(fblocks), th, st, *a, S);
  }
  if (blocks > 0) launch("sp_ranks", msimp::k_sp_ranks, dim3(blocks), th, st, V, F, S, a->counts);
  launch("sp_scan", k_compact_scan, dim3(1), th, st, S.base, blocks, a->counts);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_simplify_emit(const mgs_mesh_simplify_args* a, void* stream) {
  const int32_t rc = msimp::simplify_status(a);
  if (rc != MGS_OK) return rc;
  if (a->out_num_verts < 0 || a->out_num_faces < 0) return MGS_ERR_BAD_ARGUMENT;
  if (a->out_num_verts > a->num_verts || a->out_num_faces > a->num_faces) return MGS_ERR_BAD_ARGUMENT;
  if (a->out_num_verts == 0 && a->out_num_faces == 0) return MGS_OK;
  if (a->out_num_verts > 0 && (!a->out_verts || (a->colors && !a->out_colors))) return MGS_ERR_BAD_ARGUMENT;
  if (a->out_num_faces > 0 && !a->out_faces) return MGS_ERR_BAD_ARGUMENT;
  const int V = a->num_verts, F = a->num_faces;
  const msimp::Scratch S = msimp::scratch_of(a->scratch, (size_t)V, (size_t)F);
  launch("sp_emit", msimp::k_sp_emit, dim3(grid_of(V > F ? V : F)), dim3(msimp::kThreads), (hipStream_t)stream, *a, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
