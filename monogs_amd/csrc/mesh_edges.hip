// The unique undirected edges of an indexed triangle mesh, with the number of faces on each, and its two users: the
// topology report and Taubin / Laplacian smoothing over the unique-edge neighbours (DESIGN.md "Mesh edges and
// smoothing"; the NumPy mirrors mesh_topology.mesh_edges_numpy and mesh_smooth.smooth_mesh_numpy are the contract).
//
// mgs_mesh_edges_count
//   k_me_init      the table to kSetEmpty, the counters, degrees, flags, cursors, block totals and the record to 0
//   k_me_insert    one lane per half-edge 3 f + k: bad faces (counted) and degenerate faces (counted) insert nothing; the
//                  others go into the min-index set of the 64-bit keys (lo << 32) | hi (min_index_set.h)
//   k_me_count     one lane per inserted half-edge: r = find(); integer adds of 1 onto r's multiplicity and, when the
//                  half-edge runs lo -> hi, onto r's forward count
//   k_me_classify  one lane per half-edge, representatives (r == own index) only: the four class counters with one add
//                  per workgroup, integer adds of 1 into the degrees of lo and hi, the store of 2 into the flags of both when
//                  the multiplicity is not 2, the in-block rank and the block total
//   k_me_verts     one lane per vertex: flags |= degree > 0; the in-block exclusive scan of the degrees (the CSR offsets
//                  of smoothing), block totals of the degrees, of the referenced and of the boundary vertices
//   k_compact_scan (compact_scan.h) ONE workgroup: x = edge bases, y = degree bases; record[0..3] = edges, sum of the
//                  degrees, referenced vertices, boundary vertices
// mgs_mesh_edges_emit
//   k_me_emit      a representative writes (lo, hi) and its multiplicity at base + rank, bounded by the host's count
// mgs_mesh_smooth   the launches of the count with degrees and flags in the scratch, then
//   k_ms_prepare   one lane per vertex: the input positions into the first plane, bad (non-finite) vertices counted, the
//                  integer maximum of the |coordinate| bits (one atomicMax per wave)
//   k_ms_fill      one lane per representative: both ends take a slot of the other's CSR row through an integer cursor;
//                  every store bounded by the row length and by the 6 F entries of the plane
//   k_ms_step      once per step, one lane per vertex: the int64 sum of the row's fixed-point neighbours, one division,
//                  the update in single fp64 roundings; src and dst planes alternate, the last dst is the output.  A row
//                  of more than 256 neighbours is summed by its whole workgroup
//
// Order.  The table ends in a state that is a function of the keys alone (min_index_set.h); counters, degrees and
// neighbour sums are integer sums; the flags are stores of the one value 2; the compaction is a stable scan; the order
// in which a row's entries arrive changes no integer sum: two calls give the same bytes.
// Visibility.  Whatever a launch reads plainly was written by an earlier launch; within k_me_insert the table is touched
// by agent-scope atomics only; counters, degrees and cursors only by atomic adds within the launch that adds.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/monogs_raster.h"
#include "compact_scan.h"
#include "launch.h"
#include "min_index_set.h"
#include "rn_math.h"

namespace mgs {
namespace medge {

constexpr int kThreads = 256;
static_assert(kThreads == kCompactThreads, "block_scan2 scans a workgroup of kCompactThreads");

// 3 F <= 2^30: the table of set_table_size(3 F) words then has at most 2^31 entries, so its mask + 1 fits the unsigned
// probe counters that bound set_insert / set_find
constexpr long long kMaxFaces = (1ll << 30) / 3;
constexpr int kFixedBits = 28;                          // K: the largest |coordinate| scales into [2^28, 2^29)
constexpr double kFixedClamp = 4611686018427387904.0;   // 2^62
constexpr unsigned kLongRow = 256;                      // neighbours a single lane walks in k_ms_step

// record[0..3]: k_compact_scan's totals
enum { kRecEdges = 0, kRecDegreeSum = 1, kRecReferenced = 2, kRecBoundaryVerts = 3, kRecBoundary = 4, kRecManifold = 5,
       kRecNonmanifold = 6, kRecInconsistent = 7, kRecDegenerate = 8, kRecBadFaces = 9, kRecBadVerts = 10 };
static_assert(kRecBadVerts < MGS_MESH_EDGES_RECORD_INTS, "the record holds every counter");

struct Scratch {
  int* rep;          // [3F] -1: inserts nothing; after k_me_count the representative; after k_me_classify the in-block
                     //      rank of a representative, -1 for every other half-edge
  int* mult;         // [3F] at the representative: half-edges with its key
  int* fwd;          // [3F] at the representative: those that run lo -> hi
  uint4* base;       // [blocks(max(3F,V))] x: edges, y: degrees of the earlier blocks (z, w: referenced, boundary vertices)
  unsigned* tab;     // [set_table_size(3F)]
  unsigned mask;
  // smoothing only
  int* degree;       // [V]
  int* flags;        // [V]
  int* voff;         // [V] in-block exclusive scan of the degrees
  int* cursor;       // [V] entries of the row taken so far
  int* adj;          // [6F] CSR rows: row v starts at base[v / 256].y + voff[v]
  float* plane[2];   // [3V] the positions before and after a step
  unsigned* maxbits; // [1] max over the input of bits(|coordinate|)
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static Scratch scratch_of(void* p, size_t V, size_t F, size_t smooth, size_t* bytes = nullptr) {
  Carver c(p);
  Scratch S{};
  const size_t H = 3 * F;
  S.rep = c.take<int>(H);
  S.mult = c.take<int>(H);
  S.fwd = c.take<int>(H);
  S.base = c.take<uint4>((size_t)grid_of((long long)(V > H ? V : H)));
  const size_t t = (size_t)set_table_size(H);
  S.tab = c.take<unsigned>(t);
  S.mask = (unsigned)(t - 1);
  if (smooth) {
    S.degree = c.take<int>(V);
    S.flags = c.take<int>(V);
    S.voff = c.take<int>(V);
    S.cursor = c.take<int>(V);
    S.adj = c.take<int>(6 * F);
    S.plane[0] = c.take<float>(3 * V);
    S.plane[1] = c.take<float>(3 * V);
    S.maxbits = c.take<unsigned>(1);
  }
  if (bytes) *bytes = c.bytes;
  return S;
}

// what the launches of the count work on: the caller's outputs (mgs_mesh_edges_count) or planes of the scratch
struct Mesh {
  const int* faces;
  int V, H;          // vertices, half-edges
  int* degree;       // [V]
  int* flags;        // [V]
  int* record;
};

__device__ __forceinline__ unsigned home_of_key(unsigned long long key) { return (unsigned)mix64(key); }

// the two indices of half-edge h = 3 f + k: from faces[f,k] to faces[f,(k+1)%3]
__device__ __forceinline__ void half_edge(const int* __restrict__ faces, unsigned h, int& u, int& v) {
  const unsigned k = h % 3;
  u = faces[h];
  v = faces[k == 2 ? h - 2 : h + 1];
}
__device__ __forceinline__ unsigned long long key_of(int u, int v) {
  const unsigned lo = (unsigned)(u < v ? u : v), hi = (unsigned)(u < v ? v : u);
  return ((unsigned long long)lo << 32) | hi;
}

// does the inserted half-edge j have the key `key`
struct SameEdge {
  const int* faces;
  unsigned long long key;
  __device__ bool operator()(unsigned j, unsigned) const {
    int u, v;
    half_edge(faces, j, u, v);
    return key_of(u, v) == key;
  }
};

// *counter += the wave's lanes with `flag`: one add per wave that has any
__device__ __forceinline__ void count_lanes(bool flag, int* __restrict__ counter) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, __popcll(m));
}

// ---- the edge set -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_me_init(Scratch S, Mesh M, int nblocks) {
  const size_t stride = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + threadIdx.x;
  for (size_t i = first; i <= S.mask; i += stride) S.tab[i] = kSetEmpty;
  for (size_t i = first; i < (size_t)M.H; i += stride) { S.mult[i] = 0; S.fwd[i] = 0; }
  for (size_t i = first; i < (size_t)M.V; i += stride) {
    M.degree[i] = 0;
    M.flags[i] = 0;
    if (S.cursor) S.cursor[i] = 0;
  }
  for (size_t i = first; i < (size_t)nblocks; i += stride) S.base[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0) {
    if (threadIdx.x < MGS_MESH_EDGES_RECORD_INTS) M.record[threadIdx.x] = 0;
    if (threadIdx.x == 0 && S.maxbits) *S.maxbits = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_me_insert(Scratch S, Mesh M) {
  const unsigned h = blockIdx.x * kThreads + threadIdx.x;
  bool bad = false, degenerate = false;
  if (h < (unsigned)M.H) {
    const unsigned f3 = h - h % 3;
    const int a = M.faces[f3], b = M.faces[f3 + 1], c = M.faces[f3 + 2];
    const unsigned V = (unsigned)M.V;
    bad = !((unsigned)a < V && (unsigned)b < V && (unsigned)c < V);
    degenerate = !bad && (a == b || b == c || a == c);
    S.rep[h] = bad || degenerate ? -1 : 0;
    if (!bad && !degenerate) {
      int u, v;
      half_edge(M.faces, h, u, v);
      const unsigned long long key = key_of(u, v);
      set_insert(S.tab, S.mask, home_of_key(key), h, SameEdge{M.faces, key});
    }
  }
  const bool first = h % 3 == 0;                        // a face is counted by its first half-edge
  count_lanes(bad && first, M.record + kRecBadFaces);
  count_lanes(degenerate && first, M.record + kRecDegenerate);
}

__global__ __launch_bounds__(kThreads) void k_me_count(Scratch S, Mesh M) {
  const unsigned h = blockIdx.x * kThreads + threadIdx.x;
  if (h >= (unsigned)M.H || S.rep[h] < 0) return;
  int u, v;
  half_edge(M.faces, h, u, v);
  const unsigned long long key = key_of(u, v);
  const unsigned r = set_find(S.tab, S.mask, home_of_key(key), h, SameEdge{M.faces, key});
  if (r >= (unsigned)M.H) {                             // not met: every inserted key is in the table
    S.rep[h] = -1;
    return;
  }
  S.rep[h] = (int)r;
  atomicAdd(&S.mult[r], 1);
  if (u < v) atomicAdd(&S.fwd[r], 1);
}

__global__ __launch_bounds__(kThreads) void k_me_classify(Scratch S, Mesh M) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const unsigned h = blockIdx.x * kThreads + threadIdx.x;
  const bool is_rep = h < (unsigned)M.H && S.rep[h] == (int)h;
  int m = 0, c = 0;
  if (is_rep) {
    m = S.mult[h];
    c = S.fwd[h];
    int u, v;
    half_edge(M.faces, h, u, v);                        // both in [0,V): the half-edge was inserted
    atomicAdd(&M.degree[u], 1);
    atomicAdd(&M.degree[v], 1);
    if (m != 2) { M.flags[u] = 2; M.flags[v] = 2; }     // the one value, whoever writes it
  }
  // one add per workgroup and class that has any: with one per wave, the 50 000 waves of a million faces met at the four
  // words (577 us for this launch)
  const int boundary = __syncthreads_count(is_rep && m == 1), manifold = __syncthreads_count(is_rep && m == 2);
  const int nonmanifold = __syncthreads_count(is_rep && m >= 3), inconsistent = __syncthreads_count(is_rep && m == 2 && c != 1);
  unsigned e = is_rep ? 1u : 0u, none = 0, te, tn;
  block_scan2(e, none, te, tn, s_w);
  if (h < (unsigned)M.H) S.rep[h] = is_rep ? (int)e : -1;
  if (threadIdx.x == 0) {
    S.base[blockIdx.x].x = te;
    if (boundary) atomicAdd(M.record + kRecBoundary, boundary);
    if (manifold) atomicAdd(M.record + kRecManifold, manifold);
    if (nonmanifold) atomicAdd(M.record + kRecNonmanifold, nonmanifold);
    if (inconsistent) atomicAdd(M.record + kRecInconsistent, inconsistent);
  }
}

__global__ __launch_bounds__(kThreads) void k_me_verts(Scratch S, Mesh M) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  unsigned d = 0;
  int fl = 0;
  if (i < M.V) {
    d = (unsigned)M.degree[i];
    fl = M.flags[i] | (d > 0 ? 1 : 0);
    M.flags[i] = fl;
  }
  const unsigned referenced = (unsigned)__syncthreads_count(fl & 1), boundary = (unsigned)__syncthreads_count(fl & 2);
  unsigned none = 0, td, tn;
  block_scan2(d, none, td, tn, s_w);
  if (S.voff && i < M.V) S.voff[i] = (int)d;
  if (threadIdx.x == 0) {
    uint4* b = S.base + blockIdx.x;                     // x belongs to k_me_classify
    b->y = td; b->z = referenced; b->w = boundary;
  }
}

__global__ __launch_bounds__(kThreads) void k_me_emit(Scratch S, Mesh M, int* __restrict__ edges,
                                                      int* __restrict__ edge_faces, int out_num_edges) {
  const unsigned h = blockIdx.x * kThreads + threadIdx.x;
  if (h >= (unsigned)M.H) return;
  const int r = S.rep[h];
  if (r < 0) return;
  const unsigned id = S.base[h / kThreads].x + (unsigned)r;
  if (id >= (unsigned)out_num_edges) return;
  int u, v;
  half_edge(M.faces, h, u, v);
  edges[2 * (size_t)id] = u < v ? u : v;
  edges[2 * (size_t)id + 1] = u < v ? v : u;
  edge_faces[id] = S.mult[h];
}

// ---- smoothing --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_bits(unsigned b) { return (b & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(kThreads) void k_ms_prepare(const float* __restrict__ verts, int V, float* __restrict__ dst,
                                                         Scratch S, int* __restrict__ record) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  bool bad = false;
  unsigned mx = 0;
  if (i < V) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      const float x = verts[3 * (size_t)i + ax];
      const unsigned b = __float_as_uint(x);
      bad = bad || !finite_bits(b);
      mx = max(mx, b & 0x7FFFFFFFu);
      dst[3 * (size_t)i + ax] = x;
    }
  }
  count_lanes(bad, record + kRecBadVerts);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
  // the word only rises: a stale (smaller) read only costs an atomic that changes nothing, so the read is a plain one
  // that a cache may answer (an agent-scope read per wave, all of one word: 100 us at 530 000 vertices)
  if ((threadIdx.x & 63) == 0 && mx > *S.maxbits) atomicMax(S.maxbits, mx);
}

// where row v of the adjacency starts
__device__ __forceinline__ unsigned row_of(const Scratch& S, int v) { return S.base[v / kThreads].y + (unsigned)S.voff[v]; }

__global__ __launch_bounds__(kThreads) void k_ms_fill(Scratch S, Mesh M, unsigned capacity) {
  const unsigned h = blockIdx.x * kThreads + threadIdx.x;
  if (h >= (unsigned)M.H || S.rep[h] < 0) return;
  int u, v;
  half_edge(M.faces, h, u, v);
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const int at = side ? v : u, other = side ? u : v;
    const unsigned j = (unsigned)atomicAdd(&S.cursor[at], 1), slot = row_of(S, at) + j;
    if (j < (unsigned)S.degree[at] && slot < capacity) S.adj[slot] = other;
  }
}

// q(p) of the contract: the exact scaling by 2^shift, clamped to +-2^62, truncated
__device__ __forceinline__ long long fixed_of(float p, int shift) {
  return (long long)fmax(fmin(ldexp((double)p, shift), kFixedClamp), -kFixedClamp);
}

// sum[ax] += q of the neighbours first, first + stride, ... of the row of d entries at `row`
__device__ __forceinline__ void row_sum(const Scratch& S, int V, const float* __restrict__ src, unsigned row, unsigned d,
                                        unsigned first, unsigned stride, int shift, unsigned capacity,
                                        unsigned long long (&sum)[3]) {
  for (unsigned j = first; j < d && row + j < capacity; j += stride) {
    const int u = S.adj[row + j];
    if ((unsigned)u >= (unsigned)V) continue;           // only if the faces changed under the call
#pragma unroll
    for (int ax = 0; ax < 3; ax++) sum[ax] += (unsigned long long)fixed_of(src[3 * (size_t)u + ax], shift);
  }
}

// A row of up to kLongRow neighbours is walked by the vertex's own lane.  A longer one (the hub of a fan) is summed by
// the whole workgroup, 256 entries per trip, after the short rows: one lane took 289 ms per step for a row of a million.
// The sums are integers, so the split changes no bit.
__global__ __launch_bounds__(kThreads) void k_ms_step(Scratch S, int V, const float* __restrict__ src,
                                                      float* __restrict__ dst, double w, int pin, unsigned capacity) {
  __shared__ unsigned char s_long[kThreads];
  __shared__ unsigned long long s_part[kThreads / 64][3];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  float p[3] = {0.f, 0.f, 0.f};
  unsigned d = 0;
  bool moves = false;
  if (i < V) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) p[ax] = src[3 * (size_t)i + ax];
    d = (unsigned)S.degree[i];
    moves = d > 0 && !(pin && (S.flags[i] & 2));
  }
  const bool is_long = moves && d > kLongRow;
  const int E = (int)(*S.maxbits >> 23) - 127;
  unsigned long long sum[3] = {0, 0, 0};                // unsigned: the wrap-around of the contract, defined
  if (moves && !is_long) row_sum(S, V, src, row_of(S, i), d, 0, 1, kFixedBits - E, capacity, sum);
  s_long[threadIdx.x] = is_long ? 1 : 0;
  if (__syncthreads_or(is_long)) {                      // uniform; behind its barrier s_long is written
    for (int t = 0; t < kThreads; t++) {
      if (!s_long[t]) continue;                         // uniform
      const int v = blockIdx.x * kThreads + t;
      unsigned long long part[3] = {0, 0, 0};
      row_sum(S, V, src, row_of(S, v), (unsigned)S.degree[v], threadIdx.x, kThreads, kFixedBits - E, capacity, part);
#pragma unroll
      for (int ax = 0; ax < 3; ax++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part[ax] += (unsigned long long)__shfl_xor((long long)part[ax], off);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][ax] = part[ax];
      }
      __syncthreads();
      if ((int)threadIdx.x == t) {
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
#pragma unroll
          for (int q = 0; q < kThreads / 64; q++) sum[ax] += s_part[q][ax];
        }
      }
      __syncthreads();                                  // s_part is free for the next long row
    }
  }
  if (i >= V) return;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    float out = p[ax];
    if (moves) {
      const double m = ldexp(div_rn((double)(long long)sum[ax], (double)d), E - kFixedBits), P = (double)p[ax];
      out = (float)add_rn(P, mul_rn(w, add_rn(m, -P)));
    }
    dst[3 * (size_t)i + ax] = out;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int32_t sizes_status(int32_t V, int32_t F, const void* faces, const void* scratch, const void* record) {
  if (V < 0 || F < 0 || !scratch || !record) return MGS_ERR_BAD_ARGUMENT;
  if (F > 0 && !faces) return MGS_ERR_BAD_ARGUMENT;
  if (V > kMaxItems || F > kMaxFaces) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

static int blocks_of(const Mesh& M) { return grid_of(M.V > M.H ? M.V : M.H); }

// k_me_init .. k_compact_scan
static void launch_count(const Scratch& S, const Mesh& M, hipStream_t st) {
  const dim3 th(kThreads);
  const int hblocks = grid_of(M.H), vblocks = grid_of(M.V), blocks = blocks_of(M);
  // a grid-stride fill, four entries per lane and trip at the usual sizes
  const long long entries = (long long)S.mask + 1, per = 4 * kThreads;
  const int init_blocks = (int)(entries / per < 1 ? 1 : (entries / per > 65536 ? 65536 : entries / per));
  launch("me_init", k_me_init, dim3(init_blocks), th, st, S, M, blocks);
  if (hblocks > 0) {
    launch("me_insert", k_me_insert, dim3(hblocks), th, st, S, M);
    launch("me_count", k_me_count, dim3(hblocks), th, st, S, M);
    launch("me_classify", k_me_classify, dim3(hblocks), th, st, S, M);
  }
  if (vblocks > 0) launch("me_verts", k_me_verts, dim3(vblocks), th, st, S, M);
  launch("me_scan", k_compact_scan, dim3(1), th, st, S.base, blocks, M.record);
}

}  // namespace medge
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_mesh_edges_args_size(void) { return (int32_t)sizeof(mgs_mesh_edges_args); }
int32_t mgs_mesh_smooth_args_size(void) { return (int32_t)sizeof(mgs_mesh_smooth_args); }

uint64_t mgs_mesh_edges_scratch_bytes(int32_t num_verts, int32_t num_faces) {
  if (num_verts < 0 || num_faces < 0 || num_verts > kMaxItems || num_faces > medge::kMaxFaces) return 0;
  return carved_bytes(medge::scratch_of, (size_t)num_verts, (size_t)num_faces, (size_t)0);
}

uint64_t mgs_mesh_smooth_scratch_bytes(int32_t num_verts, int32_t num_faces) {
  if (num_verts < 0 || num_faces < 0 || num_verts > kMaxItems || num_faces > medge::kMaxFaces) return 0;
  return carved_bytes(medge::scratch_of, (size_t)num_verts, (size_t)num_faces, (size_t)1);
}

int32_t mgs_mesh_edges_count(const mgs_mesh_edges_args* a, void* stream) {
  if (!a) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rc = medge::sizes_status(a->num_verts, a->num_faces, a->faces, a->scratch, a->record);
  if (rc != MGS_OK) return rc;
  if (a->num_verts > 0 && (!a->vertex_degree || !a->vertex_flags)) return MGS_ERR_BAD_ARGUMENT;
  const medge::Scratch S = medge::scratch_of(a->scratch, (size_t)a->num_verts, (size_t)a->num_faces, 0);
  const medge::Mesh M{a->faces, a->num_verts, 3 * a->num_faces, a->vertex_degree, a->vertex_flags, a->record};
  medge::launch_count(S, M, (hipStream_t)stream);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_edges_emit(const mgs_mesh_edges_args* a, void* stream) {
  if (!a) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rc = medge::sizes_status(a->num_verts, a->num_faces, a->faces, a->scratch, a->record);
  if (rc != MGS_OK) return rc;
  if (a->out_num_edges < 0 || (long long)a->out_num_edges > 3ll * a->num_faces) return MGS_ERR_BAD_ARGUMENT;
  if (a->out_num_edges == 0) return MGS_OK;
  if (!a->edges || !a->edge_faces) return MGS_ERR_BAD_ARGUMENT;
  const medge::Scratch S = medge::scratch_of(a->scratch, (size_t)a->num_verts, (size_t)a->num_faces, 0);
  const medge::Mesh M{a->faces, a->num_verts, 3 * a->num_faces, a->vertex_degree, a->vertex_flags, a->record};
  launch("me_emit", medge::k_me_emit, dim3(grid_of(M.H)), dim3(medge::kThreads), (hipStream_t)stream, S, M, a->edges,
         a->edge_faces, a->out_num_edges);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_smooth(const mgs_mesh_smooth_args* a, void* stream) {
  if (!a) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rc = medge::sizes_status(a->num_verts, a->num_faces, a->faces, a->scratch, a->record);
  if (rc != MGS_OK) return rc;
  if (a->num_verts > 0 && (!a->verts || !a->out_verts)) return MGS_ERR_BAD_ARGUMENT;
  if (a->iterations < 0 || a->iterations > MGS_MESH_SMOOTH_MAX_ITERATIONS) return MGS_ERR_BAD_ARGUMENT;
  if (!(a->lam > 0.f && a->lam <= 1.f)) return MGS_ERR_BAD_ARGUMENT;              // a NaN fails both
  if (a->taubin && !(a->mu >= -1.f && a->mu < 0.f)) return MGS_ERR_BAD_ARGUMENT;
  const int V = a->num_verts, F = a->num_faces;
  const medge::Scratch S = medge::scratch_of(a->scratch, (size_t)V, (size_t)F, 1);
  const medge::Mesh M{a->faces, V, 3 * F, S.degree, S.flags, a->record};
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(medge::kThreads);
  medge::launch_count(S, M, st);
  if (V > 0) {
    const int vblocks = grid_of(V), steps = a->iterations * (a->taubin ? 2 : 1);
    const unsigned capacity = 6u * (unsigned)F;
    float* cur = steps == 0 ? a->out_verts : S.plane[0];
    launch("ms_prepare", medge::k_ms_prepare, dim3(vblocks), th, st, a->verts, V, cur, S, a->record);
    if (F > 0 && steps > 0) launch("ms_fill", medge::k_ms_fill, dim3(grid_of(M.H)), th, st, S, M, capacity);
    for (int s = 0; s < steps; s++) {
      float* next = s == steps - 1 ? a->out_verts : (cur == S.plane[0] ? S.plane[1] : S.plane[0]);
      const double w = (double)(a->taubin && (s & 1) ? a->mu : a->lam);
      launch("ms_step", medge::k_ms_step, dim3(vblocks), th, st, S, V, (const float*)cur, next, w,
             a->boundary_free ? 0 : 1, capacity);
      cur = next;
    }
  }
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
