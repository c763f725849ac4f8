// Mesh clean-up: connected components of an indexed triangle mesh, clusters kept by size, vertices / colours / faces
// compacted (DESIGN.md "Mesh clean-up"; the NumPy mirror in monogs_amd/mesh_clean.py is the contract).
//
//   k_cc_init        parent[v] = v, count[v] = 0; the select's histograms, its record and counts[4] cleared
//   k_cc_hook        one thread per face: lock-free union of (a,b), then of (its root, c).  Find both roots, compare-exchange the
//                    LARGER root's parent from itself to the smaller root; on failure go on from the value read.  Every
//                    retry follows a strictly smaller parent, so the loop is bounded by progress; nothing waits for
//                    another workgroup's write.  A root is therefore always the smallest vertex index of its tree.
//   k_cc_flatten     label[v] = root(v); each valid face adds one to count[root(a)] (equal roots combined inside the wave
//                    before the global integer add); faces with an index outside [0,V) are counted into counts[4]
//   k_cc_hist<1,2,3> (keep_largest given) the three histogram levels of radix_select.h over the face counts of the roots
//   k_cc_threshold   one workgroup: the keep_largest-th largest count T, and how many clusters AT T still fit
//   k_tie_prefix     (keep_largest given) rank of every root at T among the roots at T, in ascending label: in-block
//   k_compact_scan   ... and the block bases
//   k_clean_flags    keep flag per vertex (through its label) and per face (through the label of its first index), the
//                    in-block ranks of the kept ones, the block totals, the clusters and the kept clusters of the block
//   k_compact_scan   ONE workgroup, 1024 block totals per trip: exclusive bases, grand totals to `counts`
//   k_compact_emit   gathers vertices and colours, writes the re-indexed faces; every store bounded by the host's counts
//                    (both: compact_scan.h)
//
// Visibility.  During k_cc_hook workgroups on other XCDs write `parent`.  EVERY access to `parent` in that launch is an
// agent-scope relaxed atomic (load, compare-exchange, min): a plain load may return a stale line of this CU's L1 - that
// would only cost retries - but a plain STORE could overwrite, and so lose, a link another workgroup has just made.  The
// path halving of find_root() is an atomic min of a vertex's parent with its grandparent: it only ever lowers a parent,
// to a vertex of the same tree, and never touches a root (a root's parent is itself and nothing smaller is offered).
// k_cc_flatten runs after the launch boundary; it uses the same find_root(), so long chains are halved there too.
//
// No float atomics and no sort: the counts are integer sums, the labels and flags are functions of the input alone, and
// the compaction is a stable scan - two calls give the same bytes.
#include <hip/hip_runtime.h>

#include "../../include/monogs_raster.h"
#include "compact_scan.h"
#include "launch.h"
#include "radix_select.h"

namespace mgs {
namespace mclean {

constexpr int kThreads = 256;
static_assert(kThreads == kCompactThreads, "block_scan2 scans a workgroup of kCompactThreads");

enum { kSelKeepAll = 0, kSelThreshold = 1, kSelNone = 2 };

struct Scratch {
  int* parent;      // [V]
  int* label;       // [V]
  int* count;       // [V] faces of the cluster, at its root
  int* trel;        // [V] in-block rank among the roots at the threshold count
  int* vrel;        // [V] in-block rank among the kept vertices, -1 when dropped
  int* frel;        // [F] the same for faces
  uint4* tbase;     // [blocks(V)] x: ties of the earlier blocks
  uint4* base;      // [blocks(max(V,F))] x: kept vertices, y: kept faces of the earlier blocks (z, w: clusters, kept)
  RadixHists hist;  // kRadixHistInts ints, contiguous from hist.h1
  int* sel;         // [4] mode, T, ties kept
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static Scratch scratch_of(void* p, size_t V, size_t F, size_t* bytes = nullptr) {
  Carver c(p);
  Scratch S{};
  if (int* h = c.take<int>(kRadixHistInts)) S.hist = radix_hists_at(h);
  S.sel = c.take<int>();
  S.parent = c.take<int>(V);
  S.label = c.take<int>(V);
  S.count = c.take<int>(V);
  S.trel = c.take<int>(V);
  S.vrel = c.take<int>(V);
  S.frel = c.take<int>(F);
  S.tbase = c.take<uint4>((size_t)grid_of((long long)V));
  S.base = c.take<uint4>((size_t)grid_of((long long)(V > F ? V : F)));
  if (bytes) *bytes = c.bytes;
  return S;
}

// ---- union-find -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int parent_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree.  parent[y] <= y always, so every step moves to a strictly smaller index.
__device__ __forceinline__ int find_root(int* __restrict__ parent, int x) {
  for (;;) {
    const int p = parent_load(parent + x);
    if (p == x) return x;
    const int g = parent_load(parent + p);
    if (g == p) return p;
    __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // halving: g < p <= the old parent
    x = g;
  }
}

// Joins the trees of a and b; returns a vertex of the joined tree that was its root when last seen.
__device__ __forceinline__ int unite(int* __restrict__ parent, int a, int b) {
  int ra = find_root(parent, a), rb = find_root(parent, b);
  while (ra != rb) {
    const int hi = max(ra, rb), lo = min(ra, rb);
    int seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return lo;
    // hi was hooked by someone else: seen = its new parent < hi, so max(ra, rb) falls with every retry
    ra = find_root(parent, seen);
    rb = find_root(parent, lo);
  }
  return ra;
}

__device__ __forceinline__ bool face_ok(int a, int b, int c, int V) {
  return (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
}

// One integer add per distinct index and wave: the usual mesh is one giant cluster, and so is the usual histogram
// bucket.  All lanes call it.
__device__ __forceinline__ void add_aggregated(int* __restrict__ out, bool ok, int idx) {
  unsigned long long pending = __ballot(ok);
  while (pending) {
    const int lead = __shfl(idx, __ffsll((long long)pending) - 1);
    const unsigned long long same = __ballot(ok && idx == lead) & pending;
    if (ok && idx == lead && __ffsll((long long)same) - 1 == (int)(threadIdx.x & 63)) atomicAdd(&out[lead], __popcll(same));
    pending &= ~same;
  }
}

__global__ __launch_bounds__(kThreads) void k_cc_init(Scratch S, int V, int with_counts, int* __restrict__ counts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < V) {
    S.parent[i] = i;
    if (with_counts) S.count[i] = 0;
  }
  if (!with_counts) return;
  if (i < kRadixHistInts) S.hist.h1[i] = 0;
  if (i < 4) S.sel[i] = 0;
  if (i == 0) counts[4] = 0;
}

__global__ __launch_bounds__(kThreads) void k_cc_hook(const int* __restrict__ faces, int V, int F, int* __restrict__ parent) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  if (!face_ok(a, b, c, V)) return;
  int r = a;                                            // a, or a vertex above it in its tree: the second find starts there
  if (a != b) r = unite(parent, a, b);
  if (a != c && r != c) unite(parent, r, c);
}

__global__ __launch_bounds__(kThreads) void k_cc_flatten(const int* __restrict__ faces, int V, int F, int* __restrict__ parent,
                                                         int* __restrict__ label, int* __restrict__ count,
                                                         int* __restrict__ counts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < V) label[i] = find_root(parent, i);
  if (!count) return;                                   // labels only (uniform)
  bool ok = false;
  int r = 0;
  if (i < F) {
    const int a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    ok = face_ok(a, b, c, V);
    if (ok) r = find_root(parent, a);
  }
  add_aggregated(count, ok, r);
  const unsigned long long bad = __ballot(i < F && !ok);
  if (bad && (threadIdx.x & 63) == 0) atomicAdd(&counts[4], __popcll(bad));
}

// ---- select -----------------------------------------------------------------------------------------------------------
struct LargestRank {      // the K-th largest of `total` keys has ascending rank total - K; K > total: none (keep all)
  int K;
  __device__ int operator()(int total) const { return total - K; }
};

template <int LEVEL>
__global__ __launch_bounds__(kThreads) void k_cc_hist(Scratch S, int V, int K) {
  __shared__ int s_scan[kThreads / 64];
  __shared__ int s_sel[3];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int c = i < V && S.label[i] == i ? S.count[i] : 0;
  if (!__syncthreads_or(c >= 1)) return;                // a block without a root has nothing to add
  const RadixHists H = S.hist;
  RadixSelected sel{0u, 0, 0, true};
  if (LEVEL >= 2) sel = radix_select<kThreads>(H, LEVEL - 1, LargestRank{K}, s_scan, s_sel);
  const RadixBucket rb = radix_level<LEVEL>((unsigned)c, sel.prefix);
  add_aggregated(H.level(LEVEL), sel.any && c >= 1 && rb.counts, (int)rb.bucket);
}

__global__ __launch_bounds__(kThreads) void k_cc_threshold(Scratch S, int K) {
  __shared__ int s_scan[kThreads / 64];
  __shared__ int s_sel[3];
  const RadixHists H = S.hist;
  const RadixSelected sel = radix_select<kThreads>(H, 3, LargestRank{K}, s_scan, s_sel);
  if (threadIdx.x != 0) return;
  if (K == 0) {
    S.sel[0] = kSelNone;
  } else if (!sel.any) {
    S.sel[0] = kSelKeepAll;
  } else {
    // sel.rank of the clusters AT the threshold count sort below the K-th largest: the others, in ascending label, stay
    S.sel[0] = kSelThreshold;
    S.sel[1] = (int)sel.prefix;
    S.sel[2] = H.h3[sel.prefix & 1023u] - sel.rank;
  }
}

// ---- scans (block_scan2: block_scan.h; k_compact_scan and the emit: compact_scan.h) -------------------------------------
__global__ __launch_bounds__(kThreads) void k_tie_prefix(Scratch S, int V) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool tie = S.sel[0] == kSelThreshold && i < V && S.label[i] == i && S.count[i] == S.sel[1];
  unsigned t = tie ? 1u : 0u, z = 0u, tt, tz;
  block_scan2(t, z, tt, tz, s_w);
  if (i < V) S.trel[i] = (int)t;
  if (threadIdx.x == 0) S.tbase[blockIdx.x] = make_uint4(tt, 0u, 0u, 0u);
}

__device__ __forceinline__ bool keep_cluster(const Scratch& S, int root, int K, int min_faces) {
  const int c = S.count[root];
  if (c < max(min_faces, 1)) return false;
  if (K < 0) return true;
  const int mode = S.sel[0], T = S.sel[1];
  if (mode == kSelKeepAll) return true;
  if (mode == kSelNone) return false;
  if (c != T) return c > T;
  return (int)S.tbase[root / kThreads].x + S.trel[root] < S.sel[2];
}

__global__ __launch_bounds__(kThreads) void k_clean_flags(const int* __restrict__ faces, int V, int F, int K, int min_faces,
                                                          Scratch S) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  bool kv = false, root = false;
  if (i < V) {
    const int l = S.label[i];
    kv = keep_cluster(S, l, K, min_faces);
    root = l == i && S.count[i] >= 1;
  }
  bool kf = false;
  if (i < F) {
    const int a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    if (face_ok(a, b, c, V)) kf = keep_cluster(S, S.label[a], K, min_faces);
  }
  const unsigned clusters = (unsigned)__syncthreads_count(root), kept = (unsigned)__syncthreads_count(root && kv);
  unsigned v = kv ? 1u : 0u, f = kf ? 1u : 0u, tv, tf;
  block_scan2(v, f, tv, tf, s_w);
  if (i < V) S.vrel[i] = kv ? (int)v : -1;
  if (i < F) S.frel[i] = kf ? (int)f : -1;
  if (threadIdx.x == 0) S.base[blockIdx.x] = make_uint4(tv, tf, clusters, kept);
}

// launches 1-3; `label` and `count` as k_cc_flatten takes them
static void launch_components(const mgs_mesh_clean_args* a, const Scratch& S, int* label, int* count, hipStream_t st) {
  const int V = a->num_verts, F = a->num_faces;
  const int with_counts = count ? 1 : 0;
  const int init_items = with_counts && V < kRadixHistInts ? kRadixHistInts : V;
  if (init_items > 0) launch("cc_init", k_cc_init, dim3(grid_of(init_items)), dim3(kThreads), st, S, V, with_counts, a->counts);
  if (V > 0 && F > 0) launch("cc_hook", k_cc_hook, dim3(grid_of(F)), dim3(kThreads), st, a->faces, V, F, S.parent);
  const int items = with_counts && F > V ? F : V;
  if (items > 0) launch("cc_flatten", k_cc_flatten, dim3(grid_of(items)), dim3(kThreads), st, a->faces, V, F, S.parent, label, count, a->counts);
}

}  // namespace mclean
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_mesh_clean_args_size(void) { return (int32_t)sizeof(mgs_mesh_clean_args); }

uint64_t mgs_mesh_clean_scratch_bytes(int32_t num_verts, int32_t num_faces) {
  if (num_verts < 0 || num_faces < 0 || num_verts > kMaxItems || num_faces > kMaxItems) return 0;
  return carved_bytes(mclean::scratch_of, (size_t)num_verts, (size_t)num_faces);
}

int32_t mgs_mesh_components(const mgs_mesh_clean_args* a, void* stream) {
  const int32_t rc = mesh_sizes_status(a);
  if (rc != MGS_OK) return rc;
  if (a->num_verts > 0 && !a->labels) return MGS_ERR_BAD_ARGUMENT;
  const mclean::Scratch S = mclean::scratch_of(a->scratch, (size_t)a->num_verts, (size_t)a->num_faces);
  mclean::launch_components(a, S, a->labels, nullptr, (hipStream_t)stream);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_clean_count(const mgs_mesh_clean_args* a, void* stream) {
  const int32_t rc = mesh_sizes_status(a);
  if (rc != MGS_OK) return rc;
  if (!a->counts || a->keep_largest < -1 || a->min_faces < 0) return MGS_ERR_BAD_ARGUMENT;
  const int V = a->num_verts, F = a->num_faces, K = a->keep_largest;
  const mclean::Scratch S = mclean::scratch_of(a->scratch, (size_t)V, (size_t)F);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(mclean::kThreads);
  mclean::launch_components(a, S, S.label, S.count, st);
  const int vblocks = grid_of(V), blocks = grid_of(V > F ? V : F);
  if (K >= 0 && V > 0) {
    launch("cc_hist1", mclean::k_cc_hist<1>, dim3(vblocks), th, st, S, V, K);
    launch("cc_hist2", mclean::k_cc_hist<2>, dim3(vblocks), th, st, S, V, K);
    launch("cc_hist3", mclean::k_cc_hist<3>, dim3(vblocks), th, st, S, V, K);
    launch("cc_threshold", mclean::k_cc_threshold, dim3(1), th, st, S, K);
    launch("tie_prefix", mclean::k_tie_prefix, dim3(vblocks), th, st, S, V);
    launch("tie_scan", k_compact_scan, dim3(1), th, st, S.tbase, vblocks, (int*)nullptr);
  }
  if (blocks > 0) launch("clean_flags", mclean::k_clean_flags, dim3(blocks), th, st, a->faces, V, F, V > 0 ? K : -1, a->min_faces, S);
  launch("clean_scan", k_compact_scan, dim3(1), th, st, S.base, blocks, a->counts);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_clean_emit(const mgs_mesh_clean_args* a, void* stream) {
  const int32_t rc = mesh_sizes_status(a);
  if (rc != MGS_OK) return rc;
  const mclean::Scratch S = mclean::scratch_of(a->scratch, (size_t)a->num_verts, (size_t)a->num_faces);
  return compact_emit("clean_emit", compact_emit_of(*a, S.vrel, S.frel, S.base), (hipStream_t)stream);
}

}  // extern "C"
