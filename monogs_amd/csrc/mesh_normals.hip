// Mesh normals: unit normals of faces, area-weighted normals of vertices, and the normal-consistency sums of a mesh
// evaluation (DESIGN.md "Mesh normals"; the mirrors in monogs_amd/mesh_normals.py are the contract).
//
// mgs_face_normals
//   k_face_normals   one lane per face: c = (b - a) x (c - a) with the sampler's roundings, L = |c|, n = c / L; bad and
//                    degenerate faces get (0,0,0) and are counted, one integer add per wave that has any
// mgs_vertex_normals
//   k_vn_max         one lane per face: the cross product, the workgroup's integer maximum of the bits of |c.x|, |c.y|,
//                    |c.z| over its usable faces, ONE atomicMax per workgroup - and none when the word already holds as
//                    much; the counts of bad and degenerate faces
//   k_vn_add         one lane per face: the cross product again (three gathers cost less than a [F,3] plane written and
//                    read back), q = trunc(c 2^(30 - E)) by an exact fp64 scaling, nine 64-bit integer atomic adds
//   k_vn_finish      one lane per vertex: the sum as fp64, its length, the quotient, one conversion to fp32
// mgs_mesh_eval_normal_stats / _finish
//   k_normal_stats   kStatBlocks workgroups, grid stride: pairs, sum |t| in fp64, pairs with t < 0, skipped pairs; fixed tree
//   k_normal_finish  ONE workgroup: the partials of both directions in a fixed order, eight doubles of the record
//
// Order.  Every vertex sum is a sum of integers below 2^31 in magnitude, at most F < 2^31 of them: below 2^62, exact in
// any order.  The maximum is an integer maximum.  Nothing else crosses a lane, so two runs give the same bytes.
// Visibility.  The accumulators and the maximum are written by agent-scope atomics only and read after a launch
// boundary.  The relaxed load in front of the atomicMax may see an old (smaller) value: the word only grows, so the
// only cost of that is an atomic that changes nothing.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "rn_math.h"
#include "scratch_carve.h"

namespace mgs {
namespace mnorm {

constexpr int kThreads = 256;
constexpr int kStatBlocks = 256;

__device__ __forceinline__ bool finite_bits(unsigned b) { return (b & 0x7F800000u) != 0x7F800000u; }

// c = (b - a) x (c - a) of face f, the roundings of the sampler's k_face_area; false for an index outside [0,V)
__device__ __forceinline__ bool face_cross(const float* __restrict__ verts, const int* __restrict__ faces, int V, int f,
                                           float c[3]) {
  const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
  if (!((unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V)) return false;
  float e[3], g[3];
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const float a = verts[3 * (size_t)ia + ax];
    e[ax] = sub_rn(verts[3 * (size_t)ib + ax], a);
    g[ax] = sub_rn(verts[3 * (size_t)ic + ax], a);
  }
  c[0] = sub_rn(mul_rn(e[1], g[2]), mul_rn(e[2], g[1]));
  c[1] = sub_rn(mul_rn(e[2], g[0]), mul_rn(e[0], g[2]));
  c[2] = sub_rn(mul_rn(e[0], g[1]), mul_rn(e[1], g[0]));
  return true;
}

// a vertex sum takes the face: every component finite, not all of them zero
__device__ __forceinline__ bool usable(const float c[3]) {
  return finite_bits(__float_as_uint(c[0])) && finite_bits(__float_as_uint(c[1])) && finite_bits(__float_as_uint(c[2])) &&
         (c[0] != 0.f || c[1] != 0.f || c[2] != 0.f);
}

// record[0] += bad, record[1] += degenerate over the wave: one add per wave and counter, none for a zero
__device__ __forceinline__ void count_faces(bool bad, bool degenerate, int* __restrict__ record) {
  const unsigned long long nb = __ballot(bad), nd = __ballot(degenerate);
  if ((threadIdx.x & 63) == 0) {
    if (nb) atomicAdd(&record[0], __popcll(nb));
    if (nd) atomicAdd(&record[1], __popcll(nd));
  }
}

// ---- face normals ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_face_normals(mgs_mesh_normals_args A) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  bool bad = false, degenerate = false;
  if (f < A.num_faces) {
    float c[3], n[3] = {0.f, 0.f, 0.f};
    if (face_cross(A.verts, A.faces, A.num_verts, f, c)) {
      // sqrtf is the correctly rounded root (surface.hip)
      const float L = sqrtf(add_rn(add_rn(mul_rn(c[0], c[0]), mul_rn(c[1], c[1])), mul_rn(c[2], c[2])));
      if (L > 0.f && finite_bits(__float_as_uint(L))) {
#pragma unroll
        for (int ax = 0; ax < 3; ax++) n[ax] = __fdiv_rn(c[ax], L);
      } else {
        degenerate = true;
      }
    } else {
      bad = true;
    }
#pragma unroll
    for (int ax = 0; ax < 3; ax++) A.normals[3 * (size_t)f + ax] = n[ax];
  }
  count_faces(bad, degenerate, A.record);
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------
struct VertexScratch {
  long long* sum;        // [3 V] fixed-point sums
  unsigned* max_bits;    // [1] bits of the largest |component| of a usable cross product
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static VertexScratch vertex_scratch(void* p, size_t V, size_t* bytes = nullptr) {
  Carver c(p);
  VertexScratch S;
  S.sum = c.take<long long>(3 * V);
  S.max_bits = c.take<unsigned>();
  if (bytes) *bytes = c.bytes;
  return S;
}

__global__ __launch_bounds__(kThreads) void k_vn_max(mgs_mesh_normals_args A, VertexScratch S) {
  __shared__ unsigned s_m[kThreads / 64];
  const int f = blockIdx.x * kThreads + threadIdx.x;
  bool bad = false, degenerate = false;
  unsigned m = 0;
  if (f < A.num_faces) {
    float c[3];
    if (!face_cross(A.verts, A.faces, A.num_verts, f, c)) {
      bad = true;
    } else if (!usable(c)) {
      degenerate = true;
    } else {
      m = max(__float_as_uint(fabsf(c[0])), max(__float_as_uint(fabsf(c[1])), __float_as_uint(fabsf(c[2]))));
    }
  }
  count_faces(bad, degenerate, A.record);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kThreads / 64; w++) m = max(m, s_m[w]);
    if (m > __hip_atomic_load(S.max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(S.max_bits, m);
  }
}

__global__ __launch_bounds__(kThreads) void k_vn_add(mgs_mesh_normals_args A, VertexScratch S) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= A.num_faces) return;
  const unsigned mb = *S.max_bits;
  float c[3];
  if (mb == 0 || !face_cross(A.verts, A.faces, A.num_verts, f, c) || !usable(c)) return;
  const int E = ilogb((double)__uint_as_float(mb));
  long long q[3];
#pragma unroll
  for (int ax = 0; ax < 3; ax++) q[ax] = (long long)ldexp((double)c[ax], 30 - E);      // exact scaling, truncation; |q| < 2^31
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int v = A.faces[3 * (size_t)f + k];                                           // in [0,V): face_cross held
#pragma unroll
    for (int ax = 0; ax < 3; ax++)
      if (q[ax]) atomicAdd(reinterpret_cast<unsigned long long*>(S.sum + 3 * (size_t)v + ax), (unsigned long long)q[ax]);
  }
}

__global__ __launch_bounds__(kThreads) void k_vn_finish(mgs_mesh_normals_args A, VertexScratch S) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= A.num_verts) return;
  const double x = (double)S.sum[3 * (size_t)v], y = (double)S.sum[3 * (size_t)v + 1], z = (double)S.sum[3 * (size_t)v + 2];
  const double L = __dsqrt_rn(add_rn(add_rn(mul_rn(x, x), mul_rn(y, y)), mul_rn(z, z)));
  const bool ok = L > 0.0;
  A.normals[3 * (size_t)v] = ok ? (float)div_rn(x, L) : 0.f;
  A.normals[3 * (size_t)v + 1] = ok ? (float)div_rn(y, L) : 0.f;
  A.normals[3 * (size_t)v + 2] = ok ? (float)div_rn(z, L) : 0.f;
}

// ---- normal consistency ------------------------------------------------------------------------------------------------
struct NormalPartial {
  double sum;
  unsigned long long n, flipped, skipped;
};

__device__ __forceinline__ void merge(NormalPartial& a, const NormalPartial& b) {
  a.sum += b.sum; a.n += b.n; a.flipped += b.flipped; a.skipped += b.skipped;
}

// the workgroup's partial in thread 0: a fixed tree over the lanes, then the waves in order (mesh_eval.hip's)
__device__ __forceinline__ NormalPartial block_reduce(NormalPartial p, NormalPartial* s_p) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    NormalPartial o;
    o.sum = __shfl_down(p.sum, off);
    o.n = __shfl_down(p.n, off);
    o.flipped = __shfl_down(p.flipped, off);
    o.skipped = __shfl_down(p.skipped, off);
    merge(p, o);
  }
  if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kThreads / 64; w++) merge(p, s_p[w]);
  return p;
}

// the normal of the face of sample `s`; false without one (no sample, no face, or a (0,0,0) normal)
__device__ __forceinline__ bool sample_normal(const int* __restrict__ face, int num_samples, int s,
                                              const float* __restrict__ normals, int num_faces, float n[3]) {
  if ((unsigned)s >= (unsigned)num_samples) return false;
  const int f = face[s];
  if ((unsigned)f >= (unsigned)num_faces) return false;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) n[ax] = normals[3 * (size_t)f + ax];
  return n[0] != 0.f || n[1] != 0.f || n[2] != 0.f;
}

__global__ __launch_bounds__(kThreads) void k_normal_stats(mgs_mesh_eval_normal_args A, NormalPartial* __restrict__ out) {
  __shared__ NormalPartial s_p[kThreads / 64];
  NormalPartial p{0.0, 0ull, 0ull, 0ull};
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < A.num; i += (long long)kStatBlocks * kThreads) {
    float n[3], m[3];
    const bool ok = finite_bits(__float_as_uint(A.d2[i])) &&
                    sample_normal(A.face, A.num, (int)i, A.normals, A.num_faces, n) &&
                    sample_normal(A.ref_face, A.num_ref, A.index[i], A.ref_normals, A.num_ref_faces, m);
    if (!ok) {
      p.skipped++;
      continue;
    }
    const float t = add_rn(add_rn(mul_rn(n[0], m[0]), mul_rn(n[1], m[1])), mul_rn(n[2], m[2]));
    p.sum += (double)fabsf(t);
    p.n++;
    if (t < 0.f) p.flipped++;
  }
  p = block_reduce(p, s_p);
  if (threadIdx.x == 0) out[blockIdx.x] = p;
}

__global__ __launch_bounds__(kThreads) void k_normal_finish(const NormalPartial* __restrict__ parts, double* __restrict__ record) {
  __shared__ NormalPartial s_p[kThreads / 64];
  for (int dir = 0; dir < 2; dir++) {
    NormalPartial p = parts[dir * kStatBlocks + threadIdx.x];        // kStatBlocks == kThreads
    __syncthreads();                                                 // the previous direction's readers of s_p are done
    p = block_reduce(p, s_p);
    if (threadIdx.x == 0) {
      record[4 * dir + 0] = (double)p.n;
      record[4 * dir + 1] = p.sum;
      record[4 * dir + 2] = (double)p.flipped;
      record[4 * dir + 3] = (double)p.skipped;
    }
  }
}

static_assert(kStatBlocks == kThreads, "k_normal_finish takes one partial per thread");

static int32_t normals_status(const mgs_mesh_normals_args* a, bool vertex) {
  if (!a || a->num_verts < 0 || a->num_faces < 0 || !a->record) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_faces > 0 && (!a->faces || (a->num_verts > 0 && !a->verts))) return MGS_ERR_BAD_ARGUMENT;
  if ((vertex ? a->num_verts : a->num_faces) > 0 && !a->normals) return MGS_ERR_BAD_ARGUMENT;
  if (vertex && !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > kMaxItems || a->num_faces > kMaxItems) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

}  // namespace mnorm
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_mesh_normals_args_size(void) { return (int32_t)sizeof(mgs_mesh_normals_args); }
int32_t mgs_mesh_eval_normal_args_size(void) { return (int32_t)sizeof(mgs_mesh_eval_normal_args); }

uint64_t mgs_vertex_normals_scratch_bytes(int32_t num_verts) {
  if (num_verts < 0 || num_verts > kMaxItems) return 0;
  return carved_bytes(mnorm::vertex_scratch, (size_t)num_verts);
}

uint64_t mgs_mesh_eval_normal_scratch_bytes(void) { return 2 * (uint64_t)mnorm::kStatBlocks * sizeof(mnorm::NormalPartial); }

int32_t mgs_face_normals(const mgs_mesh_normals_args* a, void* stream) {
  const int32_t rc = mnorm::normals_status(a, false);
  if (rc != MGS_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!hip_ok("memset(face normal record)", hipMemsetAsync(a->record, 0, sizeof(int32_t) * MGS_MESH_NORMAL_RECORD_INTS, st))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  if (a->num_faces > 0)
    launch("face_normals", mnorm::k_face_normals, dim3(grid_of(a->num_faces)), dim3(mnorm::kThreads), st, *a);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_vertex_normals(const mgs_mesh_normals_args* a, void* stream) {
  const int32_t rc = mnorm::normals_status(a, true);
  if (rc != MGS_OK) return rc;
  const int V = a->num_verts, F = a->num_faces;
  size_t bytes = 0;
  const mnorm::VertexScratch S = mnorm::vertex_scratch(a->scratch, (size_t)V, &bytes);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(mnorm::kThreads);
  if (!hip_ok("memset(vertex normal record)", hipMemsetAsync(a->record, 0, sizeof(int32_t) * MGS_MESH_NORMAL_RECORD_INTS, st)) ||
      !hip_ok("memset(vertex normal sums)", hipMemsetAsync(a->scratch, 0, bytes, st))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  if (F > 0) {
    launch("vn_max", mnorm::k_vn_max, dim3(grid_of(F)), th, st, *a, S);
    if (V > 0) launch("vn_add", mnorm::k_vn_add, dim3(grid_of(F)), th, st, *a, S);
  }
  if (V > 0) launch("vn_finish", mnorm::k_vn_finish, dim3(grid_of(V)), th, st, *a, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

static int32_t normal_eval_status(const mgs_mesh_eval_normal_args* a) {
  if (!a || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  return MGS_OK;
}

int32_t mgs_mesh_eval_normal_stats(const mgs_mesh_eval_normal_args* a, void* stream) {
  const int32_t rc = normal_eval_status(a);
  if (rc != MGS_OK) return rc;
  if (a->num < 0 || a->num_ref < 0 || a->num_faces < 0 || a->num_ref_faces < 0 || a->direction < 0 || a->direction > 1)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->num > 0 && (!a->d2 || !a->index || !a->face)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_ref > 0 && !a->ref_face) return MGS_ERR_BAD_ARGUMENT;
  if ((a->num_faces > 0 && !a->normals) || (a->num_ref_faces > 0 && !a->ref_normals)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num > kMaxItems || a->num_ref > kMaxItems || a->num_faces > kMaxItems || a->num_ref_faces > kMaxItems)
    return MGS_ERR_UNSUPPORTED;
  mnorm::NormalPartial* parts = static_cast<mnorm::NormalPartial*>(a->scratch) + a->direction * mnorm::kStatBlocks;
  launch("normal_stats", mnorm::k_normal_stats, dim3(mnorm::kStatBlocks), dim3(mnorm::kThreads), (hipStream_t)stream, *a, parts);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_eval_normal_finish(const mgs_mesh_eval_normal_args* a, void* stream) {
  const int32_t rc = normal_eval_status(a);
  if (rc != MGS_OK) return rc;
  if (!a->record) return MGS_ERR_BAD_ARGUMENT;
  launch("normal_finish", mnorm::k_normal_finish, dim3(1), dim3(mnorm::kThreads), (hipStream_t)stream,
         static_cast<const mnorm::NormalPartial*>(a->scratch), a->record);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
