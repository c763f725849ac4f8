// Ray cast of the TSDF volumes: depth, normal and colour of the fused surface at a pose, from the dense lattice of
// tsdf.hip or the brick pool of sparse_tsdf.hip (DESIGN.md "Ray cast of the volumes"; the contract is in
// include/monogs_raster.h, the mirror is monogs_amd/tsdf_raycast.py:raycast_torch).  Every pixel is independent and
// every operation of the contract is a single fp32 rounding (rn_math.h), so the device equals the mirror bit for bit.
//
//   k_raycast_neighbors  the [cap,27] table of brick ids (-1 absent) over the POOL: entries past 27 * state[0] leave at
//                        once, so the caller reads no brick count (k_sparse_integrate's trick)
//   k_raycast<Fetch>     ONE march over a point-fetch functor (DenseFetch, SparseFetch): a wave owns an 8 x 8 pixel
//                        tile, a workgroup 16 x 16.  The functor turns a lattice point into an index of the planes or -1.
//                        SparseFetch keeps the lane's last base brick (key -> id) and reaches the bricks of the other
//                        seven corners through the table.  With skip, samples PROVED invalid are passed over: the base
//                        point's brick is absent (crossed brick by brick, one map_find each), or the ray is outside the
//                        dense box.  The proof and its margin are in DESIGN.md.
//   k_raycast_shade      the ray cast's planes to a uint8 frame, one lane per pixel
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "rn_math.h"
#include "sparse_tsdf_map.h"

namespace mgs {
namespace raycast {

constexpr int kThreads = 256;
constexpr int kTile = 8;                  // a wave's tile edge; a workgroup of four waves covers 16 x 16 pixels
constexpr float kIndexLimit = 8388608.f;  // 2^23: |floor(l)| below it converts to int exactly

struct DenseFetch {
  int nx, ny, nz;
  __device__ __forceinline__ bool begin(const int*) { return true; }
  __device__ __forceinline__ long long index(const int b[3], int c) const {
    const int i = b[0] + (c & 1), j = b[1] + ((c >> 1) & 1), k = b[2] + (c >> 2);
    if (i < 0 || j < 0 || k < 0 || i >= nx || j >= ny || k >= nz) return -1;
    return ((long long)k * ny + j) * nx + i;
  }
  // a sample can be valid only while 0 <= l_a < hi(a)
  __device__ __forceinline__ float hi(int a) const { return (float)((a == 0 ? nx : a == 1 ? ny : nz) - 1); }
};

struct SparseFetch {
  const unsigned long long* keys;
  const int* vals;
  const int* nbr;
  unsigned mask;
  int cap;
  unsigned long long last_key;      // the lane's last base brick
  int last_id;
  // the base point b lies in a brick whose coordinates are in range: |b_a| < 2^23
  __device__ __forceinline__ bool begin(const int b[3]) {
    const unsigned long long key = sparse::key_of(b[0] >> 3, b[1] >> 3, b[2] >> 3);
    if (key != last_key) {
      const int id = sparse::map_find(keys, vals, mask, key);
      last_key = key;
      last_id = (unsigned)id < (unsigned)cap ? id : -1;
    }
    return last_id >= 0;
  }
  __device__ __forceinline__ long long index(const int b[3], int c) const {
    const int i = b[0] + (c & 1), j = b[1] + ((c >> 1) & 1), k = b[2] + (c >> 2);
    // the brick of the corner is the base brick or its neighbour one up: offsets 0 / 1 per axis
    const int q = 13 + ((i >> 3) - (b[0] >> 3)) + 3 * ((j >> 3) - (b[1] >> 3)) + 9 * ((k >> 3) - (b[2] >> 3));
    int id = last_id;
    if (q != 13) {
      id = nbr[27 * (size_t)last_id + q];
      if ((unsigned)id >= (unsigned)cap) return -1;      // absent, or not a brick id: a table the caller let go stale
    }
    return (long long)id * sparse::kBP + (((k & 7) * sparse::kB + (j & 7)) * sparse::kB + (i & 7));
  }
};

struct Planes {
  const float* tsdf;
  const float* weight;
  const float* color;        // may be null
  size_t plane;              // floats between two colour planes
  float origin[3];
  float vs;
};

// lerp(a, b, f) = a + f (b - a), along x, then y, then z, over the eight corner values v[c] (bit 0 of c is x)
__device__ __forceinline__ float trilerp(const float v[8], const float f[3]) {
  float x[4], y[2];
#pragma unroll
  for (int e = 0; e < 4; e++) x[e] = add_rn(v[2 * e], mul_rn(f[0], sub_rn(v[2 * e + 1], v[2 * e])));
#pragma unroll
  for (int e = 0; e < 2; e++) y[e] = add_rn(x[2 * e], mul_rn(f[1], sub_rn(x[2 * e + 1], x[2 * e])));
  return add_rn(y[0], mul_rn(f[2], sub_rn(y[1], y[0])));
}

// the eight corner indices and the fractions of the sample at l; false: the sample is invalid
template <class Fetch>
__device__ __forceinline__ bool corners(Fetch& F, const Planes& P, float min_weight, const float l[3], long long idx[8], float f[3]) {
  int b[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float bf = floorf(l[a]);
    if (!(fabsf(bf) < kIndexLimit)) return false;      // in float: a NaN or a huge value is no index
    b[a] = (int)bf;
    f[a] = sub_rn(l[a], bf);
  }
  if (!F.begin(b)) return false;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    idx[c] = F.index(b, c);
    if (idx[c] < 0) return false;
    if (!(P.weight[idx[c]] >= min_weight)) return false;
  }
  return true;
}

template <class Fetch>
__device__ __forceinline__ bool sample(Fetch& F, const Planes& P, float min_weight, const float l[3], float& value) {
  long long idx[8];
  float f[3], v[8];
  if (!corners(F, P, min_weight, l, idx, f)) return false;
#pragma unroll
  for (int c = 0; c < 8; c++) v[c] = P.tsdf[idx[c]];
  value = trilerp(v, f);
  return true;
}

struct Ray {
  float xn, yn;
  float R[3][3], t[3];       // T's rotation and translation
};

// the lattice coordinates of the ray's point at camera depth z: the allocation's expression
__device__ __forceinline__ void lattice_of(const Ray& r, const Planes& P, float z, float l[3]) {
  const float q[3] = {sub_rn(mul_rn(r.xn, z), r.t[0]), sub_rn(mul_rn(r.yn, z), r.t[1]), sub_rn(z, r.t[2])};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float p = add_rn(add_rn(mul_rn(r.R[0][a], q[0]), mul_rn(r.R[1][a], q[1])), mul_rn(r.R[2][a], q[2]));
    l[a] = __fdiv_rn(sub_rn(p, P.origin[a]), P.vs);
  }
}

// Not part of the contract (plain arithmetic): how many FURTHER steps j = 1 .. k keep l + j s inside [lo + eps, hi - eps],
// given the estimate s of the step; -1 when l itself is not inside.  The caller takes two off the result.
__device__ __forceinline__ float stay(float l, float s, float lo, float hi, float eps) {
  lo += eps;
  hi -= eps;
  if (!(l >= lo && l <= hi)) return -1.f;
  float k = 4.0e6f;
  if (s > 0.f) k = (hi - l) / s;
  if (s < 0.f) k = (lo - l) / s;
  return k >= 0.f ? fminf(k, 4.0e6f) : -1.f;      // a NaN gives -1
}

// the margin of axis a, in lattice units, against everything fp32 does to l_a along the ray
struct SkipModel {
  float s[3];                // lattice units per step
  float eps[3];
};

__device__ __forceinline__ SkipModel skip_model(const Ray& r, const Planes& P, const mgs_raycast_view& V) {
  SkipModel m;
  const float zmax = fabsf(V.z_near) + (float)V.num_steps * V.dz;
  const float qa[3] = {fabsf(r.xn) * zmax + fabsf(r.t[0]), fabsf(r.yn) * zmax + fabsf(r.t[1]), zmax + fabsf(r.t[2])};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    m.s[a] = (r.R[0][a] * r.xn + r.R[1][a] * r.yn + r.R[2][a]) * V.dz / P.vs;
    const float M = (fabsf(r.R[0][a]) * qa[0] + fabsf(r.R[1][a]) * qa[1] + fabsf(r.R[2][a]) * qa[2] + fabsf(P.origin[a])) / P.vs;
    m.eps[a] = M * (1.f / 131072.f) + (1.f / 256.f);      // 2^-17 M + 2^-8
  }
  return m;
}

// steps after n that are proved invalid: SparseFetch - the base point stays in the absent brick of l on every axis
__device__ __forceinline__ int proved_invalid(const SparseFetch& F, const SkipModel& m, const float l[3]) {
  if (F.last_id >= 0) return 0;
  float k = 4.0e6f;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float bf = floorf(l[a]);
    if (!(fabsf(bf) < kIndexLimit)) return 0;
    const float lo = (float)(((int)bf >> 3) << 3);        // the absent brick is the one begin() looked up for this l
    k = fminf(k, stay(l[a], m.s[a], lo, lo + 8.f, m.eps[a]));
  }
  return k >= 3.f ? (int)k - 2 : 0;
}

// DenseFetch - l stays below 0 or at or above n - 1 on ONE axis: some corner is outside the box
__device__ __forceinline__ int proved_invalid(const DenseFetch& F, const SkipModel& m, const float l[3]) {
  float k = -1.f;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    k = fmaxf(k, stay(l[a], m.s[a], -INFINITY, 0.f, m.eps[a]));        // l < 0: floor(l) <= -1
    k = fmaxf(k, stay(l[a], m.s[a], F.hi(a), INFINITY, m.eps[a]));     // floor(l) + 1 >= n
  }
  return k >= 3.f ? (int)k - 2 : 0;
}

template <class Fetch>
__global__ __launch_bounds__(kThreads) void k_raycast(Fetch F, Planes P, mgs_raycast_view V) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = (blockIdx.x * 2 + (wave & 1)) * kTile + (lane & 7), y = (blockIdx.y * 2 + (wave >> 1)) * kTile + (lane >> 3);
  if (x >= V.width || y >= V.height) return;
  Ray r;
  r.xn = __fdiv_rn(sub_rn((float)x, V.cx), V.fx);
  r.yn = __fdiv_rn(sub_rn((float)y, V.cy), V.fy);
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int c = 0; c < 3; c++) r.R[a][c] = V.T[4 * a + c];
    r.t[a] = V.T[4 * a + 3];
  }
  const SkipModel model = skip_model(r, P, V);
  const int N = V.num_steps;
  bool prev_ok = false;
  float prev = 0.f, cur = 0.f;
  int hit = -1, evaluated = 0;
  for (int n = 0; n < N; n++) {
    evaluated++;
    float l[3];
    lattice_of(r, P, add_rn(V.z_near, mul_rn((float)n, V.dz)), l);
    const bool ok = sample(F, P, V.min_weight, l, cur);
    if (ok && prev_ok) {
      if (prev > 0.f && cur <= 0.f) { hit = n; break; }
      if (prev < 0.f && cur > 0.f) { hit = -2; break; }
    }
    prev_ok = ok;
    prev = cur;
    if (!ok && V.skip) n += min(proved_invalid(F, model, l), N);      // the samples passed over are invalid: prev_ok stays false
  }
  const size_t pix = (size_t)y * V.width + x;
  float depth = 0.f, nrm[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
  if (hit >= 0) {
    const float t = __fdiv_rn(prev, sub_rn(prev, cur));
    depth = add_rn(add_rn(V.z_near, mul_rn((float)(hit - 1), V.dz)), mul_rn(t, V.dz));
    float l[3], f[3], v[8], g[3];
    long long idx[8];
    lattice_of(r, P, depth, l);
    bool ok = corners(F, P, V.min_weight, l, idx, f);
    if (ok && P.color) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
#pragma unroll
        for (int c = 0; c < 8; c++) v[c] = P.color[ch * P.plane + idx[c]];
        col[ch] = trilerp(v, f);
      }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      float lp[3] = {l[0], l[1], l[2]}, lm[3] = {l[0], l[1], l[2]}, vp = 0.f, vm = 0.f;
      lp[a] = add_rn(l[a], 1.f);
      lm[a] = sub_rn(l[a], 1.f);
      ok = ok && sample(F, P, V.min_weight, lp, vp);
      ok = ok && sample(F, P, V.min_weight, lm, vm);
      g[a] = sub_rn(vp, vm);
    }
    // sqrtf is the correctly rounded root (mesh_normals.hip)
    const float L = ok ? sqrtf(add_rn(add_rn(mul_rn(g[0], g[0]), mul_rn(g[1], g[1])), mul_rn(g[2], g[2]))) : 0.f;
    if (L > 0.f && L <= 3.4028234e38f) {
      float nw[3];
#pragma unroll
      for (int a = 0; a < 3; a++) nw[a] = __fdiv_rn(g[a], L);
#pragma unroll
      for (int a = 0; a < 3; a++)
        nrm[a] = V.frame == MGS_RAYCAST_FRAME_WORLD
                     ? nw[a]
                     : add_rn(add_rn(mul_rn(r.R[a][0], nw[0]), mul_rn(r.R[a][1], nw[1])), mul_rn(r.R[a][2], nw[2]));
    } else {
      col[0] = col[1] = col[2] = 0.f;
    }
  }
  V.depth[pix] = depth;
  V.hit_step[pix] = hit;
  if (V.evaluated) V.evaluated[pix] = evaluated;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    V.normal[3 * pix + a] = nrm[a];
    V.color[3 * pix + a] = col[a];
  }
}

__global__ __launch_bounds__(kThreads) void k_raycast_neighbors(mgs_sparse_tsdf_volume V, int* __restrict__ nbr, unsigned map_mask) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= 27ll * min(max(V.state[0], 0), V.max_bricks)) return;
  nbr[e] = sparse::neighbor_find(V, (int)e, map_mask);
}

// MGS_VIEW_RGB's quantisation (viewer.hip): fmaxf(NaN, 0) = 0, a NaN is black
__device__ __forceinline__ unsigned char quantise(float x) { return (unsigned char)(int)mul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.f); }

__global__ __launch_bounds__(kThreads) void k_raycast_shade(mgs_raycast_shade_args A, long long HW) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= HW) return;
  unsigned char rgb[3] = {A.background[0], A.background[1], A.background[2]};
  if (A.hit_step[i] >= 0) {
    if (A.mode == MGS_RAYCAST_SHADE_COLOR) {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) rgb[ch] = quantise(A.color[3 * i + ch]);
    } else if (A.mode == MGS_RAYCAST_SHADE_DEPTH) {
      const float t = __fdiv_rn(sub_rn(A.depth[i], A.depth_lo), sub_rn(A.depth_hi, A.depth_lo));
      rgb[0] = rgb[1] = rgb[2] = 0;
      if (t == t) {
        const int at = min(255, (int)mul_rn(fminf(fmaxf(t, 0.f), 1.f), 256.f));
#pragma unroll
        for (int ch = 0; ch < 3; ch++) rgb[ch] = A.lut[3 * at + ch];
      }
    } else {
      const float n[3] = {A.normal[3 * i], A.normal[3 * i + 1], A.normal[3 * i + 2]};
      if (A.mode == MGS_RAYCAST_SHADE_SHADED) {
        rgb[0] = rgb[1] = rgb[2] = quantise(add_rn(0.25f, mul_rn(0.75f, fabsf(n[2]))));
      } else {
        const float rx = __fdiv_rn(sub_rn((float)(i % A.width), A.cx), A.fx), ry = __fdiv_rn(sub_rn((float)(i / A.width), A.cy), A.fy);
        const bool away = add_rn(add_rn(mul_rn(n[0], rx), mul_rn(n[1], ry)), n[2]) > 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) rgb[ch] = quantise(add_rn(mul_rn(0.5f, away ? -n[ch] : n[ch]), 0.5f));
      }
    }
  }
  unsigned char* o = A.out + 3 * i;
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// ---- host checks -----------------------------------------------------------------------------------------------------
static int32_t view_status(const mgs_raycast_view& v) {
  if (v.width < 1 || v.height < 1 || !v.T || !v.depth || !v.normal || !v.color || !v.hit_step) return MGS_ERR_BAD_ARGUMENT;
  if (!(v.fx > 0.f) || !(v.fy > 0.f) || !(v.dz > 0.f) || !(v.z_near == v.z_near)) return MGS_ERR_BAD_ARGUMENT;
  if (v.frame < MGS_RAYCAST_FRAME_CAMERA || v.frame > MGS_RAYCAST_FRAME_WORLD || v.skip < 0 || v.skip > 1) return MGS_ERR_BAD_ARGUMENT;
  if (v.num_steps < 2) return MGS_ERR_BAD_ARGUMENT;
  if (v.num_steps > MGS_RAYCAST_MAX_STEPS) return MGS_ERR_UNSUPPORTED;
  if ((int64_t)v.width * v.height > 0x7fffffff / 3) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

static dim3 tile_grid(const mgs_raycast_view& v) {
  return dim3((unsigned)((v.width + 2 * kTile - 1) / (2 * kTile)), (unsigned)((v.height + 2 * kTile - 1) / (2 * kTile)));
}

}  // namespace raycast
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_tsdf_raycast_args_size(void) { return (int32_t)sizeof(mgs_tsdf_raycast_args); }
int32_t mgs_sparse_tsdf_raycast_args_size(void) { return (int32_t)sizeof(mgs_sparse_tsdf_raycast_args); }
int32_t mgs_raycast_shade_args_size(void) { return (int32_t)sizeof(mgs_raycast_shade_args); }

uint64_t mgs_sparse_tsdf_raycast_scratch_bytes(int32_t max_bricks) {
  return sparse::bricks_ok(max_bricks) ? 27ull * (uint64_t)max_bricks * sizeof(int) : 0;
}

int32_t mgs_tsdf_raycast(const mgs_tsdf_raycast_args* a, void* stream) {
  if (!a || a->nx < 1 || a->ny < 1 || a->nz < 1 || !a->tsdf || !a->weight || !(a->voxel_size > 0.f)) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rc = raycast::view_status(a->view);
  if (rc != MGS_OK) return rc;
  if ((int64_t)a->nx * a->ny * a->nz > 0x7fffffff) return MGS_ERR_UNSUPPORTED;
  raycast::DenseFetch F{a->nx, a->ny, a->nz};
  raycast::Planes P{a->tsdf, a->weight, a->color, (size_t)a->nx * a->ny * a->nz, {a->origin[0], a->origin[1], a->origin[2]},
                    a->voxel_size};
  launch("raycast_dense", raycast::k_raycast<raycast::DenseFetch>, raycast::tile_grid(a->view), dim3(raycast::kThreads),
         (hipStream_t)stream, F, P, a->view);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_sparse_tsdf_raycast(const mgs_sparse_tsdf_raycast_args* a, void* stream) {
  if (!a) return MGS_ERR_BAD_ARGUMENT;
  int32_t rc = sparse::volume_status(&a->vol);
  if (rc == MGS_ERR_BAD_ARGUMENT) return rc;
  if (!a->scratch || a->build_table < 0 || a->build_table > 1) return MGS_ERR_BAD_ARGUMENT;
  const int32_t rv = raycast::view_status(a->view);
  if (rv == MGS_ERR_BAD_ARGUMENT) return rv;
  if (rc != MGS_OK) return rc;
  if (rv != MGS_OK) return rv;
  const unsigned map_mask = sparse::map_mask_of(a->vol);
  int* nbr = static_cast<int*>(a->scratch);
  hipStream_t st = (hipStream_t)stream;
  if (a->build_table) {
    const long long entries = 27ll * a->vol.max_bricks;
    launch("raycast_neighbors", raycast::k_raycast_neighbors, dim3((unsigned)((entries + raycast::kThreads - 1) / raycast::kThreads)),
           dim3(raycast::kThreads), st, a->vol, nbr, map_mask);
  }
  raycast::SparseFetch F{reinterpret_cast<const unsigned long long*>(a->vol.map_keys), a->vol.map_vals, nbr, map_mask, a->vol.max_bricks, sparse::kNoKey, -1};
  raycast::Planes P{a->vol.tsdf, a->vol.weight, a->vol.color, (size_t)a->vol.max_bricks * sparse::kBP,
                    {a->vol.origin[0], a->vol.origin[1], a->vol.origin[2]}, a->vol.voxel_size};
  launch("raycast_sparse", raycast::k_raycast<raycast::SparseFetch>, raycast::tile_grid(a->view), dim3(raycast::kThreads), st, F, P,
         a->view);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_raycast_shade(const mgs_raycast_shade_args* a, void* stream) {
  if (!a || a->width < 1 || a->height < 1 || !a->hit_step || !a->out) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode < MGS_RAYCAST_SHADE_SHADED || a->mode > MGS_RAYCAST_SHADE_DEPTH) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode == MGS_RAYCAST_SHADE_COLOR ? !a->color : a->mode == MGS_RAYCAST_SHADE_DEPTH ? (!a->depth || !a->lut) : !a->normal)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->mode == MGS_RAYCAST_SHADE_NORMAL && (!(a->fx > 0.f) || !(a->fy > 0.f))) return MGS_ERR_BAD_ARGUMENT;
  const long long HW = (long long)a->width * a->height;
  if (HW > 0x7fffffff / 3) return MGS_ERR_UNSUPPORTED;
  launch("raycast_shade", raycast::k_raycast_shade, dim3((unsigned)((HW + raycast::kThreads - 1) / raycast::kThreads)),
         dim3(raycast::kThreads), (hipStream_t)stream, *a, HW);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
