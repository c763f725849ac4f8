// Mesh rendering and culling: the depth image of a triangle mesh at a pose, the visibility of vertices against such an
// image, and the cull of what too few views saw (DESIGN.md "Mesh rendering and culling"; the mirrors in
// monogs_amd/mesh_render.py are the contract).
//
//   k_mr_fill      keys[pixel] = all ones; the record and the length of the large-face list cleared
//   k_mr_faces     one lane per face: indices, projection, snap, skip rules, doubled area, clamped box.  A box of at most
//                  `large_threshold` pixels is drawn by the lane; a larger one appends the face to the list
//   k_mr_large     a fixed grid strides the list (its length is read on the device): one workgroup per face, 256 threads
//                  striding the box.  The set-up is recomputed from the face index by the same function, the pixel by
//                  the same shade(): both paths write the same keys
//   k_mr_resolve   keys -> depth, face_id; record[2] = the length of the list
//   k_mesh_shade   one lane per pixel: face_id -> uint8 rgb (headlight, normal, interpolated vertex colour, background mask);
//                  the colour mode sets the face up again by the same setup_face and weighs by the same edge functions
//   k_vis          one thread per vertex: seen_count[v] += the view sees it
//   k_cull_init / k_cull_faces / k_cull_flags   the cull: face flags and vertex marks, their in-block ranks and block totals
//   k_compact_scan / k_compact_emit             the stable compaction (compact_scan.h)
//
// Exactness.  Coverage is integer: the snapped vertices lie within 2^24 of the origin in 1/256 pixel and a tested pixel
// lies inside the face's box, so every edge function is below 2^51 and converts to fp64 exactly.  Depth is a chain of
// single fp64 roundings (rn_math.h) and one conversion to fp32.  The winner of a pixel is the minimum of a 64-bit key
// under an integer atomic min: no float atomics, and the order in which faces arrive - including the order of the
// large-face list, which does depend on the execution - cannot show in the image.
//
// Visibility.  keys is only ever written by agent-scope atomics of k_mr_faces / k_mr_large (workgroups on every XCD) and
// read by k_mr_resolve after the launch boundary.  The atomic's old value is not used: no lane waits for it.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../../include/monogs_raster.h"
#include "compact_scan.h"
#include "launch.h"
#include "pinhole.h"
#include "rn_math.h"

namespace mgs {
namespace mrender {

constexpr int kThreads = 256;
static_assert(kThreads == kCompactThreads, "block_scan2 scans a workgroup of kCompactThreads");
constexpr long long kMaxPixels = (1ll << 31) - 1;
constexpr float kSnapLimit = 16777216.f;                  // 2^24, in 1/256 pixel
constexpr unsigned long long kEmptyKey = ~0ull;

// (u, v, zc) of vertex i (pinhole.h: the TSDF fusion's projection); false when !(zc > z_near)
__device__ __forceinline__ bool project_vertex(const float* __restrict__ verts, int i, const Pinhole& c, float& u, float& v, float& zc) {
  return project(c, verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2], u, v, zc);
}

// ---- render -----------------------------------------------------------------------------------------------------------
struct RenderScratch {
  unsigned long long* keys;   // [H W]
  int* list;                  // [F] faces of the large path, in arrival order
  int* num_large;             // [1]
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size (p may then be null)
static RenderScratch render_scratch(void* p, size_t HW, size_t F, size_t* bytes = nullptr) {
  Carver c(p);
  RenderScratch S;
  S.keys = c.take<unsigned long long>(HW);
  S.list = c.take<int>(F);
  S.num_large = c.take<int>();
  if (bytes) *bytes = c.bytes;
  return S;
}

enum { kFaceBad = 0, kFaceSkipped = 1, kFaceIgnored = 2, kFaceDrawn = 3 };

struct FaceSetup {
  long long x[3], y[3];       // snapped vertices, 1/256 pixel
  double iz[3];
  long long area2;            // |2A| > 0
  int sign;                   // of 2A
  int x0, y0, bw, bh;         // the clamped box; bw, bh >= 1 when drawn
};

__device__ __forceinline__ long long edge(long long ax, long long ay, long long bx, long long by, long long px, long long py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

__device__ __forceinline__ int setup_face(const mgs_mesh_render_args& A, const Pinhole& cam, int f, FaceSetup& S) {
  const int V = A.num_verts;
  int idx[3];
#pragma unroll
  for (int e = 0; e < 3; e++) idx[e] = A.faces[3 * (size_t)f + e];
  if (!((unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V)) return kFaceBad;
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 3; e++) {
    float u = 0.f, v = 0.f, zc = 0.f;
    bool good = project_vertex(A.verts, idx[e], cam, u, v, zc) && zc <= FLT_MAX;
    float xs = 0.f, ys = 0.f;
    if (good) {
      xs = rintf(mul_rn(u, 256.f));
      ys = rintf(mul_rn(v, 256.f));
      good = fabsf(xs) <= kSnapLimit && fabsf(ys) <= kSnapLimit;      // false for NaN
    }
    ok = ok && good;
    S.x[e] = good ? (long long)(int)xs : 0;
    S.y[e] = good ? (long long)(int)ys : 0;
    S.iz[e] = good ? div_rn(1.0, (double)zc) : 0.0;
  }
  if (!ok) return kFaceSkipped;
  const long long a2 = edge(S.x[0], S.y[0], S.x[1], S.y[1], S.x[2], S.y[2]);
  if (a2 == 0) return kFaceIgnored;
  S.sign = a2 > 0 ? 1 : -1;
  S.area2 = a2 > 0 ? a2 : -a2;
  const long long xmin = min(S.x[0], min(S.x[1], S.x[2])), xmax = max(S.x[0], max(S.x[1], S.x[2]));
  const long long ymin = min(S.y[0], min(S.y[1], S.y[2])), ymax = max(S.y[0], max(S.y[1], S.y[2]));
  // pixel centres 256 x inside [xmin, xmax]: x from ceil(xmin / 256) to floor(xmax / 256) (arithmetic shifts floor)
  const int x0 = (int)max((xmin + 255) >> 8, 0ll), x1 = (int)min(xmax >> 8, (long long)A.width - 1);
  const int y0 = (int)max((ymin + 255) >> 8, 0ll), y1 = (int)min(ymax >> 8, (long long)A.height - 1);
  S.x0 = x0; S.y0 = y0; S.bw = x1 - x0 + 1; S.bh = y1 - y0 + 1;
  return S.bw >= 1 && S.bh >= 1 ? kFaceDrawn : kFaceIgnored;
}

// the weight of vertex i at (X, Y), in 1/256 pixel: the edge function of the opposite edge, oriented by the area's sign
__device__ __forceinline__ long long weight(const FaceSetup& S, int i, long long X, long long Y) {
  const int a = (i + 1) % 3, b = (i + 2) % 3;
  return S.sign * edge(S.x[a], S.y[a], S.x[b], S.y[b], X, Y);
}

// pixel (px, py) of the face's clamped box: px in [0,W), py in [0,H) by construction
__device__ __forceinline__ void shade(const FaceSetup& S, int f, int px, int py, int W, unsigned long long* __restrict__ keys) {
  const long long X = 256ll * px, Y = 256ll * py;
  const long long w0 = weight(S, 0, X, Y), w1 = weight(S, 1, X, Y), w2 = weight(S, 2, X, Y);
  if (w0 < 0 || w1 < 0 || w2 < 0) return;
  const double den = add_rn(add_rn(mul_rn((double)w0, S.iz[0]), mul_rn((double)w1, S.iz[1])), mul_rn((double)w2, S.iz[2]));
  const float z = (float)div_rn((double)S.area2, den);
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)f;
  // the old value is not used: no lane waits for it.  (A relaxed load first, to skip the atomic when the key is already
  // smaller, made the lane wait every pixel: k_mr_faces 391 -> 98 us on the 11 910-face profile mesh without it.)
  __hip_atomic_fetch_min(keys + (size_t)py * W + px, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void k_mr_fill(RenderScratch S, long long HW, int* __restrict__ record) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < HW) S.keys[i] = kEmptyKey;
  if (i < MGS_MESH_RENDER_RECORD_INTS) record[i] = 0;
  if (i == 0) *S.num_large = 0;
}

__global__ __launch_bounds__(kThreads) void k_mr_faces(mgs_mesh_render_args A, RenderScratch S) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  const int F = A.num_faces;
  int status = kFaceIgnored;
  if (f < F) {
    const Pinhole cam = pinhole_of(A.T, A.fx, A.fy, A.cx, A.cy, A.z_near);
    FaceSetup P;
    status = setup_face(A, cam, f, P);
    if (status == kFaceDrawn) {
      const int npix = P.bw * P.bh;                       // <= H W < 2^31
      if (npix > A.large_threshold) {
        const int slot = atomicAdd(S.num_large, 1);       // one per face: slot < F
        if (slot < F) S.list[slot] = f;
      } else {
        for (int y = 0; y < P.bh; y++)
          for (int x = 0; x < P.bw; x++) shade(P, f, P.x0 + x, P.y0 + y, A.width, S.keys);
      }
    }
  }
  // integer counts, one add per wave
  const unsigned long long bad = __ballot(f < F && status == kFaceBad), skipped = __ballot(f < F && status == kFaceSkipped);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&A.record[0], __popcll(bad));
    if (skipped) atomicAdd(&A.record[1], __popcll(skipped));
  }
}

__global__ __launch_bounds__(kThreads) void k_mr_large(mgs_mesh_render_args A, RenderScratch S) {
  const int n = min(*S.num_large, A.num_faces);
  const Pinhole cam = pinhole_of(A.T, A.fx, A.fy, A.cx, A.cy, A.z_near);
  for (int i = blockIdx.x; i < n; i += gridDim.x) {       // uniform over the workgroup
    const int f = S.list[i];
    if ((unsigned)f >= (unsigned)A.num_faces) continue;
    FaceSetup P;
    if (setup_face(A, cam, f, P) != kFaceDrawn) continue;
    const int npix = P.bw * P.bh;
    for (int p = threadIdx.x; p < npix; p += kThreads) shade(P, f, P.x0 + p % P.bw, P.y0 + p / P.bw, A.width, S.keys);
  }
}

__global__ __launch_bounds__(kThreads) void k_mr_resolve(mgs_mesh_render_args A, RenderScratch S, long long HW) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < HW) {
    const unsigned long long key = S.keys[i];
    const bool hit = key != kEmptyKey;
    A.depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
    A.face_id[i] = hit ? (int)(unsigned)(key & 0xFFFFFFFFull) : -1;
  }
  if (i == 0) A.record[2] = min(*S.num_large, A.num_faces);
}

// ---- frames -----------------------------------------------------------------------------------------------------------
// MGS_VIEW_RGB's quantisation (viewer.hip): fmaxf(NaN, 0) = 0, a NaN is black
__device__ __forceinline__ unsigned char quantise(float x) { return (unsigned char)(int)mul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.f); }

// One lane per pixel: the colour of the face mgs_mesh_render left there (include/monogs_raster.h, mgs_mesh_shade).
__global__ __launch_bounds__(kThreads) void k_mesh_shade(mgs_mesh_shade_args A, long long HW) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= HW) return;
  const int f = A.face_id[i];
  unsigned char* o = A.out + 3 * (size_t)i;
  bool hit = (unsigned)f < (unsigned)A.num_faces;
  unsigned char rgb[3] = {A.background[0], A.background[1], A.background[2]};
  if (A.mode == MGS_MESH_SHADE_MASK) {
    if (hit) return;
  } else if (hit && A.mode == MGS_MESH_SHADE_COLOR) {
    mgs_mesh_render_args R{};
    R.num_verts = A.num_verts; R.num_faces = A.num_faces; R.width = A.width; R.height = A.height;
    R.verts = A.verts; R.faces = A.faces;
    const Pinhole cam = pinhole_of(A.T, A.fx, A.fy, A.cx, A.cy, A.z_near);
    FaceSetup P;
    if (setup_face(R, cam, f, P) == kFaceDrawn) {
      const long long X = 256ll * (i % A.width), Y = 256ll * (i / A.width);
      double t[3];
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = mul_rn((double)weight(P, k, X, Y), P.iz[k]);
      const double den = add_rn(add_rn(t[0], t[1]), t[2]);
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const size_t at = 3 * (size_t)A.faces[3 * (size_t)f + k] + ch;               // in [0,V): the face was set up
          c[k] = A.colors_u8 ? (double)__fdiv_rn((float)static_cast<const unsigned char*>(A.colors)[at], 255.f)
                             : (double)static_cast<const float*>(A.colors)[at];
        }
        const double num = add_rn(add_rn(mul_rn(t[0], c[0]), mul_rn(t[1], c[1])), mul_rn(t[2], c[2]));
        rgb[ch] = quantise((float)div_rn(num, den));
      }
    }
  } else if (hit) {
    const float nx = A.face_normal[3 * (size_t)f], ny = A.face_normal[3 * (size_t)f + 1], nz = A.face_normal[3 * (size_t)f + 2];
    float nc[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
      nc[r] = add_rn(add_rn(mul_rn(A.T[4 * r], nx), mul_rn(A.T[4 * r + 1], ny)), mul_rn(A.T[4 * r + 2], nz));
    if (A.mode == MGS_MESH_SHADE_SHADED) {
      rgb[0] = rgb[1] = rgb[2] = quantise(add_rn(0.25f, mul_rn(0.75f, fabsf(nc[2]))));
    } else {
      const float rx = __fdiv_rn(sub_rn((float)(i % A.width), A.cx), A.fx), ry = __fdiv_rn(sub_rn((float)(i / A.width), A.cy), A.fy);
      const bool away = add_rn(add_rn(mul_rn(nc[0], rx), mul_rn(nc[1], ry)), nc[2]) > 0.f;
#pragma unroll
      for (int ch = 0; ch < 3; ch++) rgb[ch] = quantise(add_rn(mul_rn(0.5f, away ? -nc[ch] : nc[ch]), 0.5f));
    }
  }
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// ---- visibility -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_vis(mgs_vertex_visibility_args A) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.num_verts) return;
  const Pinhole cam = pinhole_of(A.T, A.fx, A.fy, A.cx, A.cy, A.z_near);
  float u, v, zc;
  int x, y;
  if (!project_vertex(A.verts, i, cam, u, v, zc) || !round_to_pixel(u, v, (float)A.width, (float)A.height, x, y)) return;
  if (A.depth) {
    const float d = A.depth[(size_t)y * A.width + x];
    if (!(d > 0.f)) {
      if (!A.empty_visible) return;
    } else if (sub_rn(zc, d) > A.eps) {
      return;
    }
  }
  A.seen_count[i] += 1;
}

// ---- cull -------------------------------------------------------------------------------------------------------------
struct CullScratch {
  int* vrel;        // [V] mark of a named vertex, then its in-block rank among the kept, -1 when dropped
  int* frel;        // [F] 1 kept / 0 dropped / -1 bad, then the same rank for faces
  uint4* base;      // [blocks(max(V,F))] x: kept vertices, y: kept faces of the earlier blocks, z: bad faces
};

// the planes of the scratch buffer at p, in their order; *bytes (if given): their size, never 0 (p may then be null)
static CullScratch cull_scratch(void* p, size_t V, size_t F, size_t* bytes = nullptr) {
  Carver c(p);
  CullScratch S;
  S.vrel = c.take<int>(V);
  S.frel = c.take<int>(F);
  S.base = c.take<uint4>((size_t)grid_of((long long)(V > F ? V : F)));
  if (bytes) *bytes = c.bytes > 0 ? c.bytes : 256;
  return S;
}

__global__ __launch_bounds__(kThreads) void k_cull_init(CullScratch S, int V) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < V) S.vrel[i] = 0;
}

__global__ __launch_bounds__(kThreads) void k_cull_faces(mgs_mesh_cull_args A, CullScratch S) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.num_faces) return;
  const int V = A.num_verts;
  const int a = A.faces[3 * (size_t)i], b = A.faces[3 * (size_t)i + 1], c = A.faces[3 * (size_t)i + 2];
  if (!((unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V)) {
    S.frel[i] = -1;
    return;
  }
  const bool sa = A.seen_count[a] >= A.min_views, sb = A.seen_count[b] >= A.min_views, sc = A.seen_count[c] >= A.min_views;
  const bool keep = A.rule ? (sa || sb || sc) : (sa && sb && sc);
  S.frel[i] = keep ? 1 : 0;
  if (keep) S.vrel[a] = S.vrel[b] = S.vrel[c] = 1;      // every writer stores the same 1
}

__global__ __launch_bounds__(kThreads) void k_cull_flags(CullScratch S, int V, int F) {
  __shared__ unsigned s_w[kThreads / 64][2];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool kv = i < V && S.vrel[i] == 1;
  const int ff = i < F ? S.frel[i] : 0;
  const bool kf = ff == 1;
  const unsigned bad = (unsigned)__syncthreads_count(ff == -1);
  unsigned v = kv ? 1u : 0u, f = kf ? 1u : 0u, tv, tf;
  block_scan2(v, f, tv, tf, s_w);
  if (i < V) S.vrel[i] = kv ? (int)v : -1;
  if (i < F) S.frel[i] = kf ? (int)f : -1;
  if (threadIdx.x == 0) S.base[blockIdx.x] = make_uint4(tv, tf, bad, 0u);
}

static bool camera_ok(float fx, float fy, float cx, float cy, float z_near) {
  return fx == fx && fy == fy && cx == cx && cy == cy && z_near == z_near;
}

}  // namespace mrender
}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_mesh_render_args_size(void) { return (int32_t)sizeof(mgs_mesh_render_args); }
int32_t mgs_vertex_visibility_args_size(void) { return (int32_t)sizeof(mgs_vertex_visibility_args); }
int32_t mgs_mesh_cull_args_size(void) { return (int32_t)sizeof(mgs_mesh_cull_args); }
int32_t mgs_mesh_shade_args_size(void) { return (int32_t)sizeof(mgs_mesh_shade_args); }

uint64_t mgs_mesh_render_scratch_bytes(int32_t height, int32_t width, int32_t num_faces) {
  if (height < 1 || width < 1 || num_faces < 0 || num_faces > kMaxItems) return 0;
  if ((long long)height * width > mrender::kMaxPixels) return 0;
  return carved_bytes(mrender::render_scratch, (size_t)height * (size_t)width, (size_t)num_faces);
}

int32_t mgs_mesh_render(const mgs_mesh_render_args* a, void* stream) {
  if (!a || a->num_verts < 0 || a->num_faces < 0 || a->width < 1 || a->height < 1 || a->large_grid < 0)
    return MGS_ERR_BAD_ARGUMENT;
  if (!a->T || !a->scratch || !a->depth || !a->face_id || !a->record) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_faces > 0 && (!a->faces || (a->num_verts > 0 && !a->verts))) return MGS_ERR_BAD_ARGUMENT;
  if (!mrender::camera_ok(a->fx, a->fy, a->cx, a->cy, a->z_near)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > kMaxItems || a->num_faces > kMaxItems) return MGS_ERR_UNSUPPORTED;
  const long long HW = (long long)a->height * a->width;
  if (HW > mrender::kMaxPixels) return MGS_ERR_UNSUPPORTED;
  mgs_mesh_render_args A = *a;
  if (A.large_threshold < 0) A.large_threshold = MGS_MESH_RENDER_LARGE_BOX;
  if (A.large_grid == 0) A.large_grid = MGS_MESH_RENDER_LARGE_GRID;
  const mrender::RenderScratch S = mrender::render_scratch(A.scratch, (size_t)HW, (size_t)A.num_faces);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(mrender::kThreads);
  launch("mr_fill", mrender::k_mr_fill, dim3(grid_of(HW)), th, st, S, HW, A.record);
  if (A.num_faces > 0) {
    launch("mr_faces", mrender::k_mr_faces, dim3(grid_of(A.num_faces)), th, st, A, S);
    launch("mr_large", mrender::k_mr_large, dim3(A.large_grid), th, st, A, S);
  }
  launch("mr_resolve", mrender::k_mr_resolve, dim3(grid_of(HW)), th, st, A, S, HW);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_shade(const mgs_mesh_shade_args* a, void* stream) {
  if (!a || a->num_verts < 0 || a->num_faces < 0 || a->width < 1 || a->height < 1 || !a->face_id || !a->out)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->mode < MGS_MESH_SHADE_SHADED || a->mode > MGS_MESH_SHADE_MASK) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode != MGS_MESH_SHADE_MASK && a->num_faces > 0) {
    if (!a->T || !mrender::camera_ok(a->fx, a->fy, a->cx, a->cy, a->z_near)) return MGS_ERR_BAD_ARGUMENT;
    if (a->mode == MGS_MESH_SHADE_COLOR ? (!a->faces || !a->colors || !a->verts || a->num_verts < 1) : !a->face_normal)
      return MGS_ERR_BAD_ARGUMENT;
  }
  if (a->num_verts > kMaxItems || a->num_faces > kMaxItems) return MGS_ERR_UNSUPPORTED;
  const long long HW = (long long)a->height * a->width;
  if (3 * HW > mrender::kMaxPixels) return MGS_ERR_UNSUPPORTED;
  launch("mesh_shade", mrender::k_mesh_shade, dim3(grid_of(HW)), dim3(mrender::kThreads), (hipStream_t)stream, *a, HW);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_vertex_visibility(const mgs_vertex_visibility_args* a, void* stream) {
  if (!a || a->num_verts < 0 || a->width < 1 || a->height < 1 || !a->T) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > 0 && (!a->verts || !a->seen_count)) return MGS_ERR_BAD_ARGUMENT;
  if (!mrender::camera_ok(a->fx, a->fy, a->cx, a->cy, a->z_near) || a->eps != a->eps) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > kMaxItems || (long long)a->height * a->width > mrender::kMaxPixels) return MGS_ERR_UNSUPPORTED;
  if (a->num_verts == 0) return MGS_OK;
  launch("mesh_vis", mrender::k_vis, dim3(grid_of(a->num_verts)), dim3(mrender::kThreads), (hipStream_t)stream, *a);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

uint64_t mgs_mesh_cull_scratch_bytes(int32_t num_verts, int32_t num_faces) {
  if (num_verts < 0 || num_faces < 0 || num_verts > kMaxItems || num_faces > kMaxItems) return 0;
  return carved_bytes(mrender::cull_scratch, (size_t)num_verts, (size_t)num_faces);
}

int32_t mgs_mesh_cull_count(const mgs_mesh_cull_args* a, void* stream) {
  const int32_t rc = mesh_sizes_status(a);
  if (rc != MGS_OK) return rc;
  if (!a->counts || (a->rule != 0 && a->rule != 1)) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > 0 && a->num_faces > 0 && !a->seen_count) return MGS_ERR_BAD_ARGUMENT;
  const int V = a->num_verts, F = a->num_faces;
  const mrender::CullScratch S = mrender::cull_scratch(a->scratch, (size_t)V, (size_t)F);
  hipStream_t st = (hipStream_t)stream;
  const dim3 th(mrender::kThreads);
  const int blocks = grid_of(V > F ? V : F);
  if (V > 0) launch("cull_init", mrender::k_cull_init, dim3(grid_of(V)), th, st, S, V);
  if (F > 0) launch("cull_faces", mrender::k_cull_faces, dim3(grid_of(F)), th, st, *a, S);
  if (blocks > 0) launch("cull_flags", mrender::k_cull_flags, dim3(blocks), th, st, S, V, F);
  launch("cull_scan", k_compact_scan, dim3(1), th, st, S.base, blocks, a->counts);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_mesh_cull_emit(const mgs_mesh_cull_args* a, void* stream) {
  const int32_t rc = mesh_sizes_status(a);
  if (rc != MGS_OK) return rc;
  const mrender::CullScratch S = mrender::cull_scratch(a->scratch, (size_t)a->num_verts, (size_t)a->num_faces);
  return compact_emit("cull_emit", compact_emit_of(*a, S.vrel, S.frel, S.base), (hipStream_t)stream);
}

}  // extern "C"
