// The stable compaction shared by mesh_clean.hip and mesh_render.hip: the scan of their uint4 block totals into bases and
// grand totals, the emit of vertices / colours / faces by in-block ranks and block bases, and the host checks in front
// of it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/monogs_raster.h"
#include "block_scan.h"
#include "launch.h"
#include "scratch_carve.h"

namespace mgs {

// x and y of the block totals become exclusive bases, z and w are summed.  counts (may be null): the totals of x, y, z,
// w.  (static: one copy per translation unit that includes it)
static __global__ __launch_bounds__(kCompactThreads) void k_compact_scan(uint4* __restrict__ base, int nblocks,
                                                                         int* __restrict__ counts) {
  __shared__ unsigned s_w[kCompactThreads / 64][2];
  unsigned cz = 0, cw = 0;
  const uint2 c = scan_block_totals(nblocks, s_w, [&](int b) { return base[b]; }, [&](int b, uint2 run, uint4 own) {
    base[b].x = run.x; base[b].y = run.y;
    cz += own.z; cw += own.w;
  });
  if (!counts) return;
  unsigned tz, tw;
  block_scan2(cz, cw, tz, tw, s_w);      // used as the block's sum of z and w
  if (threadIdx.x == 0) {
    counts[0] = (int)c.x; counts[1] = (int)c.y; counts[2] = (int)tz; counts[3] = (int)tw;
  }
}

// ---- emit: what mgs_mesh_clean_emit and mgs_mesh_cull_emit do after their counts were read -----------------------------
struct CompactEmit {
  int num_verts, num_faces, out_num_verts, out_num_faces;
  const float* verts;       // [V,3]
  const float* colors;      // [V,3] or null
  const int* faces;         // [F,3]
  float* out_verts;         // [out_num_verts,3]
  float* out_colors;        // [out_num_verts,3], with colors
  int* out_faces;           // [out_num_faces,3]
  const int* vrel;          // [V] in-block rank among the kept vertices, -1 when dropped
  const int* frel;          // [F] the same for faces
  const uint4* base;        // [blocks(max(V,F))] x: kept vertices, y: kept faces of the earlier blocks
};

// the emit fields of a public argument struct (mgs_mesh_clean_args, mgs_mesh_cull_args: the same names)
template <class A>
inline CompactEmit compact_emit_of(const A& a, const int* vrel, const int* frel, const uint4* base) {
  return CompactEmit{a.num_verts, a.num_faces, a.out_num_verts, a.out_num_faces, a.verts, a.colors, a.faces,
                     a.out_verts, a.out_colors, a.out_faces, vrel, frel, base};
}

// gathers vertices and colours, writes the re-indexed faces; every store bounded by the host's counts
static __global__ __launch_bounds__(kCompactThreads) void k_compact_emit(CompactEmit A) {
  const int i = blockIdx.x * kCompactThreads + threadIdx.x;
  const int V = A.num_verts, F = A.num_faces;
  if (i < V) {
    const int r = A.vrel[i];
    if (r >= 0) {
      const unsigned id = A.base[i / kCompactThreads].x + (unsigned)r;
      if (id < (unsigned)A.out_num_verts) {
#pragma unroll
        for (int ax = 0; ax < 3; ax++) A.out_verts[3 * (size_t)id + ax] = A.verts[3 * (size_t)i + ax];
        if (A.colors && A.out_colors) {
#pragma unroll
          for (int ch = 0; ch < 3; ch++) A.out_colors[3 * (size_t)id + ch] = A.colors[3 * (size_t)i + ch];
        }
      }
    }
  }
  if (i < F) {
    const int r = A.frel[i];
    if (r >= 0) {
      const unsigned fid = A.base[i / kCompactThreads].y + (unsigned)r;
      if (fid < (unsigned)A.out_num_faces) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
          const int v = A.faces[3 * (size_t)i + e];
          int id = -1;                                  // only if the faces changed since the count
          if ((unsigned)v < (unsigned)V) id = (int)A.base[v / kCompactThreads].x + A.vrel[v];
          A.out_faces[3 * (size_t)fid + e] = id;
        }
      }
    }
  }
}

// what every entry point of the clean-up and the cull checks first, on its own argument struct
template <class A>
inline int32_t mesh_sizes_status(const A* a) {
  if (!a || a->num_verts < 0 || a->num_faces < 0 || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_faces > 0 && !a->faces) return MGS_ERR_BAD_ARGUMENT;
  if (a->num_verts > kMaxItems || a->num_faces > kMaxItems) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

// the emit's argument checks and its launch under `name` (after mesh_sizes_status); nothing to emit: no launch
static int32_t compact_emit(const char* name, const CompactEmit& e, hipStream_t st) {
  if (e.out_num_verts < 0 || e.out_num_faces < 0) return MGS_ERR_BAD_ARGUMENT;
  if (e.out_num_verts > e.num_verts || e.out_num_faces > e.num_faces) return MGS_ERR_BAD_ARGUMENT;
  if (e.out_num_verts == 0 && e.out_num_faces == 0) return MGS_OK;
  if (e.out_num_verts > 0 && (!e.verts || !e.out_verts || (e.colors && !e.out_colors))) return MGS_ERR_BAD_ARGUMENT;
  if (e.out_num_faces > 0 && !e.out_faces) return MGS_ERR_BAD_ARGUMENT;
  const int items = e.num_verts > e.num_faces ? e.num_verts : e.num_faces;
  launch(name, k_compact_emit, dim3(grid_of(items)), dim3(kCompactThreads), st, e);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace mgs
