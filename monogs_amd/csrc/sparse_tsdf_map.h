// The brick lattice of the sparse TSDF volume and its persistent map, shared by sparse_tsdf.hip (allocation, integration,
// extraction) and tsdf_raycast.hip (the ray cast): the constants, the brick keys, the read side of the map, the lookup of
// a brick's 27 neighbours and the host checks of a volume (DESIGN.md "Sparse TSDF volume").
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/monogs_raster.h"
#include "min_index_set.h"
#include "rn_math.h"

namespace mgs {
namespace sparse {

constexpr int kThreads = 256;
constexpr int kB = 8, kBP = kB * kB * kB;                  // brick edge, points of a brick
constexpr int kBias = 1 << 20;                             // brick coordinates lie in [-kBias, kBias)
constexpr int kMaxBricks = (int)(((1ll << 31) - 1) / (7 * kBP));      // 7 * 512 * bricks < 2^31: 599186
constexpr unsigned long long kNoKey = ~0ull;               // no brick key has bit 63

__device__ __forceinline__ float lattice(float o, int i, float vs) { return add_rn(o, mul_rn((float)i, vs)); }

// ---- brick keys and the persistent map -------------------------------------------------------------------------------
__host__ __device__ __forceinline__ bool coord_ok(int b) { return b >= -kBias && b < kBias; }
__host__ __device__ __forceinline__ unsigned long long key_of(int bx, int by, int bz) {
  return (unsigned long long)(bx + kBias) | (unsigned long long)(by + kBias) << 21 | (unsigned long long)(bz + kBias) << 42;
}
__device__ __forceinline__ void coords_of(unsigned long long key, int b[3]) {
#pragma unroll
  for (int a = 0; a < 3; a++) b[a] = (int)((key >> (21 * a)) & 0x1FFFFFull) - kBias;
}

// the key plane in the type of the 64-bit atomics
__device__ __forceinline__ unsigned long long* keys_of(const mgs_sparse_tsdf_volume& v) {
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "brick keys are 64-bit");
  return reinterpret_cast<unsigned long long*>(v.map_keys);
}

// the id of `key`, -1 when the map does not hold it; plain loads: the map was written by an earlier launch
__device__ __forceinline__ int map_find(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, unsigned mask,
                                        unsigned long long key) {
  unsigned slot = (unsigned)mix64(key) & mask;
  for (unsigned probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
    const unsigned long long cur = keys[slot];
    if (cur == kNoKey) return -1;
    if (cur == key) return vals[slot];
  }
  return -1;
}

// entry e = 27 * brick + q of the neighbour table: the id of the brick at offset q = (dx + 1) + 3 (dy + 1) + 9 (dz + 1)
// from `brick`, -1 when the map does not hold it or its coordinates leave the range
__device__ __forceinline__ int neighbor_find(const mgs_sparse_tsdf_volume& V, int e, unsigned map_mask) {
  const int brick = e / 27, q = e - 27 * brick;
  const int bx = V.brick_coords[3 * brick] + q % 3 - 1, by = V.brick_coords[3 * brick + 1] + (q / 3) % 3 - 1,
            bz = V.brick_coords[3 * brick + 2] + q / 9 - 1;
  int id = -1;
  if (coord_ok(bx) && coord_ok(by) && coord_ok(bz)) id = map_find(keys_of(V), V.map_vals, map_mask, key_of(bx, by, bz));
  return id;
}

// ---- host checks -----------------------------------------------------------------------------------------------------
static inline bool bricks_ok(int n) { return n >= 1 && n <= kMaxBricks; }

static inline int32_t volume_status(const mgs_sparse_tsdf_volume* v) {
  if (!v || v->max_bricks < 1) return MGS_ERR_BAD_ARGUMENT;
  if (!v->tsdf || !v->weight || !v->brick_coords || !v->map_keys || !v->map_vals || !v->state) return MGS_ERR_BAD_ARGUMENT;
  if (!(v->voxel_size > 0.f)) return MGS_ERR_BAD_ARGUMENT;
  if (v->max_bricks > kMaxBricks) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

static inline unsigned map_mask_of(const mgs_sparse_tsdf_volume& v) { return (unsigned)(set_table_size((unsigned long long)v.max_bricks) - 1); }

}  // namespace sparse
}  // namespace mgs
