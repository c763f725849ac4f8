// The fp32 pinhole projection of the TSDF fusion (tsdf.hip) and of the mesh renderer and the vertex visibility
// (mesh_render.hip): every product, sum and quotient is a single rounding (rn_math.h), in the order of
// tsdf.integrate_torch, so that the mirrors reproduce u, v, zc and the pixel bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "rn_math.h"

namespace mgs {

struct Pinhole {
  float r[3][4];                // rows 0-2 of T (world -> camera)
  float fx, fy, cx, cy, z_near;
};

__device__ __forceinline__ Pinhole pinhole_of(const float* __restrict__ T, float fx, float fy, float cx, float cy, float z_near) {
  Pinhole c;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 4; k++) c.r[r][k] = T[4 * r + k];
  c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.z_near = z_near;
  return c;
}

__device__ __forceinline__ float cam_row(const Pinhole& c, int r, float px, float py, float pz) {
  return add_rn(add_rn(add_rn(mul_rn(c.r[r][0], px), mul_rn(c.r[r][1], py)), mul_rn(c.r[r][2], pz)), c.r[r][3]);
}

// (u, v, zc) of the point (px, py, pz); false when !(zc > z_near)
__device__ __forceinline__ bool project(const Pinhole& c, float px, float py, float pz, float& u, float& v, float& zc) {
  const float xc = cam_row(c, 0, px, py, pz), yc = cam_row(c, 1, px, py, pz);
  zc = cam_row(c, 2, px, py, pz);
  if (!(zc > c.z_near)) return false;
  u = add_rn(mul_rn(c.fx, __fdiv_rn(xc, zc)), c.cx);
  v = add_rn(mul_rn(c.fy, __fdiv_rn(yc, zc)), c.cy);
  return true;
}

// the pixel (x, y) that (u, v) rounds to; false outside the image.  The range test is in float: a NaN or a huge
// coordinate never becomes an index.
__device__ __forceinline__ bool round_to_pixel(float u, float v, float width, float height, int& x, int& y) {
  const float uf = floorf(add_rn(u, 0.5f)), vf = floorf(add_rn(v, 0.5f));
  if (!(uf >= 0.f && uf < width && vf >= 0.f && vf < height)) return false;
  x = (int)uf; y = (int)vf;
  return true;
}

}  // namespace mgs
