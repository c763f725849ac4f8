// Single roundings a torch mirror reproduces bit for bit (keyframe_seed.hip, frame_prepare.hip).  HIP's __fmul_rn /
// __fadd_rn are plain operators, which the default -ffp-contract=fast-honor-pragmas still fuses into an fma; the
// pragma takes the contract flag off these.
#pragma once
#include <hip/hip_runtime.h>

namespace mgs {

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// fp64 (mesh_render.hip): the same, against a NumPy float64 mirror
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double div_rn(double a, double b) {      // IEEE division: correctly rounded
#pragma clang fp contract(off)
  return a / b;
}

}  // namespace mgs
