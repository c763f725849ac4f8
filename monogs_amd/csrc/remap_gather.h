// The bilinear gather through a 1/32-pixel fixed-point map (include/monogs_raster.h "Remap"), shared by the tile load of
// mgs_frame_prepare_remapped and the rectification of mgs_stereo_depth.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgs {

// One destination pixel's four taps: offsets into an [H][W] plane, -1 for a tap outside the image - the bounds are
// checked before an address is formed - and the integer weights.
struct FpTaps {
  int2 q;                                                          // the map entry (ix, iy) itself
  int64_t o00, o01, o10, o11;
  int w00, w01, w10, w11;
};

__device__ __forceinline__ FpTaps remap_taps(const int32_t* map_q5, size_t p, int H, int W) {
  const int2 q = reinterpret_cast<const int2*>(map_q5)[p];        // (ix, iy): one 8-byte load
  const int sx = q.x >> 5, sy = q.y >> 5, ax = q.x & 31, ay = q.y & 31;
  const bool x0 = sx >= 0 && sx < W, x1 = sx >= -1 && sx < W - 1;
  const bool y0 = sy >= 0 && sy < H, y1 = sy >= -1 && sy < H - 1;
  FpTaps t;
  t.q = q;
  t.o00 = y0 && x0 ? (int64_t)sy * W + sx : -1;
  t.o01 = y0 && x1 ? (int64_t)sy * W + (sx + 1) : -1;
  t.o10 = y1 && x0 ? (int64_t)(sy + 1) * W + sx : -1;
  t.o11 = y1 && x1 ? (int64_t)(sy + 1) * W + (sx + 1) : -1;
  t.w00 = (32 - ax) * (32 - ay);
  t.w01 = ax * (32 - ay);
  t.w10 = (32 - ax) * ay;
  t.w11 = ax * ay;
  return t;
}

// channel c of a uint8 image with `stride` interleaved channels ([H][W][stride]); a tap outside reads 0
__device__ __forceinline__ int tap_u8(const uint8_t* u, int64_t o, int c, int stride = 3) {
  return o >= 0 ? (int)u[stride * o + c] : 0;
}
__device__ __forceinline__ float tap_f32(const float* f, int64_t o) { return o >= 0 ? f[o] : 0.f; }

// the uint8 blend: k = (w00*v00 + w01*v01 + w10*v10 + w11*v11 + 512) >> 10
__device__ __forceinline__ int blend_u8_int(const FpTaps& t, const uint8_t* u, int c, int stride = 3) {
  return (t.w00 * tap_u8(u, t.o00, c, stride) + t.w01 * tap_u8(u, t.o01, c, stride) +
          t.w10 * tap_u8(u, t.o10, c, stride) + t.w11 * tap_u8(u, t.o11, c, stride) + 512) >> 10;
}

__device__ __forceinline__ float blend_f32(const FpTaps& t, const float* f) {
#pragma clang fp contract(off)
  const float f00 = (float)t.w00 * 0.0009765625f, f01 = (float)t.w01 * 0.0009765625f;     // w / 1024: exact
  const float f10 = (float)t.w10 * 0.0009765625f, f11 = (float)t.w11 * 0.0009765625f;
  return (f00 * tap_f32(f, t.o00) + f01 * tap_f32(f, t.o01)) + (f10 * tap_f32(f, t.o10) + f11 * tap_f32(f, t.o11));
}

}  // namespace mgs
