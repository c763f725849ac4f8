// Surface planes for mesh export and the viewer ("Surface planes").
//
//   k_surface_median   median depth: the view depth of the splat at which a pixel's transmittance falls through one
//                      half, found by a forward-only walk of the forward's sorted per-tile lists
//   k_depth_normal     camera-frame unit normals of any depth plane by central differences of the back-projected
//                      neighbours; every operation a single fp32 rounding (rn_math.h, __fdiv_rn, sqrtf), so the
//                      torch mirror (monogs_amd/surface.py: depth_normal_torch) gives the same bits
//
// Work-item shapes.  Median: the quadrant wave of k_view_first_hit (viewer.hip) - 64 lanes hold the 8x8 pixels of a
// quadrant, stage the reachable ones of 64 records at a time in LDS (2 KB per wave), walk them by ballot mask and
// leave at the first splat after which no lane is still open; the next chunk's records and the ids of the one after
// it are in flight during the walk, as in k_blend_fwd.  Normal: one thread per pixel, rows coalesced.
#include <hip/hip_runtime.h>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "raster_kernels.h"
#include "rn_math.h"

namespace mgs {

namespace sf {
constexpr int kThreads = 256;

__device__ __forceinline__ unsigned int load_id(const KP& P, const unsigned int* key_lo, int n, int k) {
  // low key word = Gaussian id (<< kPackBits | pair index when packed); past the list: 0, a valid record
  const unsigned int lo = k < n ? key_lo[2 * (size_t)k] : 0u;
  return P.pack ? lo >> kPackBits : lo;
}

// The blend's rules for a splat (power <= 0, alpha = min(0.99, o exp(power)) >= 1/255) and its transmittance
// T <- T (1 - alpha); the median splat is the first one after which T <= 0.5.  The walk needs no stop rule: the
// blend stops a pixel in front of the splat that would take T below 1e-4, but in front of the crossing T > 0.5 and
// alpha <= 0.99 leave T >= 0.005 behind it, so the blend's stop can never come before the crossing.
__global__ __launch_bounds__(64) void k_surface_median(KP P, float* __restrict__ median_depth,
                                                       int* __restrict__ median_index) {
  // per staged splat 32 B: (x, y, A, B) (C, opacity, depth, id)
  __shared__ float4 s_rec[kSeg * 2];
  const int item = xcd_remap<4>(blockIdx.x);
  if (item >= 4 * P.T) return;
  const int tile = item >> 2, quad = item & 3, lane = threadIdx.x;
  const int tx = tile % P.grid_x, ty = tile / P.grid_x;
  const int qx0 = tx * kTile + 8 * (quad & 1), qy0 = ty * kTile + 8 * (quad >> 1);
  if (qx0 >= P.W || qy0 >= P.H) return;
  const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
  const bool inside = px < P.W && py < P.H;
  const float fpx = (float)px, fpy = (float)py;
  int start = P.tile_offset[tile], end = P.tile_offset[tile + 1];
  start = min(start, P.cap); end = min(end, P.cap);
  const int n = end - start;
  const float bx0 = (float)qx0, by0 = (float)qy0;
  const float bx1 = fminf(bx0 + 7.f, (float)(P.W - 1)), by1 = fminf(by0 + 7.f, (float)(P.H - 1));
  bool open = inside;                     // T has not reached one half yet
  float T = 1.f, md = 0.f;
  int mi = -1;
  const unsigned int* key_lo = reinterpret_cast<const unsigned int*>(P.keys + start);
  // prologue: ids of chunks 0 and 1, records of chunk 0
  unsigned int id_n1 = load_id(P, key_lo, n, kSeg + lane);
  unsigned int cid = load_id(P, key_lo, n, lane);
  const float4* src0 = reinterpret_cast<const float4*>(P.rec + cid);
  float4 ca = src0[0], cb = src0[1];                            // (x, y, depth, o) (A, B, C, radius)
  for (int base = 0; base < n; base += kSeg) {
    // a counting splat has o exp(power) >= 1/255, i.e. the quadratic form below 2 ln(255 o): the blend's box test
    const bool reach = base + lane < n && box_reachable(ca.x, ca.y, cb.x, cb.y, cb.z, splat_qmax(ca.w), bx0, by0, bx1, by1);
    unsigned long long m = __builtin_amdgcn_ballot_w64(reach);
    // loads of the NEXT chunk (records) and of the one after it (ids)
    const unsigned int nid = id_n1;
    const float4* src1 = reinterpret_cast<const float4*>(P.rec + nid);
    const float4 na = src1[0], nb = src1[1];
    id_n1 = load_id(P, key_lo, n, base + 2 * kSeg + lane);
    if (m != 0ull) {
      __syncthreads();   // single-wave workgroup: orders the LDS traffic
      if (reach) {
        s_rec[2 * lane] = make_float4(ca.x, ca.y, cb.x, cb.y);
        s_rec[2 * lane + 1] = make_float4(cb.z, ca.w, ca.z, __int_as_float((int)cid));
      }
      __syncthreads();
      while (m != 0ull) {
        const int j = __builtin_ctzll(m);
        m &= m - 1ull;
        const float4 u = s_rec[2 * j], v = s_rec[2 * j + 1];
        const float dx = u.x - fpx, dy = u.y - fpy;
        const float power = -0.5f * (u.z * dx * dx + v.x * dy * dy) - u.w * dx * dy;
        const float a = fminf(kAlphaMax, v.y * __builtin_amdgcn_exp2f(power * 1.4426950408889634f));
        if (open && power <= 0.f && a >= kAlphaMin) {
          T = T * (1.f - a);
          if (T <= 0.5f) {
            md = v.z;
            mi = __float_as_int(v.w);
            open = false;
          }
        }
        if (__builtin_amdgcn_ballot_w64(open) == 0ull) break;   // every pixel of the quadrant has crossed
      }
    }
    if (__builtin_amdgcn_ballot_w64(open) == 0ull) break;
    cid = nid; ca = na; cb = nb;
  }
  if (inside) {
    const size_t pix = (size_t)py * P.W + px;
    median_depth[pix] = md;
    if (median_index) median_index[pix] = mi;
  }
}

__device__ __forceinline__ bool depth_valid(float d) { return d > 0.f && d < __builtin_inff(); }   // false for NaN

__global__ __launch_bounds__(kThreads) void k_depth_normal(mgs_depth_normal_args A) {
  const int HW = A.width * A.height;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= HW) return;
  const int y = pix / A.width, x = pix - y * A.width;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (x > 0 && x < A.width - 1 && y > 0 && y < A.height - 1) {
    const float dc = A.depth[pix], dl = A.depth[pix - 1], dr = A.depth[pix + 1];
    const float du = A.depth[pix - A.width], dd = A.depth[pix + A.width];
    bool ok = depth_valid(dc) && depth_valid(dl) && depth_valid(dr) && depth_valid(du) && depth_valid(dd);
    const float jump = mul_rn(A.max_jump, dc);
    ok = ok && fabsf(sub_rn(dl, dc)) <= jump && fabsf(sub_rn(dr, dc)) <= jump && fabsf(sub_rn(du, dc)) <= jump &&
         fabsf(sub_rn(dd, dc)) <= jump;
    if (ok) {
      // ray directions ((x + pixel_center - cx) / fx, (y + pixel_center - cy) / fy) of the column / row and its neighbours
      auto rx = [&](int xi) { return __fdiv_rn(sub_rn(add_rn((float)xi, A.pixel_center), A.cx), A.fx); };
      auto ry = [&](int yi) { return __fdiv_rn(sub_rn(add_rn((float)yi, A.pixel_center), A.cy), A.fy); };
      const float x0 = rx(x), y0 = ry(y);
      // a = P(x+1, y) - P(x-1, y), b = P(x, y+1) - P(x, y-1)
      const float ax = sub_rn(mul_rn(rx(x + 1), dr), mul_rn(rx(x - 1), dl));
      const float ay = sub_rn(mul_rn(y0, dr), mul_rn(y0, dl));
      const float az = sub_rn(dr, dl);
      const float bx = sub_rn(mul_rn(x0, dd), mul_rn(x0, du));
      const float by = sub_rn(mul_rn(ry(y + 1), dd), mul_rn(ry(y - 1), du));
      const float bz = sub_rn(dd, du);
      // n = b x a: a fronto-parallel plane gives n_z < 0, towards the camera
      const float cx_ = sub_rn(mul_rn(by, az), mul_rn(bz, ay));
      const float cy_ = sub_rn(mul_rn(bz, ax), mul_rn(bx, az));
      const float cz_ = sub_rn(mul_rn(bx, ay), mul_rn(by, ax));
      // sqrtf is the correctly rounded root (hipcc's default for fp32 sqrt and "/"); HIP's __fsqrt_rn is not - without
      // OCML_BASIC_ROUNDED_OPERATIONS it is the native instruction, an ulp off
      const float len = sqrtf(add_rn(add_rn(mul_rn(cx_, cx_), mul_rn(cy_, cy_)), mul_rn(cz_, cz_)));
      if (len > 0.f && len < __builtin_inff()) {
        nx = __fdiv_rn(cx_, len); ny = __fdiv_rn(cy_, len); nz = __fdiv_rn(cz_, len);
      }
    }
  }
  A.normal[pix] = nx; A.normal[(size_t)HW + pix] = ny; A.normal[2 * (size_t)HW + pix] = nz;
}
}  // namespace sf

int launch_surface_median(const KP& P, float* median_depth, int* median_index, hipStream_t st) {
  launch("surface_median", sf::k_surface_median, dim3(grid_pad(4 * P.T, 4)), dim3(64), st, P, median_depth, median_index);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_depth_normal_args_size(void) { return (int32_t)sizeof(mgs_depth_normal_args); }

int32_t mgs_depth_normal(const mgs_depth_normal_args* a, void* stream) {
  if (!a || a->width < 1 || a->height < 1 || !a->depth || !a->normal) return MGS_ERR_BAD_ARGUMENT;
  if (!(a->fx > 0.f) || !(a->fy > 0.f) || !(a->max_jump >= 0.f)) return MGS_ERR_BAD_ARGUMENT;
  if ((int64_t)a->width * a->height > 0x7fffffff - sf::kThreads) return MGS_ERR_UNSUPPORTED;
  const int HW = a->width * a->height;
  launch("depth_normal", sf::k_depth_normal, dim3((HW + sf::kThreads - 1) / sf::kThreads), dim3(sf::kThreads),
         (hipStream_t)stream, *a);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
