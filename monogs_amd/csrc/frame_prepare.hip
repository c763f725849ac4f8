// Frame preparation on the device (mgs_frame_prepare; DESIGN.md "Frame preparation on the device"): what the reference
// does to every incoming frame before it is tracked - the dataset's uint8 / uint16 conversion (utils/dataset.py:269-276)
// and Camera.compute_grad_mask (utils/camera_utils.py:110-147, stencils utils/slam_utils.py:7-41).  Stream order:
//
//   global mode (every dataset type but Replica)
//     memset           the three radix histograms (20 KB)
//     k_fp_intensity   one 64x16 tile per workgroup: ingest, grey with a one-pixel reflect halo in LDS, the mapping
//                      mask, the gradient intensity I, level 1 of the select of I's lower median
//     k_fp_level<2,3>  levels 2 and 3 over the stored I
//     k_fp_threshold   the median m from the histograms, grad_mask = I > m * edge_threshold, rgb_pixel_mask
//   patch mode (Replica)
//     k_fp_patch       one 32x32 tile per workgroup: the same ingest and stencil, then - in a whole patch - the element
//                      of rank 511 of the tile's 1024 intensities by a three-level radix select in LDS, and the masks;
//                      a tile that is no whole patch (the fringe fold() leaves at 0) gets grad_mask = 0
//
//   remapped (mgs_frame_prepare_remapped): the same operations with k_fp_intensity<true> / k_fp_patch<true>, whose tile
//                      load gathers every pixel (halo included) bilinearly through a 1/32-pixel fixed-point map - the
//                      reference's cv2.remap undistortion (utils/dataset.py:226-244,264-265).  k_fp_remap_build makes
//                      that map once per calibration, in fp64.
//
// A latency problem (3.7 MB of float planes at 640x480): every launch is one resident round of workgroups.  Counting is
// integer, nothing is summed in floating point across threads: two calls give bit-identical outputs.  No host read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "radix_select.h"
#include "raster_kernels.h"
#include "remap_gather.h"
#include "rn_math.h"

namespace mgs {

namespace {

constexpr int kFpThreads = 256;
constexpr int kFpWaves = kFpThreads / 64;
constexpr int kFpTileW = 64, kFpTileH = 16;                      // global mode's tile: a wave per row
constexpr int kFpPatch = MGS_FRAME_PATCH_SIZE;                   // patch mode's tile IS the reference's patch
constexpr int kFpPatchRank = (kFpPatch * kFpPatch - 1) / 2;      // torch.median's element of 1024 values: rank 511
constexpr int kFpStep = kFpThreads * 4;                          // pixels per workgroup and step of the 1-D passes
constexpr int kFpMaxBlocks = 256;                                // workgroups of the 1-D passes
constexpr int kFpMaxTiles = 65535;                               // per side

struct FpScratch {
  RadixHists hist;
  float* intensity;   // [H*W] (intensity_out when the caller gave one)
};

struct FpLayout { uint64_t hists, zero_bytes, intensity, bytes; };

FpLayout fp_layout(uint64_t num_pixels) {
  FpLayout L;
  uint64_t o = 0;
  L.hists = o; o = align_up(o + (uint64_t)kRadixHistInts * 4);
  L.zero_bytes = o;
  L.intensity = o; o = align_up(o + num_pixels * 4);
  L.bytes = o;
  return L;
}

// torch's "reflect" padding of one pixel (-1 -> 1, n -> n - 2), then clamped: a tile's halo may hang over the image by
// more than that one pixel, and what it holds there is never read for a pixel inside the image.
__device__ __forceinline__ int reflect(int i, int n) {
  const int r = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return min(max(r, 0), n - 1);
}

// What a kernel takes: the frame's arguments and, in the remapped instantiation, the map's.  FpArgs<false> is laid out
// as mgs_frame_prepare_args itself.
template <bool REMAP>
struct FpArgs { mgs_frame_prepare_args a; };
template <>
struct FpArgs<true> { mgs_frame_prepare_args a; mgs_frame_remap_args r; };

constexpr int kFpMapClamp = 1 << 30;   // |ix|, |iy| <= 2^30: ix + 32 and ix + 16 stay inside int32

// (the taps and blends of the remap themselves: remap_gather.h)
__device__ __forceinline__ float blend_u8(const FpTaps& t, const uint8_t* u, int c, const float* s_lut) {
  return s_lut[blend_u8_int(t, u, c)];
}

__device__ __forceinline__ float convert_depth(const mgs_frame_prepare_args& A, size_t p) {
  return A.depth_format == MGS_FRAME_DEPTH_U16
             ? (float)((double)static_cast<const uint16_t*>(A.depth_in)[p] / A.depth_scale)
             : static_cast<const float*>(A.depth_in)[p];
}

// The (TW + 2) x (TH + 2) channel sums and greys around the tile at (x0, y0) into LDS; the pixels of the tile itself
// also get their converted image / depth written.  s_lut: k -> (float)(k / 255.0).  All threads call it.
// REMAP: every pixel, halo included, is gathered through the map at its reflected position.
template <int TW, int TH, bool REMAP>
__device__ void load_tile(const FpArgs<REMAP>& F, int x0, int y0, const float* s_lut, float* s_sum, float* s_grey) {
  constexpr int P = TW + 2;
  const mgs_frame_prepare_args& A = F.a;
  const int H = A.height, W = A.width;
  const size_t HW = (size_t)H * W;
  const bool u8 = A.image_format == MGS_FRAME_IMAGE_U8_HWC;
  const bool copy_image = REMAP || (A.image && (const void*)A.image != A.image_in);
  const bool copy_depth = A.depth_format != MGS_FRAME_DEPTH_NONE && A.gt_depth && (const void*)A.gt_depth != A.depth_in;
  bool nearest = false;
  if constexpr (REMAP) nearest = F.r.depth_mode == MGS_FRAME_REMAP_DEPTH_NEAREST;
  for (int t = threadIdx.x; t < P * (TH + 2); t += kFpThreads) {
    const int ty = t / P, tx = t - ty * P;
    const int y = y0 + ty - 1, x = x0 + tx - 1;
    const size_t p = (size_t)reflect(y, H) * W + reflect(x, W);
    float r, g, b;
    int2 q = make_int2(0, 0);                                      // REMAP: the pixel's map entry
    if constexpr (REMAP) {
      const FpTaps taps = remap_taps(F.r.map_q5, p, H, W);
      q = taps.q;
      if (u8) {
        const uint8_t* u = static_cast<const uint8_t*>(A.image_in);
        r = blend_u8(taps, u, 0, s_lut);
        g = blend_u8(taps, u, 1, s_lut);
        b = blend_u8(taps, u, 2, s_lut);
      } else {
        const float* f = static_cast<const float*>(A.image_in);
        r = blend_f32(taps, f);
        g = blend_f32(taps, f + HW);
        b = blend_f32(taps, f + 2 * HW);
      }
    } else if (u8) {
      const uint8_t* u = static_cast<const uint8_t*>(A.image_in) + 3 * p;
      r = s_lut[u[0]];
      g = s_lut[u[1]];
      b = s_lut[u[2]];
    } else {
      const float* f = static_cast<const float*>(A.image_in);
      r = f[p];
      g = f[HW + p];
      b = f[2 * HW + p];
    }
    const float s = add_rn(add_rn(r, g), b);
    s_sum[t] = s;
    s_grey[t] = s / 3.f;
    if (ty >= 1 && ty <= TH && tx >= 1 && tx <= TW && y < H && x < W) {   // the tile's own pixel: p is (y, x) itself
      if (copy_image) {
        A.image[p] = r;
        A.image[HW + p] = g;
        A.image[2 * HW + p] = b;
      }
      if (REMAP && nearest) {                                      // the nearest source pixel of the converted depth
        const int dx = (q.x + 16) >> 5, dy = (q.y + 16) >> 5;
        A.gt_depth[p] = dx >= 0 && dx < W && dy >= 0 && dy < H ? convert_depth(A, (size_t)dy * W + dx) : 0.f;
      } else if (copy_depth) {
        A.gt_depth[p] = convert_depth(A, p);
      }
    }
  }
}

// The gradient intensity of the tile's pixel (tx, ty) from the greys in LDS (pitch P, the pixel at (ty + 1, tx + 1)).
// Every product and sum is rounded on its own, in the order the torch mirror writes them (no fma): where the stencil
// cancels exactly there - flat and mirror-symmetric neighbourhoods - the intensity is exactly 0 here too.
template <int P>
__device__ __forceinline__ float tile_intensity(const float* s_grey, int tx, int ty) {
#pragma clang fp contract(off)
  const float* c = s_grey + ty * P + tx;
  const float a00 = c[0], a01 = c[1], a02 = c[2];
  const float a10 = c[P], a11 = c[P + 1], a12 = c[P + 2];
  const float a20 = c[2 * P], a21 = c[2 * P + 1], a22 = c[2 * P + 2];
  const bool valid = fabsf(a00) > 0.01f && fabsf(a01) > 0.01f && fabsf(a02) > 0.01f && fabsf(a10) > 0.01f &&
                     fabsf(a11) > 0.01f && fabsf(a12) > 0.01f && fabsf(a20) > 0.01f && fabsf(a21) > 0.01f &&
                     fabsf(a22) > 0.01f;
  const float gv = (3.f * a00 + 10.f * a01 + 3.f * a02 - 3.f * a20 - 10.f * a21 - 3.f * a22) * 0.03125f;
  const float gh = (3.f * a00 - 3.f * a02 + 10.f * a10 - 10.f * a12 + 3.f * a20 - 3.f * a22) * 0.03125f;
  return valid ? sqrtf(gv * gv + gh * gh) : 0.f;
}

__device__ __forceinline__ void fill_lut(float* s_lut) {
  static_assert(kFpThreads == 256, "one entry of the uint8 table per thread");
  s_lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
}

// ---- global mode ------------------------------------------------------------------------------------------------------
template <bool REMAP>
__global__ __launch_bounds__(kFpThreads) void k_fp_intensity(const FpArgs<REMAP> F, const FpScratch S) {
  constexpr int P = kFpTileW + 2;
  const mgs_frame_prepare_args& A = F.a;
  __shared__ float s_lut[256];
  __shared__ float s_sum[P * (kFpTileH + 2)];
  __shared__ float s_grey[P * (kFpTileH + 2)];
  __shared__ int s_hist[kRadixHist1];
  const int tid = threadIdx.x, H = A.height, W = A.width;
  fill_lut(s_lut);
  for (int b = tid; b < kRadixHist1; b += kFpThreads) s_hist[b] = 0;
  __syncthreads();
  const int x0 = blockIdx.x * kFpTileW, y0 = blockIdx.y * kFpTileH;
  load_tile<kFpTileW, kFpTileH, REMAP>(F, x0, y0, s_lut, s_sum, s_grey);
  __syncthreads();
  const int tx = tid & 63, x = x0 + tx;
#pragma unroll
  for (int j = 0; j < kFpTileH / kFpWaves; j++) {
    const int ty = j * kFpWaves + (tid >> 6), y = y0 + ty;
    const bool in = y < H && x < W;
    float I = 0.f;
    if (in) {
      const size_t p = (size_t)y * W + x;
      I = tile_intensity<P>(s_grey, tx, ty);
      S.intensity[p] = I;
      A.rgb_pixel_mask_mapping[p] = s_sum[(ty + 1) * P + tx + 1] > A.rgb_boundary_threshold ? 1.f : 0.f;
    }
    // I >= 0: the bit pattern orders like the value
    radix_hist_add_aggregated(s_hist, in, radix_level<1>(__float_as_uint(I), 0u).bucket);
  }
  __syncthreads();
  radix_hist_flush<kFpThreads>(s_hist, S.hist.h1, kRadixHist1);
}

template <int PASS>
__global__ __launch_bounds__(kFpThreads) void k_fp_level(const FpScratch S, int HW) {
  __shared__ int s_hist[kRadixHist1];
  __shared__ int s_scan[kFpWaves];
  __shared__ int s_sel[3];
  const int tid = threadIdx.x;
  constexpr int nb = radix_level_buckets(PASS);
  for (int b = tid; b < nb; b += kFpThreads) s_hist[b] = 0;
  // ends in a barrier: the histogram is clear before any wave adds to it
  const RadixSelected sel = radix_select<kFpThreads>(S.hist, PASS - 1, LowerMedianRank{}, s_scan, s_sel);
  for (int base = blockIdx.x * kFpStep; base < HW; base += gridDim.x * kFpStep) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = base + j * kFpThreads + tid;
      if (i >= HW) continue;
      const RadixBucket rb = radix_level<PASS>(__float_as_uint(S.intensity[i]), sel.prefix);
      if (rb.counts) atomicAdd(&s_hist[rb.bucket], 1);
    }
  }
  __syncthreads();
  radix_hist_flush<kFpThreads>(s_hist, S.hist.level(PASS), nb);
}

__global__ __launch_bounds__(kFpThreads) void k_fp_threshold(const mgs_frame_prepare_args A, const FpScratch S, int HW) {
  __shared__ int s_scan[kFpWaves];
  __shared__ int s_sel[3];
  const int tid = threadIdx.x;
  const RadixSelected sel = radix_select<kFpThreads>(S.hist, 3, LowerMedianRank{}, s_scan, s_sel);
  const float m = __uint_as_float(sel.prefix);
  const float thr = mul_rn(m, A.edge_threshold);
  if (blockIdx.x == 0 && tid == 0 && A.median_out) A.median_out[0] = m;
  for (int base = blockIdx.x * kFpStep; base < HW; base += gridDim.x * kFpStep) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = base + j * kFpThreads + tid;
      if (i >= HW) continue;
      const float gm = S.intensity[i] > thr ? 1.f : 0.f;
      A.grad_mask[i] = gm;
      A.rgb_pixel_mask[i] = A.rgb_pixel_mask_mapping[i] * gm;
    }
  }
}

// ---- patch mode -------------------------------------------------------------------------------------------------------
// One level of the in-LDS select of a patch's PER * kFpThreads intensities: histogram, then the whole workgroup searches
// it.  prefix and rank carry the selection from level to level.  All threads call it.
template <int LEVEL, int PER>
__device__ __forceinline__ void patch_select_level(const float (&I)[PER], int* s_hist, int* s_scan, int* s_sel,
                                                   unsigned& prefix, int& rank) {
  constexpr int nb = radix_level_buckets(LEVEL);
  for (int b = threadIdx.x; b < nb; b += kFpThreads) s_hist[b] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const RadixBucket rb = radix_level<LEVEL>(__float_as_uint(I[j]), prefix);
    if (rb.counts) atomicAdd(&s_hist[rb.bucket], 1);
  }
  __syncthreads();
  block_select<kFpThreads, nb / kFpThreads>(s_hist, rank, s_scan, s_sel);
  prefix = prefix << (LEVEL == 3 ? 10 : 11) | (unsigned)s_sel[0];
  rank = s_sel[1];
  __syncthreads();   // s_sel is read before the next level's search writes it
}

template <bool REMAP>
__global__ __launch_bounds__(kFpThreads) void k_fp_patch(const FpArgs<REMAP> F) {
  constexpr int P = kFpPatch + 2, PER = kFpPatch * kFpPatch / kFpThreads;
  const mgs_frame_prepare_args& A = F.a;
  __shared__ float s_lut[256];
  __shared__ float s_sum[P * P];
  __shared__ float s_grey[P * P];
  __shared__ int s_hist[kRadixHist1];
  __shared__ int s_scan[kFpWaves];
  __shared__ int s_sel[3];
  const int tid = threadIdx.x, H = A.height, W = A.width;
  fill_lut(s_lut);
  __syncthreads();
  const int x0 = blockIdx.x * kFpPatch, y0 = blockIdx.y * kFpPatch;
  load_tile<kFpPatch, kFpPatch, REMAP>(F, x0, y0, s_lut, s_sum, s_grey);
  __syncthreads();
  const bool whole = x0 + kFpPatch <= W && y0 + kFpPatch <= H;   // the same for the whole workgroup
  const int tx = tid & (kFpPatch - 1), x = x0 + tx;
  float I[PER];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int ty = j * (kFpThreads / kFpPatch) + tid / kFpPatch, y = y0 + ty;
    const bool in = y < H && x < W;
    I[j] = in ? tile_intensity<P>(s_grey, tx, ty) : 0.f;
    if (in) {
      const size_t p = (size_t)y * W + x;
      if (A.intensity_out) A.intensity_out[p] = I[j];
      A.rgb_pixel_mask_mapping[p] = s_sum[(ty + 1) * P + tx + 1] > A.rgb_boundary_threshold ? 1.f : 0.f;
      if (!whole) {       // what fold() leaves where no whole patch lies
        A.grad_mask[p] = 0.f;
        A.rgb_pixel_mask[p] = 0.f;
      }
    }
  }
  if (!whole) return;
  // rank 511 of the 1024 intensities: three histogram levels in LDS, each searched by the whole workgroup
  unsigned prefix = 0u;
  int rank = kFpPatchRank;
  patch_select_level<1>(I, s_hist, s_scan, s_sel, prefix, rank);
  patch_select_level<2>(I, s_hist, s_scan, s_sel, prefix, rank);
  patch_select_level<3>(I, s_hist, s_scan, s_sel, prefix, rank);
  const float m = __uint_as_float(prefix);
  const float thr = mul_rn(m, A.edge_threshold);
  if (tid == 0 && A.median_out) A.median_out[blockIdx.y * (W / kFpPatch) + blockIdx.x] = m;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int ty = j * (kFpThreads / kFpPatch) + tid / kFpPatch;
    const size_t p = (size_t)(y0 + ty) * W + x;
    const float gm = I[j] > thr ? 1.f : 0.f;
    A.grad_mask[p] = gm;
    A.rgb_pixel_mask[p] = s_sum[(ty + 1) * P + tx + 1] > A.rgb_boundary_threshold ? gm : 0.f;
  }
}

int32_t frame_prepare_args_status(const mgs_frame_prepare_args* a) {
  if (!a || a->width < 2 || a->height < 2) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode != MGS_FRAME_MODE_GLOBAL && a->mode != MGS_FRAME_MODE_PATCH) return MGS_ERR_BAD_ARGUMENT;
  if (a->mode == MGS_FRAME_MODE_PATCH && (a->width < kFpPatch || a->height < kFpPatch)) return MGS_ERR_BAD_ARGUMENT;
  if (a->image_format != MGS_FRAME_IMAGE_F32_CHW && a->image_format != MGS_FRAME_IMAGE_U8_HWC) return MGS_ERR_BAD_ARGUMENT;
  if (a->depth_format < MGS_FRAME_DEPTH_NONE || a->depth_format > MGS_FRAME_DEPTH_U16) return MGS_ERR_BAD_ARGUMENT;
  if (!a->image_in || !a->grad_mask || !a->rgb_pixel_mask || !a->rgb_pixel_mask_mapping || !a->scratch)
    return MGS_ERR_BAD_ARGUMENT;
  if (a->image_format == MGS_FRAME_IMAGE_U8_HWC && !a->image) return MGS_ERR_BAD_ARGUMENT;
  if (a->depth_format != MGS_FRAME_DEPTH_NONE && !a->depth_in) return MGS_ERR_BAD_ARGUMENT;
  if (a->depth_format == MGS_FRAME_DEPTH_U16 && (!a->gt_depth || !(a->depth_scale > 0.0))) return MGS_ERR_BAD_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(a->scratch) & 15u) return MGS_ERR_BAD_ARGUMENT;
  if ((int64_t)a->width * a->height > 0x7fffffff) return MGS_ERR_UNSUPPORTED;
  if ((a->width + kFpPatch - 1) / kFpPatch > kFpMaxTiles || (a->height + kFpTileH - 1) / kFpTileH > kFpMaxTiles)
    return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

int32_t frame_remap_args_status(const mgs_frame_prepare_args* a, const mgs_frame_remap_args* r) {
  if (!r || !r->map_q5 || (reinterpret_cast<uintptr_t>(r->map_q5) & 7u)) return MGS_ERR_BAD_ARGUMENT;
  if (r->depth_mode != MGS_FRAME_REMAP_DEPTH_NONE && r->depth_mode != MGS_FRAME_REMAP_DEPTH_NEAREST)
    return MGS_ERR_BAD_ARGUMENT;
  if (!a->image || (const void*)a->image == a->image_in) return MGS_ERR_BAD_ARGUMENT;    // a gather cannot run in place
  if (r->depth_mode == MGS_FRAME_REMAP_DEPTH_NEAREST &&
      (a->depth_format == MGS_FRAME_DEPTH_NONE || !a->gt_depth || (const void*)a->gt_depth == a->depth_in))
    return MGS_ERR_BAD_ARGUMENT;
  return MGS_OK;
}

template <bool REMAP>
int launch_frame_prepare(const FpArgs<REMAP>& F, hipStream_t st) {
  const mgs_frame_prepare_args& A = F.a;
  const int H = A.height, W = A.width, HW = H * W;
  const dim3 block(kFpThreads);
  if (A.mode == MGS_FRAME_MODE_PATCH) {
    launch("fp_patch", k_fp_patch<REMAP>, dim3((W + kFpPatch - 1) / kFpPatch, (H + kFpPatch - 1) / kFpPatch), block, st,
           F);
    return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
  }
  const FpLayout L = fp_layout((uint64_t)HW);
  char* w = static_cast<char*>(A.scratch);
  FpScratch S{};
  S.hist = radix_hists_at(w + L.hists);
  S.intensity = A.intensity_out ? A.intensity_out : reinterpret_cast<float*>(w + L.intensity);
  int hb = (HW + kFpStep - 1) / kFpStep;
  hb = hb > kFpMaxBlocks ? kFpMaxBlocks : hb;
  const dim3 tiles((W + kFpTileW - 1) / kFpTileW, (H + kFpTileH - 1) / kFpTileH), hgrid(hb);
  if (!hip_ok("frame prepare memset", hipMemsetAsync(w, 0, L.zero_bytes, st))) { launches_ok(); return MGS_ERR_LAUNCH; }
  launch("fp_intensity", k_fp_intensity<REMAP>, tiles, block, st, F, S);
  launch("fp_level2", k_fp_level<2>, hgrid, block, st, S, HW);
  launch("fp_level3", k_fp_level<3>, hgrid, block, st, S, HW);
  launch("fp_threshold", k_fp_threshold, hgrid, block, st, A, S, HW);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

// ---- the map ----------------------------------------------------------------------------------------------------------
// The header's "Map build", a thread per destination pixel, fp64 in the stated order and without contraction: the
// NumPy mirror (frame_prepare.remap_build_numpy) gives the same integers.
__global__ __launch_bounds__(kFpThreads) void k_fp_remap_build(const mgs_remap_build_args B) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kFpThreads + threadIdx.x;
  if (i >= (int64_t)B.width * B.height) return;
  const int vi = (int)(i / B.width), ui = (int)(i - (int64_t)vi * B.width);
  const double u = (double)ui, v = (double)vi;
  const double X = (B.ir[0] * u + B.ir[1] * v) + B.ir[2];
  const double Y = (B.ir[3] * u + B.ir[4] * v) + B.ir[5];
  const double Wd = (B.ir[6] * u + B.ir[7] * v) + B.ir[8];
  const double x = X / Wd, y = Y / Wd;
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, txy = (2.0 * x) * y;
  const double k1 = B.dist[0], k2 = B.dist[1], p1 = B.dist[2], p2 = B.dist[3], k3 = B.dist[4];
  const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double xd = (x * kr + p1 * txy) + p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * txy;
  const float mx = (float)(B.fx * xd + B.cx), my = (float)(B.fy * yd + B.cy);
  int ix = -kFpMapClamp, iy = -kFpMapClamp;
  if (isfinite(mx) && isfinite(my)) {
    const double lim = (double)kFpMapClamp;
    ix = (int)fmin(fmax(rint((double)mx * 32.0), -lim), lim);
    iy = (int)fmin(fmax(rint((double)my * 32.0), -lim), lim);
  }
  reinterpret_cast<int2*>(B.map_q5)[i] = make_int2(ix, iy);
}

}  // namespace

}  // namespace mgs

extern "C" {

int32_t mgs_frame_prepare_args_size(void) { return (int32_t)sizeof(mgs_frame_prepare_args); }

uint64_t mgs_frame_prepare_scratch_bytes(int32_t H, int32_t W) {
  if (H < 2 || W < 2 || (int64_t)H * W > 0x7fffffff) return 0;
  return mgs::fp_layout((uint64_t)H * (uint64_t)W).bytes;
}

int32_t mgs_frame_prepare(const mgs_frame_prepare_args* args, void* stream) {
  const int32_t rc = mgs::frame_prepare_args_status(args);
  if (rc != MGS_OK) return rc;
  return mgs::launch_frame_prepare(mgs::FpArgs<false>{*args}, (hipStream_t)stream);
}

int32_t mgs_remap_build_args_size(void) { return (int32_t)sizeof(mgs_remap_build_args); }
int32_t mgs_frame_remap_args_size(void) { return (int32_t)sizeof(mgs_frame_remap_args); }

int32_t mgs_remap_build(const mgs_remap_build_args* args, void* stream) {
  if (!args || args->width < 1 || args->height < 1) return MGS_ERR_BAD_ARGUMENT;
  if (!args->map_q5 || (reinterpret_cast<uintptr_t>(args->map_q5) & 7u)) return MGS_ERR_BAD_ARGUMENT;
  const int64_t HW = (int64_t)args->width * args->height;
  if (HW > 0x7fffffff) return MGS_ERR_UNSUPPORTED;
  mgs::launch("fp_remap_build", mgs::k_fp_remap_build, dim3((unsigned)((HW + mgs::kFpThreads - 1) / mgs::kFpThreads)),
              dim3(mgs::kFpThreads), (hipStream_t)stream, *args);
  return mgs::launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

int32_t mgs_frame_prepare_remapped(const mgs_frame_prepare_args* args, const mgs_frame_remap_args* remap, void* stream) {
  int32_t rc = mgs::frame_prepare_args_status(args);
  if (rc != MGS_OK) return rc;
  rc = mgs::frame_remap_args_status(args, remap);
  if (rc != MGS_OK) return rc;
  return mgs::launch_frame_prepare(mgs::FpArgs<true>{*args, *remap}, (hipStream_t)stream);
}

}  // extern "C"
