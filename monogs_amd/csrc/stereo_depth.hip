// Stereo depth on the device (mgs_stereo_depth; DESIGN.md "Stereo depth on the device"): what the reference's
// StereoDataset.__getitem__ does to every frame on the host (utils/dataset.py:367-395) - rectify both images, semi-global
// block matching over 64 disparities, depth = bf / disparity.  The contract is the header's ("stereo depth") and
// stereo_depth.stereo_sgbm_numpy's; every step is integer arithmetic, so kernels and mirror agree bit for bit.
// Stream order (Wv = W - 64 valid columns; lane = disparity wherever a wave works on one pixel):
//
//   k_sd_grey       both images, a thread per pixel: the optional bilinear gather through a 1/32-pixel map (the taps of
//                   mgs_frame_prepare_remapped), the reduction to grey u8, the left image's float [3][H][W]
//   k_sd_pack       both images, a thread per pixel: the clipped Sobel response g and, for g and the grey, the
//                   Birchfield-Tomasi bounds - six bytes in one 8-byte word, so a pixel cost is two loads
//   k_sd_hsum       a wave per row and 64-column segment: the pixel cost summed over |dx| <= r as a running sum along
//                   the row (21 costs to start a segment, two per further column), u16 [H][Wv][64]
//   k_sd_vsum       a thread per column, 32-row segment and four disparities: the running sum over |dy| <= r of the
//                   above, packed 16-bit adds: the block cost C, u16 [H][Wv][64] - one 128-byte line per pixel
//   memset          votes = all ones
//   k_sd_aggregate  a wave per path, every path of the five directions in one launch: the recurrence needs the lane's
//                   two neighbours (DPP wave shifts) and the wave minimum (DPP row reduction, four lane reads); the
//                   next pixel's C is loaded before the dependent chain of the current one; each direction stores its
//                   L in a u16 volume of its own (plain 128-byte stores: summing into one S by atomic adds ran at the
//                   chip's atomic rate, 304 us at 752x480)
//   k_sd_select     a wave per pixel: S = the five L, argmin by a wave minimum of (S << 6 | d), uniqueness by ballot,
//                   sub-pixel, the vote for the left-right check by atomicMin
//   k_sd_finish     a thread per pixel: the left-right check and the double-precision depth
//
// No host read, no synchronisation; integer sums only: two calls give identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/monogs_raster.h"
#include "launch.h"
#include "raster_kernels.h"
#include "remap_gather.h"

namespace mgs {

namespace {

constexpr int kSdD = MGS_STEREO_DISPARITIES;     // one wave64 holds one pixel's disparity axis
constexpr int kSdP1 = 2, kSdP2 = 5;              // OpenCV's substitutes for StereoSGBM_create's P1 = P2 = 0
constexpr int kSdFt = 15;                        // preFilterCap (ftzero)
constexpr int kSdThreads = 256;
constexpr int kSdWaves = kSdThreads / 64;
constexpr int kSdSegX = 64;                      // columns per wave of k_sd_hsum
constexpr int kSdSegY = 32;                      // rows per thread of k_sd_vsum
constexpr int kSdMaxSide = 16384;
constexpr int kSdMaxHalfBlock = 14;              // (2r+1)^2 * 70 must fit 16 bits
constexpr int kSdBig = 1 << 28;                  // the neighbour of d = 0 / d = 63 that is left out
constexpr unsigned kSdNoVote = 0xffffffffu;
static_assert(kSdD == 64, "lane = disparity");
static_assert((2 * kSdMaxHalfBlock + 1) * (2 * kSdMaxHalfBlock + 1) * 70 + kSdP2 <= 65535, "C and L are stored in 16 bits");

constexpr int kSdPaths = 5;

struct SdLayout { uint64_t grey, pack, C, L, vote, disp, bytes; };

// hs (the row sums) lives in the first direction's L volume: it is dead before the aggregation writes there.
SdLayout sd_layout(uint64_t H, uint64_t W) {
  const uint64_t HW = H * W, vol = H * (W - kSdD) * kSdD;
  SdLayout L;
  uint64_t o = 0;
  L.grey = o; o = align_up(o + 2 * HW);
  L.pack = o; o = align_up(o + 2 * HW * 8);
  L.C = o; o = align_up(o + vol * 2);
  L.L = o; o = align_up(o + kSdPaths * vol * 2);
  L.vote = o; o = align_up(o + HW * 4);
  L.disp = o; o = align_up(o + HW * 2);
  L.bytes = o;
  return L;
}

bool sd_size_ok(int64_t H, int64_t W) { return H >= 1 && W > kSdD && H <= kSdMaxSide && W <= kSdMaxSide; }

struct SdScratch {
  uint8_t* grey;      // [2][H*W]
  uint2* pack;        // [2][H*W]: x = g | g_lo << 8 | g_hi << 16, y = the same of the grey
  uint16_t* hs;       // [H][Wv][64]
  uint16_t* C;        // [H][Wv][64]
  uint16_t* L;        // [5][H][Wv][64]: one volume per path direction
  unsigned* vote;     // [H][W]: (S << 6 | d) of the best voter of the RIGHT image's column, or all ones
  int16_t* disp;      // [H][W] before the left-right check
};

// ---- rectify + grey ---------------------------------------------------------------------------------------------------
// float -> the uint8 level: rint (half to even) of v * 255 in fp32, clamped to [0, 255]; NaN gives 0.
__device__ __forceinline__ int quantise(float v) {
#pragma clang fp contract(off)
  return (int)fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f);
}

// OpenCV's fixed-point RGB -> grey
__device__ __forceinline__ int grey_of(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

__global__ __launch_bounds__(kSdThreads) void k_sd_grey(const mgs_stereo_depth_args A, const SdScratch S) {
  const int H = A.height, W = A.width;
  const size_t HW = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
  if (i >= HW) return;
  const int img = blockIdx.y;
  const void* in = img ? A.right_in : A.left_in;
  const int32_t* map = img ? A.map_right : A.map_left;
  int k;
  if (map) {
    const FpTaps t = remap_taps(map, i, H, W);
    if (A.image_format == MGS_STEREO_IMAGE_U8_GREY) {
      k = blend_u8_int(t, static_cast<const uint8_t*>(in), 0, 1);
    } else if (A.image_format == MGS_STEREO_IMAGE_U8_HWC) {
      const uint8_t* u = static_cast<const uint8_t*>(in);
      k = grey_of(blend_u8_int(t, u, 0), blend_u8_int(t, u, 1), blend_u8_int(t, u, 2));
    } else {
      const float* f = static_cast<const float*>(in);
      k = grey_of(quantise(blend_f32(t, f)), quantise(blend_f32(t, f + HW)), quantise(blend_f32(t, f + 2 * HW)));
    }
  } else if (A.image_format == MGS_STEREO_IMAGE_U8_GREY) {
    k = static_cast<const uint8_t*>(in)[i];
  } else if (A.image_format == MGS_STEREO_IMAGE_U8_HWC) {
    const uint8_t* u = static_cast<const uint8_t*>(in) + 3 * i;
    k = grey_of(u[0], u[1], u[2]);
  } else {
    const float* f = static_cast<const float*>(in);
    k = grey_of(quantise(f[i]), quantise(f[HW + i]), quantise(f[2 * HW + i]));
  }
  S.grey[(size_t)img * HW + i] = (uint8_t)k;
  if (img == 0 && A.image) {
    const float v = (float)((double)k / 255.0);
    A.image[i] = v;
    A.image[HW + i] = v;
    A.image[2 * HW + i] = v;
  }
}

// ---- prefilter + Birchfield-Tomasi bounds -------------------------------------------------------------------------------
// the clipped horizontal Sobel response at (y, x); rows clamped, 15 in the first and the last column
__device__ __forceinline__ int sobel_x(const uint8_t* I, int y, int x, int H, int W) {
  if (x <= 0 || x >= W - 1) return kSdFt;
  const uint8_t* r1 = I + (size_t)y * W;
  const uint8_t* r0 = I + (size_t)max(y - 1, 0) * W;
  const uint8_t* r2 = I + (size_t)min(y + 1, H - 1) * W;
  const int g = 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r0[x + 1] - (int)r0[x - 1]) +
                ((int)r2[x + 1] - (int)r2[x - 1]);
  return min(max(g, -kSdFt), kSdFt) + kSdFt;
}

// value, min and max of {u, (u + left) / 2, (u + right) / 2} in one word
__device__ __forceinline__ unsigned bt_word(int l, int u, int r) {
  const int ul = (u + l) >> 1, ur = (u + r) >> 1;
  const int lo = min(u, min(ul, ur)), hi = max(u, max(ul, ur));
  return (unsigned)u | (unsigned)lo << 8 | (unsigned)hi << 16;
}

__global__ __launch_bounds__(kSdThreads) void k_sd_pack(const SdScratch S, int H, int W) {
  const size_t HW = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
  if (i >= HW) return;
  const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
  const uint8_t* I = S.grey + (size_t)blockIdx.y * HW;
  const int xl = max(x - 1, 0), xr = min(x + 1, W - 1);            // neighbours clamped
  const uint8_t* row = I + (size_t)y * W;
  uint2 w;
  w.x = bt_word(sobel_x(I, y, xl, H, W), sobel_x(I, y, x, H, W), sobel_x(I, y, xr, H, W));
  w.y = bt_word(row[xl], row[x], row[xr]);
  S.pack[(size_t)blockIdx.y * HW + i] = w;
}

// ---- cost volume --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bt_cost(unsigned a, unsigned b) {
  const int u = a & 255, u0 = (a >> 8) & 255, u1 = (a >> 16) & 255;
  const int v = b & 255, v0 = (b >> 8) & 255, v1 = (b >> 16) & 255;
  const int c0 = max(0, max(u - v1, v0 - u)), c1 = max(0, max(v - u1, u0 - v));
  return min(c0, c1) >> 2;
}

// the pixel cost of lane d at column x (clamped to the valid columns) of a row: x >= 64 > d, so x - d >= 1
__device__ __forceinline__ int pixel_cost(const uint2* rowL, const uint2* rowR, int x, int W, int d) {
  x = min(max(x, kSdD), W - 1);
  const uint2 a = rowL[x], b = rowR[x - d];
  return bt_cost(a.x, b.x) + bt_cost(a.y, b.y);
}

__global__ __launch_bounds__(kSdThreads) void k_sd_hsum(const SdScratch S, int H, int W, int r) {
  const int Wv = W - kSdD, nseg = (Wv + kSdSegX - 1) / kSdSegX;
  const int64_t wv = (int64_t)blockIdx.x * kSdWaves + (threadIdx.x >> 6);      // wave-uniform
  if (wv >= (int64_t)H * nseg) return;
  const int y = (int)(wv / nseg), seg = (int)(wv - (int64_t)y * nseg), d = threadIdx.x & 63;
  const uint2* rowL = S.pack + (size_t)y * W;
  const uint2* rowR = S.pack + (size_t)H * W + (size_t)y * W;
  const int xs = kSdD + seg * kSdSegX, xe = min(xs + kSdSegX, W);
  int run = 0;
  for (int dx = -r; dx <= r; dx++) run += pixel_cost(rowL, rowR, xs + dx, W, d);
  uint16_t* out = S.hs + ((size_t)y * Wv + (xs - kSdD)) * kSdD + d;
  for (int x = xs;; x++) {
    *out = (uint16_t)run;
    if (x + 1 >= xe) break;
    out += kSdD;
    run += pixel_cost(rowL, rowR, x + 1 + r, W, d) - pixel_cost(rowL, rowR, x - r, W, d);
  }
}

// four 16-bit sums in a uint2: no half carries (a window sum is at most 65 535) and none borrows (what is subtracted is
// part of the sum)
__device__ __forceinline__ uint2 add4(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ uint2 sub4(uint2 a, uint2 b) { return make_uint2(a.x - b.x, a.y - b.y); }

__global__ __launch_bounds__(kSdThreads) void k_sd_vsum(const SdScratch S, int H, int W, int r) {
  const size_t stride = (size_t)(W - kSdD) * (kSdD / 4);           // uint2 words per row
  const size_t i = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
  if (i >= stride) return;
  const uint2* hs = reinterpret_cast<const uint2*>(S.hs) + i;
  uint2* C = reinterpret_cast<uint2*>(S.C) + i;
  const int ys = blockIdx.y * kSdSegY, ye = min(ys + kSdSegY, H);
  uint2 run = make_uint2(0u, 0u);
  for (int dy = -r; dy <= r; dy++) run = add4(run, hs[(size_t)min(max(ys + dy, 0), H - 1) * stride]);
  for (int y = ys;; y++) {
    C[(size_t)y * stride] = run;
    if (y + 1 >= ye) break;
    run = sub4(add4(run, hs[(size_t)min(y + 1 + r, H - 1) * stride]), hs[(size_t)max(y - r, 0) * stride]);
  }
}

// ---- aggregation ----------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ int sd_dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }

// the minimum over the wave's 64 lanes, the same (scalar) value in every lane; all lanes active
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, sd_dpp<0xB1>(v, v));       // quad_perm:[1,0,3,2]
  v = min(v, sd_dpp<0x4E>(v, v));       // quad_perm:[2,3,0,1]
  v = min(v, sd_dpp<0x141>(v, v));      // row_half_mirror
  v = min(v, sd_dpp<0x140>(v, v));      // row_mirror: every lane holds its 16-lane row's minimum
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// One path: start pixel (xv, y) in valid-column coordinates, step (dx, dy), n pixels.
struct SdPath { int xv, y, dx, dy, n, dir; };

__device__ __forceinline__ SdPath sd_path(int64_t p, int H, int Wv) {
  SdPath P;
  if (p < H) { P = {0, (int)p, 1, 0, Wv, 0}; return P; }                     // predecessor (x-1, y)
  p -= H;
  if (p < H) { P = {Wv - 1, (int)p, -1, 0, Wv, 1}; return P; }               // (x+1, y)
  p -= H;
  if (p < Wv) { P = {(int)p, 0, 0, 1, H, 2}; return P; }                     // (x, y-1)
  p -= Wv;
  const int nd = Wv + H - 1;
  const bool right = p < nd;                                                  // (x-1, y-1): the path runs down-right
  if (!right) p -= nd;                                                        // (x+1, y-1): down-left
  const int xv = p < Wv ? (int)p : 0, y = p < Wv ? 0 : (int)(p - Wv) + 1;     // from the top row, then from the side
  if (right) P = {xv, y, 1, 1, min(Wv - xv, H - y), 3};
  else P = {Wv - 1 - xv, y, -1, 1, min(Wv - xv, H - y), 4};
  return P;
}

__global__ __launch_bounds__(kSdThreads) void k_sd_aggregate(const SdScratch S, int H, int W, int64_t num_paths) {
  const int Wv = W - kSdD, d = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kSdWaves + (threadIdx.x >> 6);      // wave-uniform
  if (p >= num_paths) return;
  const SdPath P = sd_path(p, H, Wv);
  const int64_t step = ((int64_t)P.dy * Wv + P.dx) * kSdD;
  int64_t o = ((int64_t)P.y * Wv + P.xv) * kSdD + d;
  uint16_t* out = S.L + (int64_t)P.dir * H * Wv * kSdD;                       // L <= C + P2 fits 16 bits
  int L = S.C[o];                                                             // no predecessor: L = C
  int c_next = P.n > 1 ? (int)S.C[o + step] : 0;
  out[o] = (uint16_t)L;
  for (int k = 1; k < P.n; k++) {
    o += step;
    const int c = c_next;
    if (k + 1 < P.n) c_next = S.C[o + step];                                  // in flight during the chain below
    const int m = wave_min(L);
    const int lo = sd_dpp<0x138>(kSdBig, L);                                  // wave_shr:1: lane d reads d - 1
    const int hi = sd_dpp<0x130>(kSdBig, L);                                  // wave_shl:1: lane d reads d + 1
    L = c + min(min(L, min(lo, hi) + kSdP1), m + kSdP2) - m;
    out[o] = (uint16_t)L;
  }
}

// ---- selection --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSdThreads) void k_sd_select(const SdScratch S, int H, int W, int uniq) {
  const int Wv = W - kSdD, d = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * kSdWaves + (threadIdx.x >> 6);      // wave-uniform
  if (p >= (int64_t)H * Wv) return;
  const int y = (int)(p / Wv), x = (int)(p - (int64_t)y * Wv) + kSdD;
  const int64_t vol = (int64_t)H * Wv * kSdD;
  int s = 0;                                                                  // < 2^19
#pragma unroll
  for (int k = 0; k < kSdPaths; k++) s += S.L[k * vol + p * kSdD + d];
  const int key = wave_min(s << 6 | d);                                       // the smallest d among the smallest S
  const int b = key & 63, sb = key >> 6;
  const bool far = d < b - 1 || d > b + 1;
  const bool not_unique = __ballot(far && s * (100 - uniq) < sb * 100) != 0ull;
  const int sm = __shfl(s, max(b - 1, 0)), sp = __shfl(s, min(b + 1, kSdD - 1));
  if (d != 0) return;
  int disp = -16;
  if (!not_unique) {
    atomicMin(&S.vote[(size_t)y * W + (x - b)], (unsigned)key);               // x - b >= 1
    disp = 16 * b;
    if (b > 0 && b < kSdD - 1) {
      const int den = max(sm + sp - 2 * sb, 1), num = (sm - sp) * 16 + den;
      disp += num / (2 * den);                                                // C division: toward zero
    }
  }
  S.disp[(size_t)y * W + x] = (int16_t)disp;
}

__device__ __forceinline__ bool sd_disagrees(const unsigned* vote_row, int x, int cand, int W) {
  const int xc = x - cand;
  if (xc < 0 || xc >= W) return false;
  const unsigned v = vote_row[xc];
  return v != kSdNoVote && (int)(v & 63u) != cand;
}

__global__ __launch_bounds__(kSdThreads) void k_sd_finish(const mgs_stereo_depth_args A, const SdScratch S) {
  const int H = A.height, W = A.width;
  const size_t i = (size_t)blockIdx.x * kSdThreads + threadIdx.x;
  if (i >= (size_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
  int d1 = x < kSdD ? -16 : (int)S.disp[i];
  if (d1 >= 0) {
    const unsigned* vote_row = S.vote + (size_t)y * W;
    if (sd_disagrees(vote_row, x, d1 >> 4, W) && sd_disagrees(vote_row, x, (d1 + 15) >> 4, W)) d1 = -16;
  }
  if (A.disp16) A.disp16[i] = (int16_t)d1;
  double disp = (double)d1 / 16.0;
  if (disp == 0.0) disp = 1e10;
  const float depth = (float)(A.bf / disp);
  A.depth[i] = depth < 0.f ? 0.f : depth;
}

int32_t stereo_args_status(const mgs_stereo_depth_args* a) {
  if (!a || a->width < 1 || a->height < 1) return MGS_ERR_BAD_ARGUMENT;
  if (a->image_format < MGS_STEREO_IMAGE_U8_GREY || a->image_format > MGS_STEREO_IMAGE_F32_CHW) return MGS_ERR_BAD_ARGUMENT;
  if (a->block_size < 1 || a->uniqueness_ratio < 0 || a->uniqueness_ratio > 100) return MGS_ERR_BAD_ARGUMENT;
  if (!a->left_in || !a->right_in || !a->depth || !a->scratch) return MGS_ERR_BAD_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(a->scratch) & 15u) return MGS_ERR_BAD_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(a->map_left) & 7u) || (reinterpret_cast<uintptr_t>(a->map_right) & 7u))
    return MGS_ERR_BAD_ARGUMENT;
  if (a->width <= kSdD) return MGS_ERR_BAD_ARGUMENT;                         // no valid column
  if (a->num_disparities != kSdD || a->block_size / 2 > kSdMaxHalfBlock) return MGS_ERR_UNSUPPORTED;
  if (!sd_size_ok(a->height, a->width)) return MGS_ERR_UNSUPPORTED;
  return MGS_OK;
}

int launch_stereo_depth(const mgs_stereo_depth_args& A, hipStream_t st) {
  const int H = A.height, W = A.width, Wv = W - kSdD, r = A.block_size / 2;
  const SdLayout L = sd_layout((uint64_t)H, (uint64_t)W);
  char* w = static_cast<char*>(A.scratch);
  SdScratch S{};
  S.grey = reinterpret_cast<uint8_t*>(w + L.grey);
  S.pack = reinterpret_cast<uint2*>(w + L.pack);
  S.hs = reinterpret_cast<uint16_t*>(w + L.L);
  S.C = reinterpret_cast<uint16_t*>(w + L.C);
  S.L = reinterpret_cast<uint16_t*>(w + L.L);
  S.vote = reinterpret_cast<unsigned*>(w + L.vote);
  S.disp = reinterpret_cast<int16_t*>(w + L.disp);
  const uint64_t HW = (uint64_t)H * W;
  const auto blocks = [](uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); };
  const dim3 block(kSdThreads);
  const unsigned pix_blocks = blocks(HW, kSdThreads);
  launch("sd_grey", k_sd_grey, dim3(pix_blocks, 2), block, st, A, S);
  launch("sd_pack", k_sd_pack, dim3(pix_blocks, 2), block, st, S, H, W);
  const uint64_t nseg = (uint64_t)(Wv + kSdSegX - 1) / kSdSegX;
  launch("sd_hsum", k_sd_hsum, dim3(blocks((uint64_t)H * nseg, kSdWaves)), block, st, S, H, W, r);
  launch("sd_vsum", k_sd_vsum, dim3(blocks((uint64_t)Wv * (kSdD / 4), kSdThreads), blocks((uint64_t)H, kSdSegY)), block,
         st, S, H, W, r);
  if (!hip_ok("stereo depth memset", hipMemsetAsync(S.vote, 0xff, HW * 4, st))) {
    launches_ok();
    return MGS_ERR_LAUNCH;
  }
  const int64_t num_paths = 2 * (int64_t)H + Wv + 2 * ((int64_t)Wv + H - 1);
  launch("sd_aggregate", k_sd_aggregate, dim3(blocks((uint64_t)num_paths, kSdWaves)), block, st, S, H, W, num_paths);
  launch("sd_select", k_sd_select, dim3(blocks((uint64_t)H * Wv, kSdWaves)), block, st, S, H, W,
         (int)A.uniqueness_ratio);
  launch("sd_finish", k_sd_finish, dim3(pix_blocks), block, st, A, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace

}  // namespace mgs

extern "C" {

int32_t mgs_stereo_depth_args_size(void) { return (int32_t)sizeof(mgs_stereo_depth_args); }

uint64_t mgs_stereo_scratch_bytes(int32_t H, int32_t W) {
  if (!mgs::sd_size_ok(H, W)) return 0;
  return mgs::sd_layout((uint64_t)H, (uint64_t)W).bytes;
}

int32_t mgs_stereo_depth(const mgs_stereo_depth_args* args, void* stream) {
  const int32_t rc = mgs::stereo_args_status(args);
  if (rc != MGS_OK) return rc;
  return mgs::launch_stereo_depth(*args, (hipStream_t)stream);
}

}  // extern "C"
