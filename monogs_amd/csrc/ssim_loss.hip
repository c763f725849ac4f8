// Colour-refinement objective (utils/slam_backend.py:355-358 with gaussian_splatting/utils/loss_utils.py:21-22,
// 63-101):  loss = w_l1 * mean|x - y| + w_ssim * (1 - mean S(x, y)),  S the SSIM map of an 11x11 Gaussian window
// (sigma 1.5) applied per channel with ZERO padding, C1 = 0.01^2, C2 = 0.03^2 - value AND d loss / d x in ONE launch.
//
// Gradient of the SSIM term.  At an output pixel p, S is a function of the raw moments of x under the window:
// m1 = G*x, e11 = G*x^2, e12 = G*xy (and of y's, which are constants).  With the per-pixel partial maps
//   P0 = dS/dm1 (total: sigma1^2 = e11 - m1^2 and sigma12 = e12 - m1 m2 depend on m1), P1 = dS/de11, P2 = dS/de12
// (zero outside the image: only image pixels are averaged), the chain rule through the zero-padded, symmetric window
// gives  dS_mean/dx_q = (1/M) [G*P0 + 2 x_q G*P1 + y_q G*P2]_q  - the same 11x11 zero-padded filter again.
// The L1 term is sign(x - y) / M with sign(0) = 0, as torch's abs backward has it.  M = C H W for both means.
//
// One workgroup owns a 32x32 output tile of one channel and keeps everything in LDS:
//   stage   u, v (see Precision) over the tile +-10 (52x52, zero outside the image)
//   pass A  horizontal 11-tap filter of the five moment inputs (u, v, u^2, v^2, uv) over the tile +-5 columns
//   pass B  vertical 11-tap filter -> five moments at every pixel of the tile +-5; S (summed over the tile core) and
//           the three partial maps (written over pass A's buffer after a barrier)
//   pass C  horizontal filter of the three partial maps over the tile's columns
//   pass D  vertical filter -> the tile's gradient (stored), |x - y| summed
// Every pass is register-blocked: a thread filters a run of 3..8 consecutive outputs along the pass direction from
// one register window, so each LDS value feeds up to 11 taps.  Row strides are odd where lanes walk rows (passes A
// and C), so those column walks are free of bank conflicts; passes B and D walk along rows.
// The 2-D window is the outer product of the 1-D one, so the separable passes with zero padding are exact (up to the
// fp32 rounding of a different summation order).
//
// Precision.  sigma^2 = E[x^2] - mu^2 cancels badly in fp32 on bright, flat content (x ~ 0.9, sigma^2 ~ 1e-4: PyTorch's
// fp32 path is 6e-6 off in SSIM there).  The passes therefore filter the moments of u = x - c1, v = y - c2 (zero
// outside the image), c the tile-centre values, and recover the raw moments exactly with the window mass
// W1 = G*1 (< 1 near the border):  mu1 = G*u + c1 W1,  sigma1^2 = G*u^2 - (G*u)^2 + (1 - W1)(2 c1 G*u + c1^2 W1),
// sigma12 = G*uv - G*u G*v + (1 - W1)(c1 G*v + c2 G*u + c1 c2 W1).  The gradient is shift-invariant the same way:
// dS_mean/dx_q = (1/M) [G*P0' + 2 (x_q - c1) G*P1 + (y_q - c2) G*P2]_q with P0' = P0 + 2 c1 P1 + c2 P2.
//
// Reduction: one (l1, S) partial pair per workgroup, in a fixed order inside it; the workgroup that takes the last
// ticket (the int behind the 2 n partials: zero on entry, restored here) sums them in index order.  No float atomics:
// two identical calls give bit-identical values and gradients.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   k_ssim_loss: 118 VGPRs (4 waves/SIMD by registers), 0 AGPRs, 0 spills, 67200 B LDS -> 2 workgroups = 8 waves per
//   CU, "Occupancy [waves/SIMD]: 2".  Measured (profiles/refine_profile.txt): 53 us at 3x640x480 (208 GB/s of the
//   12 C H W algorithmic bytes), 132 us at 3x1200x680.  Not HBM-bound: at 2 waves per SIMD every pass is a dependent LDS
//   round trip behind a barrier with little to hide it.  A two-launch form (partial maps through HBM) was not built.
#include <hip/hip_runtime.h>

#include "../../include/monogs_raster.h"
#include "launch.h"

namespace mgs {

namespace ssim {
constexpr int kWin = 11, kR = 5;            // window, radius
constexpr int TX = 32, TY = 32;             // output tile
constexpr int kThreads = 256;
constexpr int IX = TX + 4 * kR, IY = TY + 4 * kR;      // staged inputs: tile +-10 (52 x 52)
constexpr int MX = TX + 2 * kR, MY = TY + 2 * kR;      // moment / partial-map ring: tile +-5 (42 x 42)
constexpr int IXS = IX + 1;                 // odd row strides where lanes walk rows
constexpr int MXS = MX + 1;
constexpr int QXS = TX + 1;
constexpr int kIn = IY * IXS;               // one staged image
constexpr int kH = IY * MXS;                // one horizontal moment plane
constexpr int kP = MY * MXS;                // one partial map
constexpr int kQ = MY * QXS;                // one horizontally filtered partial map
constexpr int kLds = 2 * kIn + 5 * kH;      // floats; P and Q live in the moment planes' space
static_assert(3 * kP + 3 * kQ <= 5 * kH, "partial maps must fit over the moment planes");
// register-blocked runs
constexpr int RA = 6, NA = (MX + RA - 1) / RA;         // pass A: 6 columns per item, 7 runs per row
constexpr int RB = 6, NB = (MY + RB - 1) / RB;         // pass B: 6 rows per item, 7 runs per column
constexpr int RC = 8, NC = TX / RC;                    // pass C: 8 columns per item
constexpr int RD = 4, ND = TY / RD;                    // pass D: 4 rows per item
constexpr int kItemsB = NB * MX;                       // 294
constexpr int kRoundsB = (kItemsB + kThreads - 1) / kThreads;
static_assert(ND * TX == kThreads, "pass D: one item per thread");
static_assert(NC * MY <= kThreads, "pass C: one round");
}  // namespace ssim

struct SsimWeights { float g[ssim::kWin]; };

__device__ __forceinline__ float block_sum_fixed(float v, float* s_red) {
  // fixed order: butterfly inside the wave, then the wave totals in wave order
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < ssim::kThreads / 64; w++) t += s_red[w];
  return t;
}

__global__ __launch_bounds__(ssim::kThreads) void k_ssim_loss(mgs_ssim_loss_args A, SsimWeights Wt) {
  using namespace ssim;
  __shared__ float smem[kLds];               // static: a dynamic request above 64 KiB needs a function attribute
  __shared__ float s_red[kThreads / 64];
  __shared__ float sWx[MX], sWy[MY];          // 1-D window mass over the image, per ring column / row
  float* sX = smem;
  float* sY = sX + kIn;
  float* sH = sY + kIn;                       // 5 planes [IY][MXS]: u, v, u^2, v^2, uv
  float* sP = sH;                             // 3 planes [MY][MXS] (after pass B)
  float* sQ = sH + 3 * kP;                    // 3 planes [MY][QXS]
  const int W = A.width, H = A.height;
  const int c = blockIdx.z;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)W * H;
  const float* img = A.image + c * plane;
  const float* gtp = A.gt + c * plane;
  const int tid = threadIdx.x;
  const bool want_grad = A.grad_image != nullptr;
  float g[kWin];
#pragma unroll
  for (int k = 0; k < kWin; k++) g[k] = Wt.g[k];
  // the shift: values at the tile centre (clamped into the image; the same for every thread)
  const size_t oc = (size_t)min(y0 + TY / 2, H - 1) * W + min(x0 + TX / 2, W - 1);
  const float c1 = img[oc], c2 = gtp[oc];

  // ---- stage u = x - c1, v = y - c2 over the tile +-10, zero outside the image; the window masses
  for (int i = tid; i < IX * IY; i += kThreads) {
    const int r = i / IX, q = i - r * IX;
    const int gx = x0 - 2 * kR + q, gy = y0 - 2 * kR + r;
    float uv = 0.f, vv = 0.f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t o = (size_t)gy * W + gx;
      uv = img[o] - c1;
      vv = gtp[o] - c2;
    }
    sX[r * IXS + q] = uv;
    sY[r * IXS + q] = vv;
  }
  if (tid < MX + MY) {
    const bool is_col = tid < MX;
    const int j = is_col ? tid : tid - MX;
    const int base = (is_col ? x0 : y0) - 2 * kR + j, n = is_col ? W : H;
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; k++) m += (base + k >= 0 && base + k < n) ? g[k] : 0.f;
    (is_col ? sWx : sWy)[j] = m;
  }
  __syncthreads();

  // ---- pass A: horizontal moments over rows [0, IY) x ring columns [0, MX) (input column = ring column + k)
  for (int i = tid; i < NA * IY; i += kThreads) {
    const int r = i % IY, run = i / IY;        // lanes walk rows (odd stride)
    const int c0 = run * RA;
    float wx[RA + kWin - 1], wy[RA + kWin - 1];
#pragma unroll
    for (int k = 0; k < RA + kWin - 1; k++) {
      const int q = min(c0 + k, IX - 1);     // the clamp only feeds outputs past MX, which are not stored
      wx[k] = sX[r * IXS + q];
      wy[k] = sY[r * IXS + q];
    }
#pragma unroll
    for (int j = 0; j < RA; j++) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; k++) {
        const float xv = wx[j + k], yv = wy[j + k];
        a0 = fmaf(g[k], xv, a0);
        a1 = fmaf(g[k], yv, a1);
        a2 = fmaf(g[k], xv * xv, a2);
        a3 = fmaf(g[k], yv * yv, a3);
        a4 = fmaf(g[k], xv * yv, a4);
      }
      if (c0 + j < MX) {
        const int o = r * MXS + c0 + j;
        sH[o] = a0; sH[kH + o] = a1; sH[2 * kH + o] = a2; sH[3 * kH + o] = a3; sH[4 * kH + o] = a4;
      }
    }
  }
  __syncthreads();

  // ---- pass B: vertical moments at the ring [0, MY) x [0, MX); S over the tile core; partial maps
  constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  float s_sum = 0.f;
  float pm[kRoundsB][RB][3];
#pragma unroll
  for (int rd = 0; rd < kRoundsB; rd++) {
    const int i = tid + rd * kThreads;
    if (i >= kItemsB) break;
    const int col = i % MX, run = i / MX;      // lanes walk columns
    const int r0 = run * RB;
    float m[5][RB];
#pragma unroll
    for (int t = 0; t < 5; t++) {
      float w[RB + kWin - 1];
#pragma unroll
      for (int k = 0; k < RB + kWin - 1; k++) w[k] = sH[t * kH + min(r0 + k, IY - 1) * MXS + col];
#pragma unroll
      for (int j = 0; j < RB; j++) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; k++) a = fmaf(g[k], w[j + k], a);
        m[t][j] = a;
      }
    }
    const int px = x0 - kR + col;
    const float wx = sWx[col];
#pragma unroll
    for (int j = 0; j < RB; j++) {
      const int py = y0 - kR + r0 + j;
      const float W1 = wx * sWy[min(r0 + j, MY - 1)], w1c = 1.f - W1;
      const float mu_u = m[0][j], mu_v = m[1][j];
      const float d1 = fmaf(c1, -w1c, mu_u), d2 = fmaf(c2, -w1c, mu_v);    // mu1 - c1, mu2 - c2
      const float mu1 = d1 + c1, mu2 = d2 + c2;
      const float s11 = m[2][j] - mu_u * mu_u + w1c * c1 * (2.f * mu_u + c1 * W1);
      const float s22 = m[3][j] - mu_v * mu_v + w1c * c2 * (2.f * mu_v + c2 * W1);
      const float s12 = m[4][j] - mu_u * mu_v + w1c * (c1 * mu_v + c2 * mu_u + c1 * c2 * W1);
      const float mu12 = mu1 * mu2;
      const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2;
      const float iB1 = 1.f / (mu1 * mu1 + mu2 * mu2 + C1), iB2 = 1.f / (s11 + s22 + C2);
      const float D = iB1 * iB2;
      const float S = A1 * A2 * D;
      const bool inside = r0 + j < MY && px >= 0 && px < W && py >= 0 && py < H;
      const bool core = inside && col >= kR && col < kR + TX && r0 + j >= kR && r0 + j < kR + TY;
      if (core) s_sum += S;
      const float P1 = -S * iB2, P2 = 2.f * A1 * D;
      const float D0 = 2.f * (mu2 * A2 * D - mu1 * S * iB1);                    // dS/dmu1 with the sigmas held
      pm[rd][j][0] = inside ? D0 - 2.f * d1 * P1 - d2 * P2 : 0.f;               // P0' (shifted chain rule)
      pm[rd][j][1] = inside ? P1 : 0.f;
      pm[rd][j][2] = inside ? P2 : 0.f;
    }
  }
  __syncthreads();                             // every read of the moment planes is done: P may overwrite them
  if (want_grad) {
#pragma unroll
    for (int rd = 0; rd < kRoundsB; rd++) {
      const int i = tid + rd * kThreads;
      if (i >= kItemsB) break;
      const int col = i % MX, r0 = (i / MX) * RB;
#pragma unroll
      for (int j = 0; j < RB; j++)
        if (r0 + j < MY) {
#pragma unroll
          for (int t = 0; t < 3; t++) sP[t * kP + (r0 + j) * MXS + col] = pm[rd][j][t];
        }
    }
  }
  __syncthreads();

  // ---- pass C: horizontal filter of the partial maps over ring rows [0, MY) x tile columns [0, TX)
  if (want_grad && tid < NC * MY) {
    const int r = tid % MY, run = tid / MY;    // lanes walk rows (odd stride)
    const int c0 = run * RC;
#pragma unroll
    for (int t = 0; t < 3; t++) {
      float w[RC + kWin - 1];
#pragma unroll
      for (int k = 0; k < RC + kWin - 1; k++) w[k] = sP[t * kP + r * MXS + c0 + k];
#pragma unroll
      for (int j = 0; j < RC; j++) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; k++) a = fmaf(g[k], w[j + k], a);
        sQ[t * kQ + r * QXS + c0 + j] = a;
      }
    }
  }
  __syncthreads();

  // ---- pass D: vertical filter -> gradient of the tile; L1 sums
  const float M = (float)((double)A.channels * (double)plane);
  const float go = A.grad_out ? A.grad_out[0] : 1.f;
  const float cl = A.w_l1 * go / M, cs = -A.w_ssim * go / M;
  float l1_sum = 0.f;
  {
    const int col = tid % TX, r0 = (tid / TX) * RD;     // lanes walk columns: coalesced stores
    float q[3][RD];
    if (want_grad) {
#pragma unroll
      for (int t = 0; t < 3; t++) {
        float w[RD + kWin - 1];
#pragma unroll
        for (int k = 0; k < RD + kWin - 1; k++) w[k] = sQ[t * kQ + (r0 + k) * QXS + col];
#pragma unroll
        for (int j = 0; j < RD; j++) {
          float a = 0.f;
#pragma unroll
          for (int k = 0; k < kWin; k++) a = fmaf(g[k], w[j + k], a);
          q[t][j] = a;
        }
      }
    }
    const int gx = x0 + col;
#pragma unroll
    for (int j = 0; j < RD; j++) {
      const int gy = y0 + r0 + j;
      if (gx < W && gy < H) {
        const int o = (r0 + j + 2 * kR) * IXS + col + 2 * kR;
        const size_t og = (size_t)gy * W + gx;
        const float d = img[og] - gtp[og];      // the residual as the reference forms it (L2-resident reload)
        l1_sum += fabsf(d);
        if (want_grad) {
          const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
          const float ds = q[0][j] + 2.f * sX[o] * q[1][j] + sY[o] * q[2][j];
          A.grad_image[c * plane + (size_t)gy * W + gx] = fmaf(cl, sg, cs * ds);
        }
      }
    }
  }

  // ---- per-workgroup partials, then the last workgroup's fixed-order sum
  const float tl = block_sum_fixed(l1_sum, s_red);
  const float ts = block_sum_fixed(s_sum, s_red);
  const int n = gridDim.x * gridDim.y * gridDim.z;
  const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  __shared__ int s_last;
  if (tid == 0) {   // write-through stores, then the ticket (as k_map_loss, tracking.hip)
    __hip_atomic_store(&A.partial[blk], tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&A.partial[n + blk], ts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    int* ticket = reinterpret_cast<int*>(A.partial + 2 * n);
    s_last = atomicAdd(ticket, 1) == n - 1;
    if (s_last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  // fixed order whatever workgroup is last: thread t sums partials t, t + 256, ... then the block sum
  double al = 0.0, as = 0.0;
  for (int i = tid; i < n; i += kThreads) {
    al += (double)__hip_atomic_load(&A.partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    as += (double)__hip_atomic_load(&A.partial[n + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __shared__ double s_dred[2][kThreads / 64];
  for (int off = 32; off > 0; off >>= 1) {
    al += __shfl_xor(al, off);
    as += __shfl_xor(as, off);
  }
  if ((tid & 63) == 0) { s_dred[0][tid >> 6] = al; s_dred[1][tid >> 6] = as; }
  __syncthreads();
  if (tid == 0) {
    double sl = 0.0, ss = 0.0;
    for (int w = 0; w < kThreads / 64; w++) { sl += s_dred[0][w]; ss += s_dred[1][w]; }
    const double Md = (double)A.channels * (double)plane;
    const float l1 = (float)(sl / Md), sv = (float)(ss / Md);
    if (A.l1) A.l1[0] = l1;
    if (A.ssim) A.ssim[0] = sv;
    A.loss[0] = A.w_l1 * l1 + A.w_ssim * (1.f - sv);
  }
}

// max_radii2D[i] = max(max_radii2D[i], radii[i]) where radii[i] > 0 (slam_backend.py:360-364; a float tensor there)
__global__ __launch_bounds__(256) void k_radii_fold(const int* __restrict__ radii, float* __restrict__ max_radii, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int r = radii[i];
    if (r > 0) max_radii[i] = fmaxf(max_radii[i], (float)r);
  }
}

int launch_radii_fold(const int* radii, float* max_radii, int n, hipStream_t st) {
  if (!radii || !max_radii || n < 1) return MGS_ERR_BAD_ARGUMENT;
  launch("radii_fold", k_radii_fold, dim3((n + 255) / 256), dim3(256), st, radii, max_radii, n);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

static SsimWeights ssim_weights() {
  // loss_utils.py:42-51: exp(-(x - 5)^2 / (2 sigma^2)) in double, stored as fp32, normalised in fp32
  SsimWeights w;
  float sum = 0.f;
  for (int k = 0; k < ssim::kWin; k++) {
    w.g[k] = (float)exp(-(double)((k - ssim::kR) * (k - ssim::kR)) / (2.0 * 1.5 * 1.5));
    sum += w.g[k];
  }
  for (int k = 0; k < ssim::kWin; k++) w.g[k] = w.g[k] / sum;
  return w;
}

static void ssim_grid(int32_t C, int32_t H, int32_t W, dim3& grid) {
  grid = dim3((unsigned)((W + ssim::TX - 1) / ssim::TX), (unsigned)((H + ssim::TY - 1) / ssim::TY), (unsigned)C);
}

}  // namespace mgs

using namespace mgs;

extern "C" {

int32_t mgs_ssim_loss_partial_count(int32_t channels, int32_t height, int32_t width) {
  if (channels < 1 || height < 1 || width < 1 || height > 65535 * ssim::TY || channels > 65535) return -1;
  dim3 g;
  ssim_grid(channels, height, width, g);
  const int64_t n = (int64_t)g.x * g.y * g.z;
  if (2 * n + 1 > 0x7fffffff) return -1;
  return (int32_t)(2 * n + 1);
}

int32_t mgs_ssim_loss(const mgs_ssim_loss_args* a, void* stream) {
  if (!a || !a->image || !a->gt || !a->partial || !a->loss) return MGS_ERR_BAD_ARGUMENT;
  if (mgs_ssim_loss_partial_count(a->channels, a->height, a->width) < 0) return MGS_ERR_BAD_ARGUMENT;
  dim3 grid;
  ssim_grid(a->channels, a->height, a->width, grid);
  static const SsimWeights w = ssim_weights();
  launch("ssim_loss", k_ssim_loss, grid, dim3(ssim::kThreads), (hipStream_t)stream, *a, w);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // extern "C"
