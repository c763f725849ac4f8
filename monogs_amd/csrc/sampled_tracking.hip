// Pixel-sampled first-order tracking (mgs_tracking_iteration_sampled; DESIGN.md "Pixel-sampled first-order
// tracking").  The forward is the full render; only the GRADIENT is estimated from K pixels drawn with
// probability q_i = v_i / sum v, v_i = sum_c |r_ic| + 1e-8, weighted by 1 / (K q_i):
//   k_samp_weights   1 workgroup / tile: the residual rows of its 256 pixels -> v (tile order), and the
//                    tile sums of |h|^p (the exact objective), of |r| (best-iterate L1) and of v
//   k_samp_scan      1 workgroup: fp64 prefix of the tile sums of v, and the K draws as SORTED uniforms
//                    (normalised partial sums of K + 1 exponentials from a counter-based hash of (key, i)):
//                    the order statistics of K iid uniforms, so the drawn pixels come out in tile order
//   k_samp_draw      1 wave / sample: inverse CDF - the tile by binary search, the pixel by a wave scan
//   k_samp_replay    (replay_indices only) 1 workgroup: the given pixels ranked into tile order
//   k_samp_pose_bwd  1 workgroup / tile: the tile's samples replay its list front to back from the forward's
//                    per-item checkpoints (lanes = the 32 splats of an item, half a wave per sample); the six
//                    screen-space sums of a splat are added over the tile's samples and chained to d tau
//                    (raster_math.h: project_gaussian_backward, as k_preprocess_bwd) once per (tile, splat)
// No float atomics: every sum has a fixed order, so two runs are bit-identical.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "objective_math.h"
#include "raster_kernels.h"

namespace mgs {

constexpr int kSampWaves = 8;          // waves per workgroup of k_samp_pose_bwd
constexpr int kSampChunk = 256;        // samples staged in LDS at a time by k_samp_pose_bwd

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// tile-order position (tile * 256 + quadrant-major index) -> pixel
__device__ __forceinline__ void pos_to_xy(int pos, int grid_x, int& x, int& y) {
  const int tile = pos >> 8, r = pos & 255, q = r >> 6, l = r & 63;
  x = (tile % grid_x) * kTile + (l & 7) + 8 * (q & 1);
  y = (tile / grid_x) * kTile + (l >> 3) + 8 * (q >> 1);
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// residual rows of one pixel (objective_math.h: the rows of track_loss_pass), their value sums and
// the UN-normalised upstream gradient: gr[c] = d(sum_c |h_c|^p / p)/d(image_c) / gain, gd = .../d depth
struct SampPixel {
  float psi, l1, v, gr[3], gd;
};

__device__ __forceinline__ void samp_pixel(const KS& S, size_t p, float gain, float bias, SampPixel& o) {
  const size_t HW = (size_t)S.HW;
  const float pn = norm_p(S.pnorm);
  const float opa = S.opacity[p];
  const float om = opa * (S.mask ? S.mask[p] : 1.f);
  const float wr = S.rgbd ? S.w_rgb : 1.f;
  ObjSums s = {0.f, 0.f, 0.f, 0.f};       // (the exposure sums are not used: the backward forms them per sample)
  o.gd = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float im = S.image[c * HW + p], gt = S.gt[c * HW + p];
    o.gr[c] = colour_row(S.rgbd, om, gain, bias, im, gt, wr, 1.f, S.huber_delta, pn, s);
  }
  if (S.rgbd)
    o.gd = depth_row(S.gt_depth[p], opa, S.depth[p], S.depth_thr, S.opa_thr, S.w_depth, S.huber_delta, pn, s);
  o.psi = s.phi; o.l1 = s.l1;
  o.v = o.l1 + 1e-8f;
}

__global__ __launch_bounds__(256) void k_samp_weights(KP P, KS S) {
  __shared__ float s_red[3][4];
  const int tile = blockIdx.x, pos = tile * 256 + threadIdx.x;
  int x, y;
  pos_to_xy(pos, P.grid_x, x, y);
  const float gain = fabsf(S.exposure_a[0]) + S.exposure_eps, bias = S.exposure_b[0];
  SampPixel px;
  px.psi = 0.f; px.l1 = 0.f; px.v = 0.f;
  if (x < P.W && y < P.H) samp_pixel(S, (size_t)y * P.W + x, gain, bias, px);
  S.v[pos] = px.v;
  const float a = wsum(px.psi), b = wsum(px.l1), c = wsum(px.v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_red[0][wave] = a; s_red[1][wave] = b; s_red[2][wave] = c; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float* r = s_red[threadIdx.x];
    S.part[threadIdx.x * P.T + tile] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

// inclusive fp64 scan of one value per thread over a 1024-thread workgroup: a shuffle scan per wave, then the 16
// wave totals (fixed order throughout)
__device__ double block_scan_incl(double v, double* s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  if (lane == 63) s[wave] = v;
  __syncthreads();
  double before = 0.0;
  for (int w = 0; w < wave; w++) before += s[w];
  __syncthreads();
  return before + v;
}

__global__ __launch_bounds__(1024) void k_samp_scan(KS S) {
  __shared__ double s[16];
  __shared__ double s_total, s_sum;
  // (1) prefix[t] = sum of the tile sums of v in front of tile t (fp64), prefix[T] = total
  const int T = S.T;
  {
    const int per = (T + 1023) / 1024, i0 = min(T, (int)threadIdx.x * per), i1 = min(T, i0 + per);
    double acc = 0.0;
    for (int i = i0; i < i1; i++) acc += (double)S.part[2 * T + i];
    double run = block_scan_incl(acc, s) - acc;
    for (int i = i0; i < i1; i++) { S.prefix[i] = run; run += (double)S.part[2 * T + i]; }
    if (threadIdx.x == 1023) { S.prefix[T] = run; s_total = run; }
  }
  if (S.replay) return;
  __syncthreads();
  const double total = s_total;
  // (2) target[k] = total * E_0..k / E_0..K: K sorted uniforms (exponential spacings), i.e. K iid draws in order
  const int n = S.K + 1, per = (n + 1023) / 1024, i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
  auto expo = [&](int i) {
    const unsigned long long h = splitmix64(S.key ^ splitmix64(0x632BE59BD9B4E019ull + (unsigned long long)i));
    const double u = ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);   // (0, 1)
    return -log(u);
  };
  double acc = 0.0;
  for (int i = i0; i < i1; i++) acc += expo(i);
  const double incl = block_scan_incl(acc, s);
  if (threadIdx.x == 1023) s_sum = incl;           // sum of all K + 1 exponentials
  __syncthreads();
  const double norm = total / s_sum;
  double run = incl - acc;
  for (int i = i0; i < i1 && i < S.K; i++) { run += expo(i); S.target[i] = run * norm; }
}

// one wave per sample: tile by binary search over the prefix, pixel by a wave scan over the tile's v
__global__ __launch_bounds__(256) void k_samp_draw(KP P, KS S) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= S.K) return;
  const double t = S.target[k];
  int lo = 0, hi = S.T - 1;                      // last tile with prefix <= t and some mass
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (S.prefix[mid] <= t) lo = mid; else hi = mid - 1;
  }
  while (lo > 0 && S.prefix[lo + 1] <= S.prefix[lo]) lo--;     // rounding at the top end: an empty tile
  const double rr = t - S.prefix[lo];
  const float4 v4 = reinterpret_cast<const float4*>(S.v + (size_t)lo * 256)[lane];
  const double ls = ((double)v4.x + (double)v4.y) + ((double)v4.z + (double)v4.w);
  double incl = ls;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  const unsigned long long hit = __ballot(incl > rr);
  const unsigned long long pos_m = __ballot(ls > 0.0);
  int sel, e = 3;
  if (hit) {
    sel = __builtin_ctzll(hit);
  } else {
    sel = 63 - __builtin_clzll(pos_m);          // rounding: the last pixel with mass
  }
  const double excl = __shfl(incl - ls, sel);
  const float vv[4] = {__shfl(v4.x, sel), __shfl(v4.y, sel), __shfl(v4.z, sel), __shfl(v4.w, sel)};
  if (hit) {
    double run = excl;
    e = 3;
    for (int i = 0; i < 4; i++) { run += (double)vv[i]; if (run > rr) { e = i; break; } }
  }
  while (e > 0 && vv[e] <= 0.f) e--;
  if (lane == 0) {
    const int pos = lo * 256 + 4 * sel + e;
    int x, y;
    pos_to_xy(pos, P.grid_x, x, y);
    S.pos[k] = pos;
    S.weight[k] = vv[e] > 0.f ? (float)(S.prefix[S.T] / ((double)S.K * (double)vv[e])) : 0.f;
    S.indices[k] = y * P.W + x;
  }
}

// replay: the given flat pixel indices ranked into tile order (ties by input order); weights as for a draw
__global__ __launch_bounds__(1024) void k_samp_replay(KP P, KS S) {
  const int K = S.K;
  auto key = [&](int i) {
    const int f = S.replay_idx[i];
    if (f < 0 || f >= S.HW) return 0x7fffffff;     // out of range: sorts last, weight 0
    const int x = f % P.W, y = f / P.W, tx = x / kTile, ty = y / kTile, xi = x % kTile, yi = y % kTile;
    return (ty * P.grid_x + tx) * 256 + 64 * ((yi >> 3) * 2 + (xi >> 3)) + (yi & 7) * 8 + (xi & 7);
  };
  for (int i = threadIdx.x; i < K; i += 1024) {
    const int ki = key(i);
    int rank = 0;
    for (int j = 0; j < K; j++) {
      const int kj = key(j);
      rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    const bool ok = ki != 0x7fffffff;
    const float v = ok ? S.v[ki] : 0.f;
    S.pos[rank] = ok ? ki : 0x7fffffff;
    S.indices[rank] = S.replay_idx[i];
    S.weight[rank] = (ok && v > 0.f) ? (float)(S.prefix[S.T] / ((double)K * (double)v)) : 0.f;
  }
}

__device__ __forceinline__ void load_camera_s(Camera& c, const KP& P) {
#pragma unroll
  for (int i = 0; i < 16; i++) { c.V[i] = P.V[i]; c.PM[i] = P.PM[i]; c.Praw[i] = P.Praw[i]; }
  c.campos[0] = P.campos[0]; c.campos[1] = P.campos[1]; c.campos[2] = P.campos[2];
  c.W = P.W; c.H = P.H; c.tanfovx = P.tanfovx; c.tanfovy = P.tanfovy;
  c.focal_x = P.focal_x; c.focal_y = P.focal_y; c.scale_modifier = P.mod;
  c.sh_degree = P.deg; c.sh_coeffs = P.K; c.grid_x = P.grid_x; c.grid_y = P.grid_y;
  c.clamp_grad_upstream = P.clamp_up;
}

// first index in [0, K) whose sorted position is >= key
__device__ __forceinline__ int lower_pos(const int* pos, int K, int key) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pos[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// raw screen-space sums (Sx, Sy, Sxx, Sxy, Syy, Rd) of one splat -> d tau (the pose part of k_preprocess_bwd)
__device__ __forceinline__ void chain_tau(const KP& P, const Camera& cam, int id, const float a[6], float tau[6]) {
  const float4 r1 = reinterpret_cast<const float4*>(P.rec + id)[1];
  const float p[3] = {P.means[3 * id], P.means[3 * id + 1], P.means[3 * id + 2]};
  const float g_xy[2] = {-(r1.x * a[0] + r1.y * a[1]), -(r1.z * a[1] + r1.y * a[0])};
  const float g_con[3] = {-0.5f * a[2], -a[3], -0.5f * a[4]};
  GaussGrad gg;
  if (P.covp) {
    float c6[6];
#pragma unroll
    for (int i = 0; i < 6; i++) c6[i] = P.covp[6 * (size_t)id + i];
    project_gaussian_backward(cam, p, nullptr, nullptr, c6, g_xy, g_con, 0.f, a[5], gg);
  } else {
    const float sc[3] = {P.scales[3 * id], P.scales[3 * id + 1], P.scales[3 * id + 2]};
    const float4 qq = reinterpret_cast<const float4*>(P.rots)[id];
    const float q[4] = {qq.x, qq.y, qq.z, qq.w};
    project_gaussian_backward(cam, p, sc, q, nullptr, g_xy, g_con, 0.f, a[5], gg);
  }
#pragma unroll
  for (int i = 0; i < 6; i++) tau[i] += gg.dtau[i];
}

constexpr float kLog2eS = 1.4426950408889634f;

// orders this wave's LDS writes before its own later LDS reads (the chain queue belongs to one wave)
__device__ __forceinline__ void wave_lds_fence_s() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__global__ __launch_bounds__(64 * kSampWaves) void k_samp_pose_bwd(KP P, KS S) {
  // per staged sample: tile-order index r, n_contrib, weighted upstream (g0, g1, g2, gd), colour + depth still to
  // come behind the list start (final colour + T_final bg, final depth)
  __shared__ int s_r[kSampChunk], s_nc[kSampChunk];
  __shared__ float4 s_g[kSampChunk];
  __shared__ float4 s_f[kSampChunk];
  __shared__ float s_ex[2][kSampWaves];
  __shared__ int s_max[kSampWaves];
  __shared__ int s_qid[kSampWaves][64];
  __shared__ float s_qa[kSampWaves][6][64];
  __shared__ float s_tau[kSampWaves][6];
  const int tile = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kb = lower_pos(S.pos, S.K, tile * 256), ke = lower_pos(S.pos, S.K, tile * 256 + 256);
  if (kb >= ke) {
    if (threadIdx.x < 6) S.tau_part[tile * 6 + threadIdx.x] = 0.f;
    if (threadIdx.x < 2) S.expo_part[threadIdx.x * P.T + tile] = 0.f;
    return;
  }
  const float a_exp = S.exposure_a[0];
  const float gain = fabsf(a_exp) + S.exposure_eps, bias = S.exposure_b[0];
  const float sgn_a = a_exp > 0.f ? 1.f : (a_exp < 0.f ? -1.f : 0.f);
  const float bg0 = P.bg[0], bg1 = P.bg[1], bg2 = P.bg[2];
  const size_t HW = (size_t)S.HW;
  float tau[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ex_a = 0.f, ex_b = 0.f;                          // thread 0: the tile's exposure sums, chunk by chunk
  const int it0 = min(P.seg_offset[tile], P.max_segs), it1 = min(P.seg_offset[tile + 1], P.max_segs);
  const int j = lane & 31, half = lane >> 5;
  int qn = 0;                                            // entries of this wave's chain queue
  auto flush = [&]() {
    wave_lds_fence_s();
    if (lane < qn) {
      Camera cam;                                        // loaded here: not live across the walk (registers)
      load_camera_s(cam, P);
      float a[6];
#pragma unroll
      for (int i = 0; i < 6; i++) a[i] = s_qa[wave][i][lane];
      chain_tau(P, cam, s_qid[wave][lane], a, tau);
    }
    qn = 0;
    wave_lds_fence_s();
  };
  for (int c0 = kb; c0 < ke; c0 += kSampChunk) {
    const int ns = min(kSampChunk, ke - c0);
    // ---- stage the chunk's samples ----
    float ga = 0.f, gb = 0.f;
    int nc_t = 0;
    if ((int)threadIdx.x < ns) {
      const int k = c0 + threadIdx.x;
      const int pos = S.pos[k], r = pos & 255;
      int x, y;
      pos_to_xy(pos, P.grid_x, x, y);
      const size_t p = (size_t)y * P.W + x;
      const float wk = S.weight[k];
      SampPixel px;
      samp_pixel(S, p, gain, bias, px);
      const float4 tc = P.final_TC[(size_t)tile * 256 + r];
      const int2 dl = P.final_DL[(size_t)tile * 256 + r];
      float g[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        g[c] = wk * px.gr[c];
        ga += g[c] * S.image[c * HW + p];
        gb += g[c];
      }
      s_r[threadIdx.x] = r;
      s_nc[threadIdx.x] = wk != 0.f ? dl.y : 0;
      nc_t = wk != 0.f ? dl.y : 0;
      s_g[threadIdx.x] = make_float4(g[0] * gain, g[1] * gain, g[2] * gain, wk * px.gd);
      s_f[threadIdx.x] = make_float4(tc.y + tc.x * bg0, tc.z + tc.x * bg1, tc.w + tc.x * bg2, __int_as_float(dl.x));
    }
    {
      const float sa = wsum(ga), sb = wsum(gb);
      int m = nc_t;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
      if (lane == 0) { s_ex[0][wave] = sa; s_ex[1][wave] = sb; s_max[wave] = m; }
    }
    __syncthreads();
    int maxnc = 0;
    for (int w = 0; w < kSampWaves; w++) maxnc = max(maxnc, s_max[w]);
    if (threadIdx.x == 0)
      for (int w = 0; w < kSampWaves; w++) { ex_a += s_ex[0][w]; ex_b += s_ex[1][w]; }
    // ---- the tile's items, wave-strided; an item behind every sample's last contribution is not visited ----
    int4 sr_n = make_int4(0, 0, 0, 0);
    uint4 rw_n = make_uint4(0u, 0u, 0u, 0u);
    if (it0 + wave < it1) { sr_n = P.seg_rec[it0 + wave]; rw_n = P.reach[it0 + wave]; }
    for (int it = it0 + wave; it < it1; it += kSampWaves) {
      const int4 sr = sr_n;
      const uint4 rw = rw_n;
      if (it + kSampWaves < it1) { sr_n = P.seg_rec[it + kSampWaves]; rw_n = P.reach[it + kSampWaves]; }   // next item
      const int k0 = sr.y, nb = sr.z, base = sr.w;
      if (base >= maxnc) break;                 // items of a tile are in list order
      if (nb <= 0) continue;
      // the item's splat j in both halves of the wave
      const bool have = j < nb;
      unsigned int id = 0u;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = make_float4(0.f, 0.f, 0.f, 0.f);
      float2 bd = make_float2(0.f, 0.f);
      if (have) {
        const unsigned int lo = (unsigned int)P.keys[k0 + j];
        id = P.pack ? lo >> kPackBits : lo;
        const float4* src = reinterpret_cast<const float4*>(P.rec + id);
        const float4 qa = src[0];
        const float3 qb = *reinterpret_cast<const float3*>(src + 1), q2 = *reinterpret_cast<const float3*>(src + 2);
        u = make_float4(qa.x, qa.y, -0.5f * kLog2eS * qb.x, -kLog2eS * qb.y);
        v = make_float4(-0.5f * kLog2eS * qb.z, qa.w, q2.x, q2.y);
        bd = make_float2(q2.z, qa.z);
      }
      const float* ck = base > 0 ? P.ckpt + (size_t)it * (5 * 256) : nullptr;
      float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int g0i = 0; g0i < ns; g0i += 64) {
        // checkpoints of up to 64 samples, one per lane, in one round trip
        const int sl = g0i + lane;
        float4 k4 = make_float4(1.f, 0.f, 0.f, 0.f);
        float k3 = 0.f;
        if (ck && sl < ns && s_nc[sl] > base) {
          const int r = s_r[sl];
          k4 = reinterpret_cast<const float4*>(ck)[r];
          k3 = ck[1024 + r];
        }
        const int ng = min(64, ns - g0i);
        for (int pi = 0; pi < ng; pi += 2) {
          const int si = pi + half;                   // sample of this half, inside the group
          const bool sv = si < ng;
          const int sidx = g0i + (sv ? si : 0);
          const float4 c4 = make_float4(__shfl(k4.x, sidx - g0i), __shfl(k4.y, sidx - g0i), __shfl(k4.z, sidx - g0i),
                                        __shfl(k4.w, sidx - g0i));
          const float c3 = __shfl(k3, sidx - g0i);
          const int r = s_r[sidx], nc = sv ? s_nc[sidx] : 0;
          const float4 gg = s_g[sidx], ff = s_f[sidx];
          const int q = r >> 6, l = r & 63;
          const float px = (float)((tile % P.grid_x) * kTile + (l & 7) + 8 * (q & 1));
          const float py = (float)((tile / P.grid_x) * kTile + (l >> 3) + 8 * (q >> 1));
          const unsigned int rq = q == 0 ? rw.x : (q == 1 ? rw.y : (q == 2 ? rw.z : rw.w));
          const float dx = u.x - px, dy = u.y - py;
          const float pw = dx * (u.z * dx + u.w * dy) + v.x * dy * dy;
          const float ar = v.y * exp2_sat(pw);
          const bool k = have && base < nc && base + j < nc && ((rq >> j) & 1u) && ar >= kAlphaMin;
          const float a = k ? ar : 0.f;
          const float ae = fminf(kAlphaMax, a);
          const float om = 1.f - ae;
          // transmittance in front of splat j: checkpoint T times the product of (1 - alpha) of the splats before it
          float pr = om;
#pragma unroll
          for (int off = 1; off < 32; off <<= 1) {
            const float o = __shfl_up(pr, off, 32);
            if (j >= off) pr *= o;
          }
          float ex = __shfl_up(pr, 1, 32);
          if (j == 0) ex = 1.f;
          const float Tj = c4.x * ex;
          const float gc = __builtin_fmaf(gg.z, bd.x, gg.x * v.z) + __builtin_fmaf(gg.w, bd.y, gg.y * v.w);
          const float w = ae * Tj;
          float xs = w * gc;
#pragma unroll
          for (int off = 1; off < 32; off <<= 1) {
            const float o = __shfl_up(xs, off, 32);
            if (j >= off) xs += o;
          }
          const float gS0 = gg.x * (ff.x - c4.y) + gg.y * (ff.y - c4.z) + gg.z * (ff.z - c4.w) + gg.w * (ff.w - c3);
          const float gS = gS0 - xs;
          const float dA = Tj * gc - __builtin_amdgcn_rcpf(om) * gS;
          const float Wt = k ? a * dA : 0.f;
          const float wd = k ? w * gg.w : 0.f;
          acc[0] += Wt * dx; acc[1] += Wt * dy;
          acc[2] += Wt * dx * dx; acc[3] += Wt * dx * dy; acc[4] += Wt * dy * dy;
          acc[5] += wd;
        }
      }
      // the two halves walked the same splats: add them, then queue the splats that received something
#pragma unroll
      for (int i = 0; i < 6; i++) acc[i] += __shfl_down(acc[i], 32);
      const bool put = lane < 32 && have &&
                       (acc[0] != 0.f || acc[1] != 0.f || acc[2] != 0.f || acc[3] != 0.f || acc[4] != 0.f || acc[5] != 0.f);
      const unsigned long long pm = __ballot(put);
      const int cnt = __popcll(pm);
      if (cnt == 0) continue;
      if (qn + cnt > 64) flush();
      if (put) {
        const int at = qn + __popcll(pm & ((1ull << lane) - 1ull));
        s_qid[wave][at] = (int)id;
#pragma unroll
        for (int i = 0; i < 6; i++) s_qa[wave][i][at] = acc[i];
      }
      qn += cnt;
    }
    if (qn > 0) flush();
    __syncthreads();                             // the chunk's LDS is reused
  }
#pragma unroll
  for (int i = 0; i < 6; i++) tau[i] = wsum(tau[i]);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < 6; i++) s_tau[wave][i] = tau[i];
  __syncthreads();
  if (threadIdx.x < 6) {
    float s = 0.f;
    for (int w = 0; w < kSampWaves; w++) s += s_tau[w][threadIdx.x];
    S.tau_part[tile * 6 + threadIdx.x] = s;
  }
  if (threadIdx.x == 0) { S.expo_part[tile] = ex_a * sgn_a; S.expo_part[P.T + tile] = ex_b; }
}

// optional: the un-normalised estimate (tau[6] = [rho; theta], d/da, d/db) summed in tile order
__global__ __launch_bounds__(64) void k_samp_grad_out(KP P, KS S) {
  const int c = threadIdx.x;
  if (c >= 8) return;
  float s = 0.f;
  for (int t = 0; t < P.T; t++) s += c < 6 ? S.tau_part[t * 6 + c] : S.expo_part[(c - 6) * P.T + t];
  S.grad_out[c] = s;
}

SampLayout samp_layout(int T, int K) {
  SampLayout L;
  uint64_t o = 0;
  L.v = o; o = align_up(o + (uint64_t)T * 256 * 4);
  L.part = o; o = align_up(o + (uint64_t)T * 3 * 4);
  L.prefix = o; o = align_up(o + (uint64_t)(T + 1) * 8);
  L.target = o; o = align_up(o + (uint64_t)(K + 1) * 8);
  L.pos = o; o = align_up(o + (uint64_t)K * 4);
  L.weight = o; o = align_up(o + (uint64_t)K * 4);
  L.tau_part = o; o = align_up(o + (uint64_t)T * 6 * 4);
  L.expo_part = o; o = align_up(o + (uint64_t)T * 2 * 4);
  L.bytes = o;
  return L;
}

int launch_sampled_pose(const KP& P, const KS& S, hipStream_t st) {
  launch("samp_weights", k_samp_weights, dim3(P.T), dim3(256), st, P, S);
  launch("samp_scan", k_samp_scan, dim3(1), dim3(1024), st, S);
  if (S.replay) launch("samp_replay", k_samp_replay, dim3(1), dim3(1024), st, P, S);
  else launch("samp_draw", k_samp_draw, dim3((S.K + 3) / 4), dim3(256), st, P, S);
  launch("samp_pose_bwd", k_samp_pose_bwd, dim3(P.T), dim3(64 * kSampWaves), st, P, S);
  if (S.grad_out) launch("samp_grad_out", k_samp_grad_out, dim3(1), dim3(64), st, P, S);
  return launches_ok() ? MGS_OK : MGS_ERR_LAUNCH;
}

}  // namespace mgs
