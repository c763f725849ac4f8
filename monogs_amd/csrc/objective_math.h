// Per-sample arithmetic of the tracking objective - the ONE definition of its colour and depth rows.  Users:
// track_loss_pass (tracking.hip), the objective epilogue of blend_fwd (raster_forward.hip), samp_pixel
// (sampled_tracking.hip) and, for the residuals only, sketch_residual_block (sketch_kernels.h).  All of them form the
// same residual bit for bit because all of them call these functions.
#pragma once
#include <hip/hip_runtime.h>

namespace mgs {

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Pseudo-Huber of the reference's tracking objective (utils/slam_utils.py:58-75): h(x) = x for |x| < delta,
// else sign(x) sqrt(2 delta |x| - delta^2); dh = dh/dx.  delta <= 0 switches it off.
__device__ __forceinline__ float huber(float x, float delta, float& dh) {
  const float ax = fabsf(x);
  if (delta <= 0.f || ax < delta) { dh = 1.f; return x; }
  const float s = sqrtf(2.f * delta * ax - delta * delta);
  dh = delta / s;
  return copysignf(s, x);
}

// The p-norm objective (sum |h|^p)^(1/p) of utils/slam_frontend.py:596-600 (p = 2 with Huber, RGN.pnorm
// without).  Per sample: phi = |h|^p (what is summed) and gam = |h|^(p-1) sign(h); with S = sum phi the value is
// loss = S^(1/p) and d loss / d h = loss^(1-p) gam - the scalar factor is applied by the consumer of the sums
// (norm_finish), everything in between being linear in it.  p = 2: (h^2, h), the form of rounds 1-3.
// p = 1: (|h|, sign h), sign(0) = 0 as torch.norm's derivative has it.
__device__ __forceinline__ float norm_p(float pnorm) { return pnorm > 0.f ? pnorm : 2.f; }

__device__ __forceinline__ void norm_terms(float h, float p, float& phi, float& gam) {
  if (p == 2.f) { phi = h * h; gam = h; return; }
  const float ah = fabsf(h);
  if (p == 1.f) { phi = ah; gam = sgn(h); return; }
  const float q = ah > 0.f ? powf(ah, p - 1.f) : 0.f;
  phi = q * ah; gam = copysignf(q, h);
}

// loss = S^(1/p) and scale = loss^(1-p) (0 when the loss is 0: torch.norm's derivative at the origin)
__device__ __forceinline__ void norm_finish(float S, float p, float& loss, float& scale) {
  if (p == 2.f) { loss = sqrtf(S); scale = loss > 0.f ? 1.f / loss : 0.f; return; }
  if (p == 1.f) { loss = S; scale = 1.f; return; }
  loss = S > 0.f ? powf(S, 1.f / p) : 0.f;
  scale = loss > 0.f ? powf(loss, 1.f - p) : 0.f;
}

// The four sums of the objective, in the order of its block partials: [n] sum |h|^p | [n] d/da | [n] d/db | [n] sum |r|
// (|r| before Huber: the best-iterate criterion).  d/da lacks sign(a): the writer of the partial applies it once.
struct ObjSums { float l1, db, da, phi; };

// The row functions take their operands BY REFERENCE so that each is read where its expression stands, as in the
// hand-inlined code they replace: the compiler then emits that code's instructions (checked on the ISA of k_blend_fwd
// and k_samp_*: identical to the form with the rows written out in place).

// Colour residual of one sample, om = opacity * mask.  RGB-D: times w_rgb at the caller, the Huber step comes after it.
__device__ __forceinline__ float colour_residual(const float& om, const float& gain, const float& bias, const float& im,
                                                 const float& gt) {
  return om * (gain * im + bias - gt);
}

// Colour row: adds to the four sums and returns g = d/d(gain * image + bias) = ((k gam) dh) om [w_rgb], WITHOUT the
// norm's loss^(1-p); d/d image = g * gain.  k is the upstream factor (1.f, exact, where the consumer of the sums
// applies it).  weighted (RGB-D: the row times w_rgb) is a compile-time constant at every site but samp_pixel.
__device__ __forceinline__ float colour_row(bool weighted, const float& om, const float& gain, const float& bias,
                                            const float& im, const float& gt, const float& w_rgb, const float& k,
                                            const float& delta, const float& p, ObjSums& s) {
  float r = colour_residual(om, gain, bias, im, gt);
  if (weighted) r *= w_rgb;
  s.l1 += fabsf(r);
  float dh, phi, gam;
  const float h = huber(r, delta, dh);
  norm_terms(h, p, phi, gam);
  s.phi += phi;
  float g = k * gam * dh * om;
  if (weighted) g *= w_rgb;
  s.da += g * im;
  s.db += g;
  return g;
}

// RGB-D depth row r_d = w_depth (depth dm - gt_depth dm), dm = (gt_depth > depth_thr) & (opacity > opa_thr)
__device__ __forceinline__ float depth_residual(const float& depth, const float& gt_depth, const float& dm,
                                                const float& w_depth) {
  return w_depth * (depth * dm - gt_depth * dm);
}

// ... adds its |r| and phi to the sums and returns d/d depth (un-normalised); it does not touch the exposure sums
__device__ __forceinline__ float depth_row(const float& gt_depth, const float& opacity, const float& depth,
                                           const float& depth_thr, const float& opa_thr, const float& w_depth,
                                           const float& delta, const float& p, ObjSums& s) {
  const float dm = (gt_depth > depth_thr && opacity > opa_thr) ? 1.f : 0.f;
  const float rd = depth_residual(depth, gt_depth, dm, w_depth);
  float dh, phi, gam;
  s.l1 += fabsf(rd);
  const float h = huber(rd, delta, dh);
  norm_terms(h, p, phi, gam);
  s.phi += phi;
  return gam * dh * w_depth * dm;
}

}  // namespace mgs
