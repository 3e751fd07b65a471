// gsdr-mi355x: the demodulator epilogue maths (FM discriminator, AM envelope) of fir_engine.hpp and quad_demod.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "fir_samples.hpp"

namespace gsdr {

// FM discriminator of consecutive FIR outputs: g * arg(y1 * conj(y0)) (reference src/fm.cu:66-68,
// src/quad_demod.cu:30-31).
// atan2 for the discriminators: octant reduction t = min/max (v_rcp_f32), an odd minimax polynomial
// for atan on [0, 1] (max abs error 3.3e-7 rad in float32 evaluation, tools/atan_fit.py), then the
// octant fix-ups. Outside 2^-100 < |x| + |y| < 2^100 (zeros, infinities, NaN, and magnitudes where
// v_rcp_f32 would leave the normal range) the library atan2f is used, so its special values
// (atan2(0, 0) = 0, atan2(+-0, -0) = +-pi, ...) are unchanged. The discriminator bar is 3.1e-5 rad
// (1e-5 of pi; tests/helpers.py wrapped_angle_err).
// The scalar form (disc_atan2 / fm_disc) and the two-at-a-time form (fm_disc2, packed FMAs) run the
// same IEEE operations in the same order, so every kernel's discriminator outputs are bit-identical.
__device__ __forceinline__ bool disc_fast(float y, float x) {
  const float s = fabsf(x) + fabsf(y);
  return s > 0x1p-100f && s < 0x1p100f;
}

__device__ __forceinline__ gsdr_f32x2 atan_poly2(gsdr_f32x2 t) {
  const gsdr_f32x2 s = t * t;
  gsdr_f32x2 p = __builtin_elementwise_fma(gsdr_f32x2{0.006811787374317646f, 0.006811787374317646f}, s,
                                           gsdr_f32x2{-0.0336042121052742f, -0.0336042121052742f});
  p = __builtin_elementwise_fma(p, s, gsdr_f32x2{0.07962368428707123f, 0.07962368428707123f});
  p = __builtin_elementwise_fma(p, s, gsdr_f32x2{-0.132333442568779f, -0.132333442568779f});
  p = __builtin_elementwise_fma(p, s, gsdr_f32x2{0.19807817041873932f, 0.19807817041873932f});
  p = __builtin_elementwise_fma(p, s, gsdr_f32x2{-0.3331736922264099f, -0.3331736922264099f});
  p = __builtin_elementwise_fma(p, s, gsdr_f32x2{0.9999961256980896f, 0.9999961256980896f});
  return p * t;
}

// octant fix-ups of the polynomial result r = atan(min/max) for (y, x)
__device__ __forceinline__ float disc_octant(float r, float y, float x) {
  if (fabsf(y) > fabsf(x)) r = 1.57079637f - r;
  if (x < 0.0f) r = 3.14159274f - r;
  return copysignf(r, y);
}

__device__ __forceinline__ float disc_atan2(float y, float x) {
  if (!disc_fast(y, x)) return atan2f(y, x);
  const float ax = fabsf(x), ay = fabsf(y);
  const float t = fminf(ax, ay) * __builtin_amdgcn_rcpf(fmaxf(ax, ay));
  return disc_octant(atan_poly2(gsdr_f32x2{t, t}).x, y, x);
}

__device__ __forceinline__ float2 disc_product(float2 y0, float2 y1) {
  return make_float2(y1.x * y0.x + y1.y * y0.y, y1.y * y0.x - y1.x * y0.y);
}

__device__ __forceinline__ float fm_disc(float2 y0, float2 y1, float g) {
  const float2 z = disc_product(y0, y1);
  return g * disc_atan2(z.y, z.x);
}

// fm_disc(a0, a1) and fm_disc(b0, b1) with the polynomial, the fix-up subtractions and the gain on
// packed FMAs / multiplies (two outputs per instruction)
// arg(za), arg(zb) of two discriminator products on packed FMAs (disc_atan2's operations)
__device__ __forceinline__ gsdr_f32x2 disc_angle2(float2 za, float2 zb) {
  const float axa = fabsf(za.x), aya = fabsf(za.y), axb = fabsf(zb.x), ayb = fabsf(zb.y);
  const gsdr_f32x2 t = gsdr_f32x2{fminf(axa, aya), fminf(axb, ayb)} *
                       gsdr_f32x2{__builtin_amdgcn_rcpf(fmaxf(axa, aya)), __builtin_amdgcn_rcpf(fmaxf(axb, ayb))};
  gsdr_f32x2 r = atan_poly2(t);
  const gsdr_f32x2 q = gsdr_f32x2{1.57079637f, 1.57079637f} - r;
  r.x = aya > axa ? q.x : r.x;
  r.y = ayb > axb ? q.y : r.y;
  const gsdr_f32x2 h = gsdr_f32x2{3.14159274f, 3.14159274f} - r;
  r.x = za.x < 0.0f ? h.x : r.x;
  r.y = zb.x < 0.0f ? h.y : r.y;
  r = gsdr_f32x2{copysignf(r.x, za.y), copysignf(r.y, zb.y)};
  if (!disc_fast(za.y, za.x)) r.x = atan2f(za.y, za.x);
  if (!disc_fast(zb.y, zb.x)) r.y = atan2f(zb.y, zb.x);
  return r;
}

__device__ __forceinline__ gsdr_f32x2 fm_disc2(float2 a0, float2 a1, float2 b0, float2 b1, float g) {
  return gsdr_f32x2{g, g} * disc_angle2(disc_product(a0, a1), disc_product(b0, b1));
}

// AM envelope: 2 * saturate(|y|) - 1, saturate(NaN) = 0 (reference src/am.cu:49, quad_demod.cu:47-48).
// |y| as the hardware square root of x^2 + y^2 (within 1 ulp of hypotf, whose library form rescales through a
// double frexp / ldexp: ~14 instructions an output against ~8). The saturation makes the rescaling moot: a sum
// that overflows gives +inf where hypotf gives a finite value > 1 (both saturate to 1), one that underflows gives 0
// where hypotf gives a value below 2^-24 (both give -1); an infinite component gives +inf even beside a NaN, as
// hypotf does.
__device__ __forceinline__ float am_env(float2 y) {
  float m = __builtin_amdgcn_sqrtf(fmaf(y.x, y.x, y.y * y.y));
  if (__builtin_isinf(y.x) || __builtin_isinf(y.y)) m = __builtin_inff();
  m = (m > 0.0f) ? (m < 1.0f ? m : 1.0f) : 0.0f;
  return 2.0f * m - 1.0f;
}

}  // namespace gsdr
