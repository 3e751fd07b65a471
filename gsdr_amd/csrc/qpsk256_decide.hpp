// gsdr-mi355x: the 256-point demodulation decision, once, for every kernel of qpsk256.hip that decides.
//
// The reference's own rule (qpsk256.cu:171-181), bit for bit -- the first index attaining the minimum of
// cuCabsf(received - point) over all 256 points, strict '<', initialised to +inf (so a NaN/inf symbol maps
// to 0). cuCabsf is CUDA cuComplex.h's scaled hypot (ref_cabsf below), with `1 + t*t` contracted to one fma
// as nvcc does by default. The fast paths rank candidates by the cheaper squared distance
// s_i = fl(fl(dx*dx) + fl(dy*dy)) of the same rounded differences: when the smallest s beats every other
// candidate by a relative margin of 2^-18, which is far wider than the combined rounding of s (2^-23) and
// of cuCabsf (about 4 ulp), the cuCabsf order agrees and that candidate is the reference's answer.
// Otherwise (a near-tie) the candidates are re-ranked with cuCabsf itself in ascending index order. For the
// rectangular grid a received point inside |re|,|im| <= 4|a| can only be won by one of the 3 x 3 grid points
// around its per-axis nearest level (every other point is farther by >= 0.035 a^2); circular tables use
// per-cell candidate lists (qpsk256_tables.hpp); anything else takes the exhaustive cuCabsf search.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qpsk256_tables.hpp"

namespace gsdr {

__device__ __forceinline__ float sqdist(float2 r, float2 c) {
  const float dx = __fsub_rn(r.x, c.x);
  const float dy = __fsub_rn(r.y, c.y);
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

// cuCabsf (CUDA cuComplex.h, called at qpsk256.cu:173, 182): v = max(|a|, |b|), w = min, t = w / v,
// |z| = v * sqrt(fma(t, t, 1)), v + w when v == 0 or either exceeds FLT_MAX. IEEE division and square
// root, as nvcc's defaults (-prec-div, -prec-sqrt) give: '/' and __builtin_sqrtf are correctly rounded
// under HIP's defaults (__fsqrt_rn is not: this toolchain maps it to the ~1-ulp v_sqrt_f32).
__device__ __forceinline__ float ref_cabsf(float re, float im) {
  const float a = fabsf(re), b = fabsf(im);
  const float v = a > b ? a : b;
  const float w = a > b ? b : a;
  float t = __fdiv_rn(w, v);
  t = fmaf(t, t, 1.0f);
  t = __fmul_rn(v, __builtin_sqrtf(t));
  if (v == 0.0f || v > 3.402823466e38f || w > 3.402823466e38f) t = __fadd_rn(v, w);
  return t;
}

// the reference's distance of received point r to table point c (cuCsubf, then cuCabsf)
__device__ __forceinline__ float ref_dist(float2 r, float2 c) { return ref_cabsf(__fsub_rn(r.x, c.x), __fsub_rn(r.y, c.y)); }

// fast-path acceptance: every other candidate's squared distance exceeds s_min by 2^-18 relative
__device__ __forceinline__ float tie_threshold(float smin) { return fmaf(smin, 0x1p-18f, smin); }

// One step of the reference's loop: candidate k at cuCabsf distance d takes over only with strict '<', so
// with candidates offered in ascending index order from best = +inf, idx = 0 the result is the first argmin.
// (The out-of-line searches below declare idx before best: the compiler orders a step's two selects by the
// caller's locals, and that order keeps their code what it was before the step was shared)
__device__ __forceinline__ void rank_step(float d, uint32_t k, float& best, uint32_t& idx) {
  if (d < best) {
    idx = k;
    best = d;
  }
}

__device__ __noinline__ uint32_t demod_exhaustive(const float2* __restrict__ tab, float2 r) {
  uint32_t idx = 0;
  float best = INFINITY;
  for (uint32_t i = 0; i < 256; ++i) rank_step(ref_dist(r, tab[i]), i, best, idx);
  return idx;
}

// ---- rectangular table ----
// Table entry 16 i + q is (lx[i], ly[q]) -- the I coordinate depends on i only and the Q coordinate on q
// only (qpsk256.cu:33-34) -- so every candidate distance is a rounded sum fl(ex[i] + ey[q]) of per-axis
// squares read from level arrays, bit-identical to sqdist() on the table entries. lxp / lyp are the level
// arrays padded with +inf at both ends (entry k + 1 = level k), so neighbours outside [0, 15] have infinite
// distance and never win.
//
// The 3 x 3 neighbourhood of the per-axis nearest levels contains the exhaustive argmin for
// |re|,|im| <= 4|a|. Rounded addition is monotone in each operand, so with a = first argmin of ex and
// b = first argmin of ey the minimum is dmin = fl(ex[a] + ey[b]), and every other candidate is >= the
// second-smallest ex plus ey[b], or >= ex[a] plus the second-smallest ey. When both of those exceed
// dmin by the 2^-18 margin, (a, b) is the reference's answer; otherwise (a near-tie at a decision
// boundary) the 9 candidates are ranked by cuCabsf in ascending index order with strict '<', as the
// reference's exhaustive loop does (no point outside the 3 x 3 can be that close). demod_rect_fast returns
// 256 when the symbol needs the exhaustive search (outside |re|,|im| <= 4|a|, or NaN).
constexpr int kRectLevels = 40;  // floats of LDS: lxp at 0, lyp at kRectLyp (18 used each)
constexpr int kRectLyp = 20;

// The padded level arrays from the rectangular table tsrc, by the workgroup's first 18 threads; the caller's
// barrier publishes them.
__device__ __forceinline__ void rect_fill_levels(float* levp, const float2* tsrc) {
  if (threadIdx.x < 18) {
    const int k = (int)threadIdx.x - 1;
    float* const lxp = levp;
    float* const lyp = levp + kRectLyp;
    lxp[threadIdx.x] = (k < 0 || k > 15) ? INFINITY : tsrc[k * 16].x;
    lyp[threadIdx.x] = (k < 0 || k > 15) ? INFINITY : tsrc[k].y;
  }
}

// scale (levels per unit) and lim (the fast paths' reach) from a = the table's entry 255, x: (15 - 7.5) / 7.5 * a == a
// exactly. The fast paths need a finite, non-zero amplitude: else lim < 0 and every symbol takes the exhaustive
// search, as with the values a kernel starts from, lim = -1, scale = 0.
__device__ __forceinline__ void rect_limits(float a, float& lim, float& scale) {
  scale = 7.5f / a;
  lim = isfinite(scale) ? 4.0f * fabsf(a) : -1.0f;
}

// The near-tie ranking of demod_rect_fast's 3 x 3 candidates by cuCabsf, in ascending index order with
// strict '<' as the reference's loop. Out of line: it runs for a few symbols in a million, and inlined
// into each of a thread's 16 unrolled symbols (nine divisions and square roots each) it made the
// kernel ~60 KB of code.
__device__ __noinline__ uint32_t demod_rect_tie(float dx0, float dx1, float dx2, float dy0, float dy1, float dy2,
                                                int i0, int q0) {
  const float dx[3] = {dx0, dx1, dx2}, dy[3] = {dy0, dy1, dy2};
  uint32_t idx = 0;
  float best = INFINITY;
#pragma unroll
  for (int di = 0; di < 3; ++di) {
#pragma unroll
    for (int dq = 0; dq < 3; ++dq) {
      // out-of-grid neighbours (padded +inf levels) give an infinite difference and never win
      rank_step(ref_cabsf(dx[di], dy[dq]), (uint32_t)((i0 - 1 + di) * 16 + (q0 - 1 + dq)), best, idx);
    }
  }
  return idx;
}

typedef float gsdr_f32x2 __attribute__((ext_vector_type(2)));

// floor(v + 0.5) as an integer in one instruction (v_cvt_rpi_i32_f32); the centre of the 3 x 3 neighbourhood.
// (It differs from rintf only at exact halves, where both nearest levels are in either neighbourhood.)
__device__ __forceinline__ int cvt_rpi(float v) {
  int r;
  asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(v));
  return r;
}

// The three per-axis candidates (levels c - 1, c, c + 1 of the padded array lp): squared differences e0..e2
// (the first two on packed instructions, straight from the two loaded levels), their minimum, median and
// the first index reaching the minimum.
struct AxisCand {
  float d[3], e[3], emin, emed;
  int arg;
};
__device__ __forceinline__ AxisCand axis_cand(const float* __restrict__ lp, float v) {
  AxisCand c;
  const gsdr_f32x2 l01 = gsdr_f32x2{lp[0], lp[1]};
  const gsdr_f32x2 d01 = gsdr_f32x2{v, v} - l01;  // __fsub_rn each: -ffp-contract=off, no fusing
  const float d2 = v - lp[2];
  const gsdr_f32x2 e01 = d01 * d01;
  c.d[0] = d01.x;
  c.d[1] = d01.y;
  c.d[2] = d2;
  c.e[0] = e01.x;
  c.e[1] = e01.y;
  c.e[2] = d2 * d2;
  c.emin = fminf(fminf(c.e[0], c.e[1]), c.e[2]);
  c.emed = __builtin_amdgcn_fmed3f(c.e[0], c.e[1], c.e[2]);
  c.arg = c.e[0] == c.emin ? 0 : (c.e[1] == c.emin ? 1 : 2);
  return c;
}

__device__ __forceinline__ uint32_t demod_rect_fast(const float* __restrict__ lxp, const float* __restrict__ lyp, float2 r,
                                                    float lim, float scale) {
  if (!(fabsf(r.x) <= lim && fabsf(r.y) <= lim)) return 256u;
  // level i sits at (i - 7.5) / 7.5 * a  =>  i ~= v * (7.5 / a) + 7.5 (both axes in one packed fma)
  const gsdr_f32x2 u =
      __builtin_elementwise_fma(gsdr_f32x2{r.x, r.y}, gsdr_f32x2{scale, scale}, gsdr_f32x2{7.5f, 7.5f});
  const int i0 = min(max(cvt_rpi(u.x), 0), 15);
  const int q0 = min(max(cvt_rpi(u.y), 0), 15);
  const AxisCand cx = axis_cand(lxp + i0, r.x), cy = axis_cand(lyp + q0, r.y);
  const float thr = tie_threshold(__fadd_rn(cx.emin, cy.emin));
  if (__fadd_rn(cx.emed, cy.emin) > thr && __fadd_rn(cx.emin, cy.emed) > thr) {
    return (uint32_t)((i0 - 1 + cx.arg) * 16 + (q0 - 1 + cy.arg));
  }
  return demod_rect_tie(cx.d[0], cx.d[1], cx.d[2], cy.d[0], cy.d[1], cy.d[2], i0, q0);
}

// Rectangular decision in ~15 VALU operations, taken when it is provably the reference's answer. u is the symbol's
// position in level units per axis (level k at u = k up to rounding: < 2^-17 of a level spacing, from scale, the
// fma and the host-built levels). When the clamped u of both axes is more than kRectMargin from every midpoint
// between two levels, the nearest level is unambiguous by a margin (in squared distance the runner-up is farther by
// >= 2^-11 of dmin) that no rounding of the reference's cuCabsf ranking can reverse, so (i, q) is its first argmin.
// Symbols within the margin of a midpoint (~1e-4 of noisy symbols) or beyond |re|,|im| <= 4|a| (or NaN) return
// false and take demod_rect_fast's careful path.
constexpr float kRectMargin = 0x1p-10f;
__device__ __forceinline__ bool demod_rect_quick(float2 r, float lim, float scale, uint32_t& k) {
  const gsdr_f32x2 u = __builtin_elementwise_fma(gsdr_f32x2{r.x, r.y}, gsdr_f32x2{scale, scale}, gsdr_f32x2{7.5f, 7.5f});
  const float tx = __builtin_amdgcn_fmed3f(u.x, 0.0f, 15.0f), ty = __builtin_amdgcn_fmed3f(u.y, 0.0f, 15.0f);
  const float ix = __builtin_rintf(tx), iy = __builtin_rintf(ty);
  const gsdr_f32x2 d = gsdr_f32x2{tx, ty} - gsdr_f32x2{ix, iy};
  k = (uint32_t)ix * 16u + (uint32_t)iy;
  return fabsf(r.x) <= lim && fabsf(r.y) <= lim && fmaxf(fabsf(d.x), fabsf(d.y)) <= 0.5f - kRectMargin;
}

// ---- circular table ----
// cword, clists, cR, inv_cs: the LDS image of CircCells (cR == 0: no lookup).
// The cell word of r's cell; false off the grid (or NaN, or no lookup).
__device__ __forceinline__ bool circ_cell(const uint16_t* cword, float cR, float inv_cs, float2 r, uint32_t& wc) {
  const float fx = (r.x + cR) * inv_cs, fy = (r.y + cR) * inv_cs;
  if (!(cR > 0.0f && fx >= 0.0f && fy >= 0.0f && fx < (float)kCellGrid && fy < (float)kCellGrid)) return false;
  wc = cword[(int)fy * kCellGrid + (int)fx];
  return true;
}

// The decision of r from its cell word wc (circ_cell).
__device__ __forceinline__ uint32_t circ_decide(const uint8_t* clists, const float2* tab, float2 r, uint32_t wc) {
  const uint32_t len = wc >> 12;
  if (len == 1u) return wc & 0xfffu;  // a one-point cell: no distance needed
  const uint32_t b = wc & 0xfffu, e = b + len;
  float best = INFINITY, second = INFINITY;
  uint32_t idx = 0;
  // four candidates per step with independent LDS loads; slots past the list end repeat its
  // last entry (a duplicate of an entry already ranked: skipped for the runner-up)
  for (uint32_t m = b; m < e; m += 4) {
    uint32_t k[4];
    float2 pt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = clists[m + j < e ? m + j : e - 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) pt[j] = tab[k[j]];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (j == 0 || m + j < e) ? sqdist(r, pt[j]) : INFINITY;
      if (d < best) {
        second = best;
        best = d;
        idx = k[j];
      } else if (d < second) {
        second = d;
      }
    }
  }
  if (second > tie_threshold(best)) return idx;
  // near-tie: the list (ascending indices, every point that can win in the cell) ranked by
  // cuCabsf with strict '<', as the reference's loop
  best = INFINITY;
  idx = 0;
  for (uint32_t m = b; m < e; ++m) {
    const uint32_t k = clists[m];
    rank_step(ref_dist(r, tab[k]), k, best, idx);
  }
  return idx;
}

}  // namespace gsdr
