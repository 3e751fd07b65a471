// gsdr-mi355x, FIR engine: the kernels' launch parameters, the exact-phase NCO and the mixers a tile's staging applies.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fir_samples.hpp"
#include "stream_step.hpp"

namespace gsdr {

// ------------------------------------------------------------------------------------------------
// Launch parameters (one struct for every mode; passed by value)
// ------------------------------------------------------------------------------------------------
// (enum Mode { kModeFir, kModeFm, kModeAm, kModeIq }: stream_step.hpp)
struct FirParams {
  const void* in;
  const void* taps;
  void* out;
  uint64_t L;            // input samples readable
  uint64_t N;            // outputs to write
  uint32_t T;            // tap count (>= 1)
  uint32_t nch;          // tap chunks per phase column
  uint32_t tile_stride;  // outputs advanced per tile (KT, or KT - 1 for the FM discriminator)
  uint32_t D;            // decimation (used by the generic kernel)
  uint32_t nco_inc;      // NCO phase increment per sample, 2^-32 cycles
  uint32_t nco_n0;       // low 32 bits of firstSampleIndex
  float fm_gain;         // FM discriminator gain
  uint32_t out_phase;    // absolute index of output 0 mod 16 (the int8 matrix-core kernels' block grid)
  // Anchored chains (the polyphase kernels in FM / AM / IQ mode, MixAnchored below): tile t covers outputs
  // [t KT - tile_shift, (t + 1) KT - tile_shift) of the call, and tile 0 is sub-tile cell_sub0 of its NCO cell.
  uint32_t tile_shift;
  uint32_t cell_sub0;
  // The streaming object's one-launch path (stream.hip): output 0's window starts at sample in_off of the
  // caller's chunk; chunk samples at negative offsets i >= -hist_len come from hist[hist_len + i] (the
  // stream's history), and samples [hist_from, hist_from + hist_n) (same offsets) are copied to hist_out
  // (the next history) by workgroup 0. The int8 matrix-core kernels (fir_i8_mfma.hpp) take `in` = the
  // chunk and L = its length; the tiled kernels below take `in` = chunk + in_off (output 0's window, so
  // the tile arithmetic is unchanged; the pointer may precede the chunk, and samples before it are read
  // only through the history) and L = samples readable from there.
  int64_t in_off;
  const void* hist;
  uint64_t hist_len;
  void* hist_out;
  int64_t hist_from;
  uint64_t hist_n;
};

// ------------------------------------------------------------------------------------------------
// NCO: exact integer phase P(n) = n * inc mod 2^32 from the absolute sample
// index n, turned into a unit phasor by a fixed function of n alone, so any split of a stream into
// calls (and any tiling inside a call) mixes every sample with bit-identical values:
//   n even: (cos, sin)(2 pi P(n) / 2^32) from the hardware v_cos_f32 / v_sin_f32, whose argument is
//           in revolutions (max abs error 1.9e-7 measured over 2^28 phases, tools/nco_accuracy.hip;
//           the (int32)P -> float rounding adds <= 2^-25 revolutions, as sincospif did);
//   n odd:  phasor(n - 1) rotated by w = phasor of one step (P = inc).
// One transcendental pair per two samples: the mixer was a third of the FM chain's VALU work with
// a sincospif per sample.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 nco_direct(uint32_t phase) {
  const float r = (float)(int32_t)phase * 0x1p-32f;  // revolutions in [-0.5, 0.5)
  return make_float2(__builtin_amdgcn_cosf(r), __builtin_amdgcn_sinf(r));
}

// a * b with explicit fmas: (fma(a.x, b.x, -(a.y b.y)), fma(a.x, b.y, a.y b.x)). Written on
// two-lane vectors so it is one v_pk_mul_f32 (a.y * (-b.y, b.x)) and one v_pk_fma_f32 (a.x * b + that), plus the
// swapped, negated b (one more v_pk_mul_f32 by (1, -1), hoisted when b is a loop constant); the library builds with
// -ffp-contract=off, so the rounding is fixed here rather than left to the contraction pass. (Round 6 tried the
// sign as a neg_lo source modifier of the v_pk_mul_f32, written as inline asm -- the compiler never forms it for
// packed F32 -- which saves that instruction for every product whose b varies, e.g. each staged granule's NCO mix.
// An isolated check agreed bit for bit on 2^22 products, but inside the chain kernels the results were wrong (109
// GPU tests failed), so it is not used.)
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  const gsdr_f32x2 bv = gsdr_f32x2{b.x, b.y};
  // (-b.y, b.x) as b swapped times (-1, 1) (exact): one v_pk_mul_f32, where building it with a sign flip
  // and a move took two instructions
  const gsdr_f32x2 t = gsdr_f32x2{a.y, a.y} * (bv.yx * gsdr_f32x2{-1.0f, 1.0f});
  const gsdr_f32x2 r = __builtin_elementwise_fma(gsdr_f32x2{a.x, a.x}, bv, t);
  return make_float2(r.x, r.y);
}

// phasor of absolute sample n (low 32 bits suffice: P is taken mod 2^32)
__device__ __forceinline__ float2 nco_phasor(uint32_t n, uint32_t inc) {
  const float2 w = nco_direct(inc);
  const float2 e = nco_direct((n & ~1u) * inc);
  return (n & 1u) ? cmul(e, w) : e;
}

__device__ __forceinline__ float2 nco_mix(float2 x, uint32_t n, uint32_t inc) { return cmul(x, nco_phasor(n, inc)); }

// NCO mixing of one granule (two complex samples n, n + 1) given ph = n * inc mod 2^32, the phase of
// its first sample; `odd` = n & 1 (wave-uniform in the tiled kernels: they stage granules at even
// offsets from the tile start). The phasor is a pure function of the absolute index: even n from
// nco_direct, odd n = phasor(n - 1) * w, w = nco_direct(inc).
template <class InT, int MODE>
__device__ __forceinline__ float4 stage_transform_ph(float4 v, uint32_t ph, bool odd, uint32_t inc) {
  if constexpr (MODE != kModeFir) {
    static_assert(SampleT<InT>::kPerGranule == 2, "NCO modes take complex input");
    const float2 w = nco_direct(inc);
    float2 ea, eb;
    if (odd) {
      ea = cmul(nco_direct(ph - inc), w);
      eb = nco_direct(ph + inc);
    } else {
      ea = nco_direct(ph);
      eb = cmul(ea, w);
    }
    const float2 a = cmul(make_float2(v.x, v.y), ea);
    const float2 b = cmul(make_float2(v.z, v.w), eb);
    v = make_float4(a.x, a.y, b.x, b.y);
  }
  return v;
}

// s = local sample index of a granule's first sample (only its low 32 bits matter: the NCO phase is
// taken mod 2^32).
template <class InT, int MODE>
__device__ __forceinline__ float4 stage_transform(float4 v, uint32_t s, const FirParams& p) {
  if constexpr (MODE != kModeFir) {
    const uint32_t n = p.nco_n0 + s;  // absolute index of the granule's first sample mod 2^32
    return stage_transform_ph<InT, MODE>(v, n * p.nco_inc, __builtin_amdgcn_readfirstlane(n & 1u) != 0, p.nco_inc);
  }
  return v;
}

// Phase walk of a thread's tile-body granules: granule g = k * WG + tid of a tile starting at S0 has
// phase ph0 + k * step (mod 2^32) -- the same integer as (n0 + S0 + g * G) * inc, so the phasors
// are unchanged, without a 32-bit integer multiply (a quarter-rate instruction) per granule.
struct PhaseWalk {
  uint32_t ph0, step, inc;
  bool odd;
};

template <int G, int WG>
__device__ __forceinline__ PhaseWalk phase_walk(uint32_t n0, uint64_t S0, uint32_t inc) {
  const uint32_t n = n0 + (uint32_t)S0 + (uint32_t)(threadIdx.x * G);
  return PhaseWalk{n * inc, (uint32_t)(WG * G) * inc, inc, __builtin_amdgcn_readfirstlane(n & 1u) != 0};
}

// ------------------------------------------------------------------------------------------------
// Staging mixers: what stage_tile does to a granule between its load and its LDS store. A thread's tile granules
// are g = k WG + tid, row k = 0, 1, ...; stage_tile hands each of them to its mixer once, in ascending row order:
//   row(v, k, odd)     granule of body row k (k and the NCO start parity `odd`, see per_parity, are compile-time
//                      constants after unrolling);
//   shifted_row(v, k, prev)  body row k of the shifted path: the loaded pair (sample 2g - 1, sample 2g); `prev`,
//                      from begin_shifted(), is what the mixer keeps for sample 2g - 1 and lives in that path only;
//   next(v, s, advance)  the thread's next granule (the halo; every granule of a history tile, whose first row
//                      passes advance = false); s = the local index of its first sample. After shifted_halo(prev)
//                      these granules are those one granule before the rows' pairs (g = k WG + tid - 1).
// A mixer holds phasor state only. Every path must form the same phasor for the same sample: that is what makes any
// split of a stream into calls bit-identical.
// ------------------------------------------------------------------------------------------------
// FIR mode (and the probes' staging without the mix): the identity
struct MixNone {
  template <class F>
  __device__ __forceinline__ void per_parity(F&& body) {
    body(std::false_type{});
  }
  template <class ODD>
  __device__ __forceinline__ float4 row(float4 v, int, ODD) {
    return v;
  }
  struct Prev {};
  __device__ __forceinline__ Prev begin_shifted() { return {}; }
  __device__ __forceinline__ float4 shifted_row(float4 v, int, Prev&) { return v; }
  __device__ __forceinline__ void shifted_halo(const Prev&) {}
  __device__ __forceinline__ float4 next(float4 v, uint64_t, bool = true) { return v; }
};

// The absolute phasor (k_fir_contig's chains): a pure function of the absolute sample index, so any way of arriving
// at the same integer phase gives the same bits. The body rows walk the phase (PhaseWalk); the rest multiply.
template <class InT, int MODE, int WG>
struct MixAbsolute {
  const FirParams& p;
  PhaseWalk pw;
  __device__ __forceinline__ MixAbsolute(const FirParams& p_, uint64_t S0)
      : p(p_), pw(phase_walk<SampleT<InT>::kPerGranule, WG>(p_.nco_n0, S0, p_.nco_inc)) {}
  // The body loop is instantiated once per NCO start parity (`odd` is uniform over the tile): with the parity a
  // runtime value the compiler kept a branch around every granule's phasor.
  template <class F>
  __device__ __forceinline__ void per_parity(F&& body) {
    if (pw.odd) {
      body(std::true_type{});
    } else {
      body(std::false_type{});
    }
  }
  template <class ODD>
  __device__ __forceinline__ float4 row(float4 v, int k, ODD) {
    return stage_transform_ph<InT, MODE>(v, pw.ph0 + (uint32_t)k * pw.step, ODD::value, pw.inc);
  }
  struct Prev {};
  __device__ __forceinline__ Prev begin_shifted() { return {}; }
  // samples S0 + 2g - 1 (odd start relative to the tile) and S0 + 2g: the odd-start pairs mix exactly as the
  // even-start ones would
  __device__ __forceinline__ float4 shifted_row(float4 v, int k, Prev&) {
    return stage_transform_ph<InT, MODE>(v, pw.ph0 + (uint32_t)k * pw.step - pw.inc, !pw.odd, pw.inc);
  }
  __device__ __forceinline__ void shifted_halo(const Prev&) {}
  __device__ __forceinline__ float4 next(float4 v, uint64_t s, bool = true) {
    return stage_transform<InT, MODE>(v, (uint32_t)s, p);
  }
};

// ------------------------------------------------------------------------------------------------
// Anchored NCO (the polyphase kernels in FM / AM mode). The FM discriminator and the AM envelope are
// invariant to a rotation common to the FIR outputs they combine, so a tile need not mix with the absolute
// phasor e^(j 2 pi P(n) / 2^32): it may mix relative to an anchor sample, as long as every output and its
// discriminator partner share the anchor. The anchors form an absolute grid: output q (absolute index
// q = firstSampleIndex / D + m) belongs to cell q / CELL (CELL = the decimation's largest tile, 1,024 outputs
// at D = 4), and all of a cell's FIR outputs -- in FM mode also the first output of the next cell, which the
// cell's last discriminator pairs with -- come from samples mixed relative to the cell's first sample.
// Within a cell, granule (row k, lane l) (samples 2 (k WG + l) and 2 (k WG + l) + 1 after the anchor) takes the
// phasors e_k(l) and e_k(l) w, with e_0(l) = E(2 l), e_k(l) = e_(k-1)(l) F, F = E(2 WG), w = E(1) (E: the exact
// integer phase through v_cos / v_sin, nco_direct): one complex multiply a granule instead of the absolute
// scheme's transcendental pair, and every phasor a fixed sequence of operations on (l, k) alone. The
// short-call tiles are sub-tiles of a cell that start their chains at row r0 by r0 multiplies, and every
// staging path (aligned, shifted, streaming) forms the same values, so every tile shape and any split of a
// stream into calls give bit-identical outputs. (IQ mode, whose complex output does see the
// rotation, undoes it per cell in the epilogue: anchor_rotate below.)
// ------------------------------------------------------------------------------------------------
template <int WG>
__device__ __forceinline__ float2 rel_chain_start(uint32_t lane, uint32_t rows, uint32_t inc) {
  const float2 F = nco_direct((uint32_t)(2 * WG) * inc);
  float2 e = nco_direct((2u * lane) * inc);
  for (uint32_t i = 0; i < rows; ++i) e = cmul(e, F);
  return e;
}

// a granule (two complex samples) mixed with (e, e w)
__device__ __forceinline__ float4 rel_mix(float4 v, float2 e, float2 w) {
  const float2 eb = cmul(e, w);
  const float2 a = cmul(make_float2(v.x, v.y), e);
  const float2 b = cmul(make_float2(v.z, v.w), eb);
  return make_float4(a.x, a.y, b.x, b.y);
}

// The tile starts row0 WG - sh granules into its cell (0 <= sh < WG): tile granule g = k WG + tid (the staging map
// of stage_tile) is cell granule (row0 + k) WG + tid - sh, i.e. lane l = (tid - sh) mod WG of cell row r + k with
// r = row0, or row0 - 1 for tid < sh. So a thread walks lane l's chain from row r, one multiply a row, made when the
// row is mixed (none for the tile's first row). The sequence of multiplies per (lane, row) is the contract.
template <int WG>
struct MixAnchored {
  uint32_t inc, lane, crow;  // the chain: cell lane, and the cell row of tile row 0
  float2 w, F, e;
  __device__ __forceinline__ MixAnchored(uint32_t inc_, uint32_t row0, uint32_t sh)
      : inc(inc_), lane((threadIdx.x + WG - sh) % WG), crow(row0 - (threadIdx.x < sh ? 1u : 0u)) {
    w = nco_direct(inc);
    F = nco_direct((uint32_t)(2 * WG) * inc);
    e = rel_chain_start<WG>(lane, crow, inc);
  }
  template <class F_>
  __device__ __forceinline__ void per_parity(F_&& body) {
    body(std::false_type{});
  }
  __device__ __forceinline__ float4 next(float4 v, uint64_t, bool advance = true) {
    if (advance) e = cmul(e, F);
    return rel_mix(v, e, w);
  }
  template <class ODD>
  __device__ __forceinline__ float4 row(float4 v, int k, ODD) {
    return next(v, 0, k > 0);
  }
  // loaded pair g holds samples 2g - 1 (the odd half of granule g - 1: lane l - 1's chain, or for lane 0
  // lane WG - 1's chain one row behind) and 2g (granule g): the previous lane's chain `ep` runs beside this one
  struct Prev {
    float2 ep;
    bool lag;  // lane 0 of a cell's first row has no previous granule in the cell
  };
  __device__ __forceinline__ Prev begin_shifted() {
    const uint32_t lp = (lane + WG - 1) % WG;
    Prev q{nco_direct((2u * lp) * inc), lane == 0 && crow == 0};
    for (uint32_t i = 0; i < crow; ++i) {
      const float2 t = cmul(q.ep, F);
      q.ep = (lane == 0 && i == 0) ? q.ep : t;  // lane 0 follows lane WG - 1 one row behind
    }
    return q;
  }
  __device__ __forceinline__ float4 shifted_row(float4 v, int k, Prev& q) {
    if (k > 0) {
      e = cmul(e, F);
      const float2 t = cmul(q.ep, F);
      q.ep = (k == 1 && q.lag) ? q.ep : t;
    }
    const float2 a = cmul(make_float2(v.x, v.y), cmul(q.ep, w));  // sample 2g - 1
    const float2 b = cmul(make_float2(v.z, v.w), e);            // sample 2g
    return make_float4(a.x, a.y, b.x, b.y);
  }
  // the shifted halo's granule g is lane l - 1's (lane 0: lane WG - 1's, one row back), i.e. the previous-lane
  // chain's
  __device__ __forceinline__ void shifted_halo(const Prev& q) { e = q.ep; }
};

// A complex output (kModeIq) is not invariant to the anchor: a cell's FIR outputs, accumulated from samples mixed
// relative to the cell's first sample, are the absolute-phase outputs times conj(A), A = the absolute phasor of that
// sample, so the epilogue multiplies each by A. cell_out0 = the call-local index of the cell's first output (low 32
// bits; below zero, wrapped, for a call that starts inside a cell): its first sample is absolute sample
// n_anchor = nco_n0 + cell_out0 D mod 2^32 -- the same integer from whichever call, tile shape or sub-tile reaches
// the cell -- and A = nco_direct(n_anchor inc) a function of it alone, applied by one cmul(acc, A) per output. The
// rotated outputs therefore keep the anchored accumulators' property: the same bits for the same absolute output.
template <int R>
__device__ __forceinline__ void anchor_rotate(const FirParams& p, uint32_t cell_out0, uint32_t D, float2 (&acc)[R]) {
  const uint32_t n_anchor = p.nco_n0 + cell_out0 * D;
  const float2 A = nco_direct(n_anchor * p.nco_inc);
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = cmul(acc[r], A);
}

}  // namespace gsdr
