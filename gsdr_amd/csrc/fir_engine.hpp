// gsdr-mi355x: the decimating-FIR engine behind gsdrFir*, gsdrFmDemod and gsdrAmDemod.
//
// What it computes (reference src/fir.cu:26-71):
//     y[k] = sum_{i<T} x[k*D + i] * t[i]
// optionally with an NCO mix applied to x first (reference src/adjustFrequency.cu:25-56, re-specified in
// SURVEY.md App. A.3) and a demodulator epilogue (FM: reference src/fm.cu:59-68, AM: src/am.cu:49).
//
// How (MI355X / gfx950, wave64, 160 KiB LDS per CU):
//   * One workgroup owns a tile of KT = WG * R consecutive outputs. It stages the tile's input span
//     (KT*D + taps samples) from HBM into LDS with 16-byte loads (one "granule" = 2 complex or 4 real
//     samples); the NCO mix, when present, is applied once per staged sample on the way in.
//   * Each thread then computes R consecutive outputs from a register-resident sliding window read out
//     of LDS with ds_read_b128, so each staged sample is read from LDS ~(R+JC-1)/R times instead of
//     T/D times. Taps are wave-uniform: they are read with scalar loads straight into SGPR operands of
//     the FMAs (no VGPRs, no LDS traffic for taps).
//   * Decimation D that is a multiple of the granule width is handled polyphase: a granule holds G
//     consecutive phases of one input "row" (D samples), and the window for one granule column only
//     carries the phases that meet the taps t[j*D + h*G + e] in flight -- no wasted window registers.
//   * A thread's segment is SG granules; when SG is even a one-granule pad is inserted after each
//     segment so the per-lane stride is odd and the 16-lane groups of ds_read_b128 are bank-conflict
//     free, while every window offset stays a compile-time constant.
//   * Input may also be interleaved int8 I/Q (Iq8): converted to float as it is staged, so the float
//     samples exist only in LDS. HBM loads and FIR stores are non-temporal (streamed once).
//   * The default core is packed VALU. An exact-f32 matrix-core core (k_fir_mfma_bc, 4x4x1 outer
//     products with broadcast taps, bit-identical to the oracle) exists as a variant; it runs at a
//     higher clock under the cap but needs more cycles and more energy per launch (4 % slower). The
//     kernel is bound by the part's 1400 W power cap with staging and MACs together.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "fir_demod.hpp"
#include "fir_nco.hpp"
#include "fir_samples.hpp"
#include "fir_staging.hpp"
#include "stream_step.hpp"

namespace gsdr {

// Taps are fetched with scalar buffer loads (s_buffer_load_dword{,x2,x4,x8}) through a buffer
// descriptor whose range is exactly the caller's T taps: the hardware range check returns 0 for the
// zero-padding past T, so no clamp/select instructions are needed and the tap lands directly in the
// SGPR operand of v_pk_fma_f32 (broadcast with op_sel_hi).
typedef int gsdr_v4i32 __attribute__((ext_vector_type(4)));
__device__ float gsdr_s_buffer_load_f32(gsdr_v4i32 rsrc, int offset, int aux) __asm("llvm.amdgcn.s.buffer.load.f32");

struct TapBuf {
  gsdr_v4i32 rsrc;
};

// A window of the tap array starting at tap `base` (wave-uniform): the descriptor is re-based so
// every tap inside the window is an immediate offset. Read tap by tap (tap_at), neighbouring taps merge into
// s_buffer_load_dwordx2/x4/x8, in batches the compiler sizes and each ends with a full lgkmcnt(0) drain (the
// polyphase core read a column's 32 taps as eight batches of four dwordx2); TapChunk below reads a whole chunk.
template <class TapT>
__device__ __forceinline__ TapBuf tap_window(const void* taps, uint32_t T, uint32_t base) {
  const uint64_t a = reinterpret_cast<uint64_t>(reinterpret_cast<const TapT*>(taps) + base);
  const uint32_t bytes = base < T ? (T - base) * (uint32_t)sizeof(TapT) : 0u;
  TapBuf b;
  b.rsrc = gsdr_v4i32{(int)(uint32_t)a, (int)(uint32_t)(a >> 32) & 0xffff, (int)bytes, 0x00020000};
  return b;
}

// Tap `i` (a compile-time constant after unrolling) of a window; past T it reads as zero.
template <class TapT>
__device__ __forceinline__ TapT tap_at(const TapBuf& tb, int i);
template <>
__device__ __forceinline__ float tap_at<float>(const TapBuf& tb, int i) {
  return gsdr_s_buffer_load_f32(tb.rsrc, i * 4, 0);
}
template <>
__device__ __forceinline__ float2 tap_at<float2>(const TapBuf& tb, int i) {
  return make_float2(gsdr_s_buffer_load_f32(tb.rsrc, i * 8, 0), gsdr_s_buffer_load_f32(tb.rsrc, i * 8 + 4, 0));
}

// A whole tap chunk at once (the polyphase core): the chunk's taps are contiguous, so they are fetched as
// s_buffer_load_dwordx16 (the widest form; merged single loads stop at x8) into NQ * 16 SGPRs and waited for ONCE,
// before the chunk's first window read. Scalar loads return out of order and share their counter with LDS, so a wait
// for a tap is always a full drain of that counter: with the taps settled up front, every later wait of the chunk
// is a counted one on the in-order LDS reads alone.
typedef float gsdr_f32x16 __attribute__((ext_vector_type(16)));
__device__ gsdr_f32x16 gsdr_s_buffer_load_f32x16(gsdr_v4i32 rsrc, int offset, int aux) __asm(
    "llvm.amdgcn.s.buffer.load.v16f32");

template <int NQ>
struct TapChunk {
  gsdr_f32x16 q[NQ];
  __device__ __forceinline__ void load(const TapBuf& tb) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) q[i] = gsdr_s_buffer_load_f32x16(tb.rsrc, i * 64, 0);
  }
  // The taps are "used" here, so the one wait for them lands here; no LDS read moves above it.
  __device__ __forceinline__ void settle() {
#pragma unroll
    for (int i = 0; i < NQ; ++i) asm volatile("" : "+s"(q[i])::"memory");
  }
  // tap `i` of the chunk (a compile-time constant after unrolling)
  template <class TapT>
  __device__ __forceinline__ TapT at(int i) const {
    if constexpr (std::is_same<TapT, float>::value) {
      return q[i / 16][i % 16];
    } else {
      return make_float2(q[(2 * i) / 16][(2 * i) % 16], q[(2 * i + 1) / 16][(2 * i + 1) % 16]);
    }
  }
  // Real taps `i` (even) and `i + 1` as the even-aligned SGPR pair they were loaded into. v_pk_fma_f32 broadcasts
  // either half of a 64-bit scalar operand (op_sel / op_sel_hi), and the compiler selects the high half when the tap is
  // element 1 of a two-element vector; read as element 2k + 1 of the sixteen it copied every odd tap to an even SGPR
  // first (s_mov_b32, one per odd tap and use). The empty asm (no instruction, not volatile, the pair its only operand)
  // keeps the pair a value of its own, so the element-of-sixteen form is not folded back in.
  __device__ __forceinline__ gsdr_f32x2 pair(int i) const {
    gsdr_f32x2 t = {q[i / 16][i % 16], q[i / 16][i % 16 + 1]};
    asm("" : "+s"(t));
    return t;
  }
};
// dwords of a chunk of `taps` taps, and whether it is fetched whole (1, 2 or 4 x16 loads: up to 64 SGPRs)
template <class TapT>
constexpr int tap_chunk_dwords(int taps) {
  return taps * (int)(sizeof(TapT) / 4);
}
constexpr bool tap_chunk_whole(int dwords) { return dwords == 16 || dwords == 32 || dwords == 64; }

// ------------------------------------------------------------------------------------------------
// Epilogues
// ------------------------------------------------------------------------------------------------
template <class OutT, int R, bool NTS = false>
__device__ __forceinline__ void store_fir(OutT* __restrict__ out, uint64_t k0, uint64_t N, const OutT (&acc)[R]) {
  constexpr int PER16 = 16 / sizeof(OutT);
  // 16-byte stores when R fills them (a thread's outputs are contiguous), else one output at a time.
  // (k0 < N first: an anchored tile's leading outputs (kModeIq) have k0 wrapped below zero, and k0 + R would wrap
  // back into range; the anchored grid's tile_shift may also leave the address 8 bytes off, then the scalar stores)
  if constexpr (R % PER16 == 0) {
    if (k0 < N && N - k0 >= (uint64_t)R && (reinterpret_cast<uintptr_t>(out + k0) & 15u) == 0) {
      float4* o = reinterpret_cast<float4*>(out + k0);
#pragma unroll
      for (int q = 0; q < R / PER16; ++q) {
        float4 w;
        if constexpr (PER16 == 2) {
          w = make_float4(reinterpret_cast<const float2&>(acc[2 * q]).x, reinterpret_cast<const float2&>(acc[2 * q]).y,
                          reinterpret_cast<const float2&>(acc[2 * q + 1]).x,
                          reinterpret_cast<const float2&>(acc[2 * q + 1]).y);
        } else {
          w = make_float4(reinterpret_cast<const float&>(acc[4 * q]), reinterpret_cast<const float&>(acc[4 * q + 1]),
                          reinterpret_cast<const float&>(acc[4 * q + 2]),
                          reinterpret_cast<const float&>(acc[4 * q + 3]));
        }
        if constexpr (NTS) {
          store16_nt(o + q, w);
        } else {
          o[q] = w;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (k0 + r < N) out[k0 + r] = acc[r];
  }
}

// FIR-mode store of a whole tile through LDS (CST != 0): thread t holds outputs t*R .. t*R+R-1, so a
// direct 16-byte store puts the lanes of one wave instruction R*sizeof(OutT) bytes apart (2 KB, 16
// cache lines per instruction for complex R = 4). Transposed through LDS, slot q*WG + t of the tile
// goes out with lane t, and every wave instruction writes one contiguous 1 KB run. CST = 2 uses
// streaming (non-temporal) stores. Returns false (nothing written) for a partial or misaligned tile,
// which then takes the per-thread store; the condition is uniform over the workgroup.
template <int CST, class OutT, int R, int WG>
__device__ __forceinline__ bool store_tile_lds(float4* lds, const FirParams& p, uint64_t out0, const OutT (&acc)[R]) {
  constexpr int NQ = R * (int)sizeof(OutT) / 16;  // float4 per thread
  static_assert(NQ * 16 == R * (int)sizeof(OutT), "R outputs must fill whole 16-byte slots");
  OutT* out = reinterpret_cast<OutT*>(p.out) + out0;
  if (out0 + (uint64_t)WG * R > p.N || (reinterpret_cast<uintptr_t>(out) & 15u) != 0) return false;
  const uint32_t t = threadIdx.x;
  __syncthreads();  // every wave is done reading the input tile
  float4 w[NQ];
  __builtin_memcpy(w, acc, sizeof(w));
#pragma unroll
  for (int q = 0; q < NQ; ++q) lds[t * NQ + q] = w[q];
  __syncthreads();
  float4* o = reinterpret_cast<float4*>(out);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float4 v = lds[q * WG + t];
    if constexpr (CST == 2) {
      store16_nt(o + q * WG + t, v);
    } else {
      o[q * WG + t] = v;
    }
  }
  return true;
}

// Shared by the tiled kernels. `xs` is a WG-sized LDS exchange area (FM mode only); `tile` the staged
// input tile, which FM mode with COAL reuses (WG * R floats) once every wave is done with it.
// A thread's R consecutive demodulated outputs, local indices ml0 .. ml0 + R - 1 of the tile (those below `lim`)
// at output m0: one 8- or 16-byte store when all R are in range and the address allows, so the lanes of a wave
// store one contiguous run (R * 256 bytes); one store each otherwise.
template <int R>
__device__ __forceinline__ void store_chain(float* __restrict__ out, uint64_t m0, uint32_t ml0, uint32_t lim, uint64_t N,
                                            const float (&o)[R]) {
  if constexpr (R == 2 || R == 4) {
    // (m0 < N first: the anchored tiles' leading outputs have m0 wrapped below zero)
    if (ml0 + R <= lim && m0 < N && N - m0 >= R && (reinterpret_cast<uintptr_t>(out + m0) % (4 * R)) == 0) {
      if constexpr (R == 4) {
        *reinterpret_cast<float4*>(out + m0) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
        *reinterpret_cast<float2*>(out + m0) = make_float2(o[0], o[1]);
      }
      return;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (ml0 + r < lim && m0 + r < N) out[m0 + r] = o[r];
  }
}

// COAL (FM, the contiguous-window kernels' tiles): the discriminator outputs leave through LDS in wave-contiguous
// runs; without it (the anchored polyphase tiles) each thread stores its R outputs with one vector store
// (store_chain), which is as contiguous and needs neither the LDS round trip nor its barrier.
template <int MODE, class OutT, int R, int WG, bool NTS = false, bool COAL = false>
__device__ __forceinline__ void tile_epilogue(const FirParams& p, uint64_t out0, OutT (&acc)[R], float2* xs,
                                              float4* tile = nullptr) {
  const uint32_t t = threadIdx.x;
  const uint32_t local0 = t * R;
  if constexpr (MODE == kModeFir || MODE == kModeIq) {
    // (kModeIq: the FIR store behind the NCO staging; the anchored tiles have rotated acc to the absolute phase,
    // anchor_rotate)
    store_fir<OutT, R, NTS>(reinterpret_cast<OutT*>(p.out), out0 + local0, p.N, acc);
  } else if constexpr (MODE == kModeAm) {
    float o[R];
#pragma unroll
    for (int r = 0; r < R; ++r) o[r] = am_env(acc[r]);
    store_chain<R>(reinterpret_cast<float*>(p.out), out0 + local0, local0, 0xffffffffu, p.N, o);
  } else {
    // Tiles overlap: the last thread's outputs (anchored polyphase tiles, tile_stride = KT - R) or the last one or
    // two (the other kernels, KT - 1 or KT - 2, fm_tile_stride) are only partners; the neighbouring thread's
    // first output comes through LDS.
    xs[t] = acc[0];
    __syncthreads();
    // value select (both loads in range): a select of the two addresses became a flat load through
    // scratch when R = 1
    const float2 nb = xs[t + 1 < WG ? t + 1 : t];
    const float2 nxt = (t + 1 < WG) ? nb : acc[R - 1];
    float o[R];
#pragma unroll
    for (int r = 0; r + 1 < R; r += 2) {
      const float2 y2 = (r + 2 < R) ? acc[r + 2] : nxt;
      const gsdr_f32x2 v = fm_disc2(acc[r], acc[r + 1], acc[r + 1], y2, p.fm_gain);
      o[r] = v.x;
      o[r + 1] = v.y;
    }
    if constexpr (R % 2 == 1) o[R - 1] = fm_disc(acc[R - 1], nxt, p.fm_gain);
    float* out = reinterpret_cast<float*>(p.out);
    if constexpr (COAL && R > 1) {
      // Through LDS so that every wave instruction stores one contiguous 256-byte run: stored
      // straight from registers, a thread's R outputs put the lanes of one dword store R * 4 bytes
      // apart. The tile area is free: every wave has passed the barrier above, i.e. finished its MACs.
      float* lo = reinterpret_cast<float*>(tile);
#pragma unroll
      for (int r = 0; r < R; ++r) lo[local0 + r] = o[r];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const uint32_t ml = q * WG + t;
        const uint64_t m = out0 + ml;
        if (ml < p.tile_stride && m < p.N) out[m] = lo[ml];
      }
    } else {
      store_chain<R>(out, out0 + local0, local0, p.tile_stride, p.N, o);
    }
  }
}

// An ordering point (no instruction): memory accesses written after it stay after the products accumulated into `a`
// so far.
__device__ __forceinline__ void after_products(float& a) { asm volatile("" : "+v"(a)::"memory"); }
__device__ __forceinline__ void after_products(float2& a) {
  gsdr_f32x2 v = {a.x, a.y};
  asm volatile("" : "+v"(v)::"memory");
  a = make_float2(v.x, v.y);
}

// ------------------------------------------------------------------------------------------------
// Polyphase compute core shared by the polyphase kernels: thread t accumulates its R outputs from
// the staged tile in LDS. JC = tap rows per chunk (a multiple of R); a chunk covers JC*D taps.
//   * Taps: the whole chunk in one scalar batch, settled before the first window read (TapChunk), where the chunk
//     is 16, 32 or 64 dwords; other shapes fetch them per column.
//   * Window: column h of chunk c is rows u = 0 .. R+JC-2 of that column, and its last R-1 rows are the first R-1
//     rows of the same column in chunk c+1 (the chunk advances JC rows). Those granules stay in registers across the
//     other columns instead of being read from LDS again: (R-1) * CPR granules carried, (R-1) of R+JC-1 reads a column
//     saved in every chunk but the first. The first chunk is peeled, so which reads exist is fixed at compile time.
//   The order of every accumulator's products (chunk c, column h, row j, element e) is untouched by either.
// ROUND8: the round-8 core, which FIR mode has and the chains do not yet have ("Left out"):
// a granule's two real taps read from their SGPR pair, and the carried rows read where the old ones die. Without it
// the odd taps are copied out of their pair and the carried rows are read with the rest of the window and copied.
// ------------------------------------------------------------------------------------------------
template <class TapT, class InT, int D, int R, int JC, int WG, bool ROUND8>
__device__ __forceinline__ void poly_compute(const float4* __restrict__ lds, const FirParams& p,
                                             typename Product<TapT, InT>::type (&acc)[R]) {
  using Geo = TileGeo<InT, D, R, WG>;
  constexpr int G = Geo::G;
  constexpr int CPR = D / G;  // granule columns per input row
  static_assert(D % G == 0, "polyphase kernel needs whole granules per row");
  static_assert(JC % R == 0, "chunk rows must be whole thread segments");
  constexpr int NWIN = R + JC - 1;
  constexpr int NCARRY = R - 1;  // (JC >= R: the carried rows are the chunk's own reads)
  constexpr int CHUNK_DW = tap_chunk_dwords<TapT>(JC * D);
  constexpr bool WHOLE = tap_chunk_whole(CHUNK_DW);
  // real taps against complex samples: a granule's two taps are one even-aligned SGPR pair (TapChunk::pair)
  constexpr bool PAIRED = ROUND8 && WHOLE && std::is_same<TapT, float>::value && G == 2 && D % 2 == 0;
  // the rows carried to the next chunk are read where the carried rows of this one die (below)
  constexpr int NLATE = (ROUND8 && NCARRY > 0 && JC > 2 * NCARRY) ? NCARRY : 0;
  // (tap row of that point: 3 tap rows, 12 R FMAs, ahead of the new rows' first product; no earlier than the old rows'
  // last)
  constexpr int LATE_J = (JC - NCARRY - 3) > NCARRY ? (JC - NCARRY - 3) : NCARRY;
  const uint32_t t = threadIdx.x;
  float4 carry[CPR][NCARRY > 0 ? NCARRY : 1];
  auto chunk = [&](uint32_t c, auto first) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first)::value;
    const float4* __restrict__ seg = lds + (t + c * (JC / R)) * Geo::SGP;
    TapChunk<WHOLE ? CHUNK_DW / 16 : 1> tc;
    if constexpr (WHOLE) {
      tc.load(tap_window<TapT>(p.taps, p.T, c * JC * D));
      tc.settle();
    }
#pragma unroll
    for (int h = 0; h < CPR; ++h) {
      TapT tv[JC][G];
      if constexpr (PAIRED) {
#pragma unroll
        for (int j = 0; j < JC; ++j) {
          const gsdr_f32x2 tp = tc.pair(j * D + h * G);
          tv[j][0] = tp.x;
          tv[j][1] = tp.y;
        }
      } else if constexpr (WHOLE) {
#pragma unroll
        for (int j = 0; j < JC; ++j) {
#pragma unroll
          for (int e = 0; e < G; ++e) tv[j][e] = tc.template at<TapT>(j * D + h * G + e);
        }
      } else {
        const TapBuf tb = tap_window<TapT>(p.taps, p.T, c * JC * D + h * G);
#pragma unroll
        for (int j = 0; j < JC; ++j) {
#pragma unroll
          for (int e = 0; e < G; ++e) tv[j][e] = tap_at<TapT>(tb, j * D + e);
        }
      }
      float4 win[NWIN];
      auto read_row = [&](int u) __attribute__((always_inline)) {
        const int q = u * CPR + h;
        return seg[q + Geo::PAD * (q / Geo::SG)];
      };
#pragma unroll
      for (int u = 0; u < NWIN - NLATE; ++u) {
        if (!FIRST && u < NCARRY) {
          win[u] = carry[h][u];
        } else {
          win[u] = read_row(u);
        }
      }
      if constexpr (NLATE == 0) {
#pragma unroll
        for (int u = 0; u < NCARRY; ++u) carry[h][u] = win[JC + u];
      }
#pragma unroll
      for (int j = 0; j < JC; ++j) {
        // Rows JC .. JC + NCARRY - 1 become the next chunk's rows 0 .. NCARRY - 1. The old rows' last products are
        // tap row j = NCARRY - 1's (into acc[0 .. NCARRY - 1]) and the new rows' first are tap row j = JC - NCARRY's,
        // so read at this point the new rows never live beside the old ones and take their registers: read with the
        // rest of the window, they were copied into them (v_mov_b64, 2 a carried granule and chunk). after_products
        // keeps the reads behind those products while registers are assigned.
        if constexpr (NLATE > 0) {
          if (j == LATE_J) {
#pragma unroll
            for (int u = 0; u < NCARRY; ++u) after_products(acc[u]);
#pragma unroll
            for (int u = 0; u < NCARRY; ++u) win[JC + u] = carry[h][u] = read_row(JC + u);
          }
        }
#pragma unroll
        for (int e = 0; e < G; ++e) {
#pragma unroll
          for (int r = 0; r < R; ++r) mac(acc[r], granule_sample<typename LdsSample<InT>::type>(win[r + j], e), tv[j][e]);
        }
      }
    }
  };
  if constexpr (NCARRY > 0) {
    if (p.nch == 0) return;
    chunk(0u, std::true_type{});
    for (uint32_t c = 1; c < p.nch; ++c) chunk(c, std::false_type{});
  } else {
    for (uint32_t c = 0; c < p.nch; ++c) chunk(c, std::true_type{});
  }
}

// ------------------------------------------------------------------------------------------------
// Exact zero-padding semantics. The tiled cores round T up to whole tap chunks and multiply the
// padding (taps read as +0 past T) like any other tap. For a finite sample x*0 is a signed zero and
// adding it leaves the sum unchanged, but for x = +-Inf or NaN it is NaN, which the reference never
// computes: its loop stops at tap T-1 (fir.cu:29-31, 58-60). A padding product can therefore only turn
// an output into NaN. So every output that came out non-finite (a NaN or Inf output: a cheap test, and
// rare) is recomputed from the staged tile in the SAME MAC order with the padding products skipped --
// exactly the fast path's sum whenever no padding product was NaN, and the reference's set of products
// otherwise. The result depends only on the output's own window, never on the tiling, so chunked and
// monolithic calls stay bit-identical.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_out(float a) { return __builtin_isfinite(a); }
__device__ __forceinline__ bool finite_out(float2 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y); }

struct NoPad {
  __host__ __device__ static constexpr uint32_t padded(uint32_t g) { return g; }
};

// sample s of the tile (local index) from the LDS granule layout (padded as TileGeo when PADDED)
template <class InT, class Geo, bool PADDED>
__device__ __forceinline__ typename LdsSample<InT>::type tile_sample(const float4* __restrict__ lds, uint32_t s) {
  using LdsT = typename LdsSample<InT>::type;
  constexpr uint32_t G = SampleT<InT>::kPerGranule;
  const uint32_t g = s / G;
  const uint32_t slot = PADDED ? Geo::padded(g) : g;
  return reinterpret_cast<const LdsT*>(lds)[slot * G + s % G];
}

// Polyphase order (poly_compute): chunk c, granule column h, row j, element e -- tap
// i = (c*JC + j)*D + h*G + e of local output m = threadIdx.x * R + r.
template <class TapT, class InT, int D, int R, int JC, int WG>
__device__ __forceinline__ void poly_fixup(const float4* __restrict__ lds, const FirParams& p,
                                        typename Product<TapT, InT>::type (&acc)[R]) {
  using Geo = TileGeo<InT, D, R, WG>;
  constexpr int G = Geo::G, CPR = D / G;
  const TapT* __restrict__ taps = reinterpret_cast<const TapT*>(p.taps);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (finite_out(acc[r])) continue;
    const uint32_t s0 = (threadIdx.x * R + r) * D;
    typename Product<TapT, InT>::type a;
    set_zero(a);
#pragma unroll 1
    for (uint32_t c = 0; c < p.nch; ++c) {
#pragma unroll 1
      for (int h = 0; h < CPR; ++h) {
#pragma unroll 1
        for (int j = 0; j < JC; ++j) {
          const uint32_t i0 = (c * JC + j) * D + h * G;
#pragma unroll
          for (int e = 0; e < G; ++e) {
            if (i0 + e < p.T) mac(a, tile_sample<InT, Geo, true>(lds, s0 + i0 + e), taps[i0 + e]);
          }
        }
      }
    }
    acc[r] = a;
  }
}

// Ascending tap order (contiguous-window, runtime-decimation and matrix-core cores): local output m at
// local sample m * D.
template <class TapT, class InT, class Geo, bool PADDED, int R>
__device__ __forceinline__ void ascending_fixup(const float4* __restrict__ lds, const FirParams& p, uint32_t D,
                                             uint32_t m0, typename Product<TapT, InT>::type (&acc)[R]) {
  const TapT* __restrict__ taps = reinterpret_cast<const TapT*>(p.taps);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (finite_out(acc[r])) continue;
    const uint32_t s0 = (m0 + r) * D;
    typename Product<TapT, InT>::type a;
    set_zero(a);
#pragma unroll 1
    for (uint32_t i = 0; i < p.T; ++i) mac(a, tile_sample<InT, Geo, PADDED>(lds, s0 + i), taps[i]);
    acc[r] = a;
  }
}

// Wave-cheap screen for the fix-up: the sum of a thread's outputs is finite when they all are (a NaN or
// Inf term makes it NaN or Inf). A finite set whose sum overflows only sends the thread through the
// per-output test in the fix-up, which then changes nothing. Packed adds: 5 VALU operations for R = 4
// complex outputs instead of one class test per component.
template <int R>
__device__ __forceinline__ bool all_finite(const float2 (&acc)[R]) {
  gsdr_f32x2 s = {acc[0].x, acc[0].y};
#pragma unroll
  for (int r = 1; r < R; ++r) s += gsdr_f32x2{acc[r].x, acc[r].y};
  return __builtin_isfinite(s.x + s.y);
}
template <int R>
__device__ __forceinline__ bool all_finite(const float (&acc)[R]) {
  if constexpr (R % 2 == 0) {
    gsdr_f32x2 s = {acc[0], acc[1]};
#pragma unroll
    for (int r = 2; r < R; r += 2) s += gsdr_f32x2{acc[r], acc[r + 1]};
    return __builtin_isfinite(s.x + s.y);
  } else {
    float s = acc[0];
#pragma unroll
    for (int r = 1; r < R; ++r) s += acc[r];
    return __builtin_isfinite(s);
  }
}

// ------------------------------------------------------------------------------------------------
// Kernel 1: polyphase-granule kernel, one tile per workgroup (D a multiple of the granule width G).
// ------------------------------------------------------------------------------------------------
// A tile's shape, as a row of GSDR_FIR_ROWS or GSDR_FIR_D4_VARIANTS states it (fir_plan.hpp; SUBS: tiles an NCO cell).
template <int D_, int R_, int JC_, int WG_, int SUBS_ = 1>
struct TileShape {
  static constexpr int D = D_, R = R_, JC = JC_, WG = WG_, SUBS = SUBS_;
};
// A tile's options, all off by default. NT: non-temporal (streaming) HBM loads for the staged input, and stores; XM:
// XCD-aware tile order (tile_of_block); CST: the FIR tile stored through LDS (store_tile_lds; 1 plain, 2 streaming
// stores); DMA: the tile body staged by LDS-DMA (stage_body_dma). PROBE (tuning probes, gsdrxFirFCVariant >= 100 of
// the probes library): the tile with a part of its work left out -- one half of it, the chains' NCO mix, or FM's
// discriminator (a plain float store instead).
template <bool NT_ = false, bool XM_ = false, int CST_ = 0, bool DMA_ = false, int PROBE_ = 0>
struct TileOpts {
  static constexpr bool NT = NT_, XM = XM_, DMA = DMA_;
  static constexpr int CST = CST_, PROBE = PROBE_;
};
using TileStreamed = TileOpts<true>;  // what every default shape runs
constexpr int kProbeStageOnly = 1, kProbeComputeOnly = 2, kProbeNoMix = 8, kProbeNoDisc = 16;
template <class Opts, int MASK>
struct Probed : Opts {
  static constexpr int PROBE = MASK;
};

// Tile of workgroup b. XCD-aware (XM): workgroups are dispatched round-robin over the 8 XCDs, so
// with the identity map neighbouring tiles (which share a halo of input rows) sit on different L2s;
// remapped, XCD x walks one contiguous range of tiles and the halo of the previous tile is still in
// its L2.
template <bool XM>
__device__ __forceinline__ uint32_t tile_of_block() {
  if constexpr (!XM) {
    return blockIdx.x;
  } else {
    const uint32_t nb = gridDim.x, b = blockIdx.x;
    const uint32_t per = nb / 8, rem = nb % 8, x = b % 8, i = b / 8;
    return x * per + (x < rem ? x : rem) + i;
  }
}

// One tile of the polyphase kernel (the body of k_fir_poly and of k_fir_poly_grouped). FM / AM tiles are
// anchored (MixAnchored): tile t covers outputs [t S - tile_shift, t S - tile_shift + KT) with S = tile_stride
// (KT for AM; KT - R for FM, whose last thread's outputs only serve as the discriminator partners of the one before,
// so every discriminator pairs two outputs of one tile in one NCO frame) and is sub-tile (cell_sub0 + t) mod SUBS of
// its NCO cell of SUBS tiles.
template <class TapT, class InT, class Shape, bool VEC, int MODE, int SH, class Opts>
__device__ __forceinline__ void fir_poly_tile(const FirParams& p, uint32_t tile) {
  constexpr int D = Shape::D, R = Shape::R, JC = Shape::JC, WG = Shape::WG, SUBS = Shape::SUBS, CST = Opts::CST;
  constexpr bool NT = Opts::NT, DMA = Opts::DMA && SH == 0;  // (the shifted loads have no LDS-DMA form)
  constexpr bool STAGE_ONLY = (Opts::PROBE & kProbeStageOnly) != 0, COMPUTE_ONLY = (Opts::PROBE & kProbeComputeOnly) != 0;
  constexpr bool NO_MIX = (Opts::PROBE & kProbeNoMix) != 0, NO_DISC = (Opts::PROBE & kProbeNoDisc) != 0;
  using Geo = TileGeo<InT, D, R, WG>;
  using OutT = typename Product<TapT, InT>::type;
  constexpr int G = Geo::G;
  constexpr bool ANCH = MODE != kModeFir;
  constexpr int BPT = Geo::SG * (Geo::KT / Geo::ROUT) / WG;  // granule rows of the tile body

  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const InT* __restrict__ in = reinterpret_cast<const InT*>(p.in);
  const HistSample<InT> hist = stream_history_load<InT>(p);

  // (an anchored call's first tile may start before output 0: out0 and S0 are then "negative", wrapped)
  const uint64_t out0 = (uint64_t)tile * p.tile_stride - (ANCH ? p.tile_shift : 0u);
  const uint64_t S0 = out0 * D;
  const uint32_t span = p.nch * JC * D;
  const uint32_t NG = ((Geo::KT - 1) * D + span + G - 1) / G;
  // LDS: [tile granules | FM exchange (WG float2)]
  // the tile is sub-tile `sub` of its NCO cell: it starts sub (KT - R) outputs (FM) or sub KT outputs (AM, IQ) into
  // the cell, i.e. sub BPT granule rows in, less sub SG granules for FM (MixAnchored)
  const uint32_t sub = ANCH ? (p.cell_sub0 + tile) % SUBS : 0u;
  // Whole tiles of the full-size FIR tile on aligned complex samples are staged wave by wave, with the wave's own
  // wait behind them (stage_tile_wave; uniform over the workgroup). Everything else -- the chains, the shifted and DMA
  // staging, the tile stores through LDS, smaller workgroups, and the tiles that path declines -- keeps the workgroup's
  // map and its barrier.
  constexpr bool WAVE = MODE == kModeFir && std::is_same<InT, float2>::value && VEC && SH == 0 && !DMA && CST == 0 &&
                        WG == 256 && 64 % Geo::SG == 0 && !STAGE_ONLY && !COMPUTE_ONLY;
  bool waved = false;
  if constexpr (!COMPUTE_ONLY) {
    if constexpr (ANCH && !NO_MIX) {
      stage_tile<InT, Geo, WG, VEC, NT, DMA, SH>(
          lds, in, S0, NG, p, MixAnchored<WG>(p.nco_inc, sub * BPT, MODE == kModeFm ? sub * Geo::SG : 0u));
    } else {
      if constexpr (WAVE) waved = stage_tile_wave<Geo, WG, NT>(lds, in, S0, NG, p);
      if (!waved) stage_tile<InT, Geo, WG, VEC, NT, DMA, SH>(lds, in, S0, NG, p, MixNone{});
    }
  }
  if (waved) {
    wave_staged();
  } else {
    __syncthreads();
  }
  stream_history_store<InT>(p, hist);
  float2* xs = reinterpret_cast<float2*>(lds + Geo::padded(NG - 1) + 1);

  OutT acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) set_zero(acc[r]);
  if constexpr (STAGE_ONLY) {
    const float4 v = lds[Geo::padded(threadIdx.x * Geo::SG)];
#pragma unroll
    for (int r = 0; r < R; ++r) mac(acc[r], granule_sample<typename LdsSample<InT>::type>(v, r % G), 1.0f);
  } else {
    poly_compute<TapT, InT, D, R, JC, WG, MODE == kModeFir>(lds, p, acc);
    if constexpr (Opts::PROBE == 0) {
      if (!all_finite(acc)) poly_fixup<TapT, InT, D, R, JC, WG>(lds, p, acc);
    }
  }
  if constexpr (MODE == kModeIq && !NO_MIX) {
    // back to the absolute phase: the cell's first output is sub * tile_stride outputs before the tile's
    anchor_rotate(p, (uint32_t)out0 - sub * p.tile_stride, D, acc);
  }

  if constexpr (CST != 0 && MODE == kModeFir) {
    if (store_tile_lds<CST, OutT, R, WG>(lds, p, out0, acc)) return;
  }
  if constexpr (NO_DISC && MODE == kModeFm) {
    float* out = reinterpret_cast<float*>(p.out);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t ml = threadIdx.x * R + r;
      if (ml < p.tile_stride && out0 + ml < p.N) out[out0 + ml] = acc[r].x + acc[r].y;
    }
    return;
  }
  tile_epilogue<MODE, OutT, R, WG, NT, !ANCH>(p, out0, acc, xs, lds);
}

template <class TapT, class InT, class Shape, bool VEC, int MODE, int SH, class Opts>
__global__ __launch_bounds__(Shape::WG) void k_fir_poly(FirParams p) {
  fir_poly_tile<TapT, InT, Shape, VEC, MODE, SH, Opts>(p, tile_of_block<Opts::XM>());
}

// ------------------------------------------------------------------------------------------------
// Multi-channel NCO + FIR + demodulator (the intent of the reference's
// dead k_Fm4x, src/fm.cu:71-179): up to kMaxMultiChannels channels of one input per launch.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxMultiChannels = 16;

struct MultiParams {
  uint32_t count;                     // channels in this launch
  uint32_t inc[kMaxMultiChannels];    // NCO phase increment per channel
  float gain[kMaxMultiChannels];      // FM gain per channel
  uint64_t out_stride;                // outputs between consecutive channels' first outputs (>= N)
};

// Kernel 1g: multi-channel chains as C single-channel tiles per input tile, grouped for the L2. Block b
// runs channel c of tile t, with b mod 8 = t mod 8 and the C channels of a tile consecutive among the
// blocks of that residue: workgroups are dispatched round-robin over the 8 XCDs, so the C workgroups of a
// tile run close together on ONE XCD and all but the first stage the tile from that XCD's L2 rather
// than HBM. Each block is exactly the single-channel kernel's tile (same template, same code), so
// channel c is bit-identical to gsdrFmDemod / gsdrAmDemod with its own frequency by construction, at
// the single-channel kernel's register budget. (The first multi-channel kernel read each input tile
// into registers once and looped over the channels: 228 VGPRs, 2 waves per SIMD, 5 % slower.)
template <class TapT, class InT, class Shape, bool VEC, int MODE, int SH>
__global__ __launch_bounds__(Shape::WG) void k_fir_poly_grouped(FirParams p, MultiParams mp, uint32_t tiles) {
  const uint32_t C = mp.count;
  const uint32_t b = blockIdx.x, r = b >> 3;
  const uint32_t tile = (r / C) * 8u + (b & 7u), c = r % C;
  if (tile >= tiles) return;  // the grid is rounded up to whole groups of 8 tiles
  FirParams pc = p;
  pc.nco_inc = mp.inc[c];
  pc.fm_gain = mp.gain[c];
  // (out_stride counts outputs: floats for FM / AM, complex elements for the frequency-translating FIR)
  using ChanOutT = std::conditional_t<MODE == kModeIq, float2, float>;
  pc.out = reinterpret_cast<ChanOutT*>(p.out) + (uint64_t)c * mp.out_stride;
  if (c != 0) pc.hist_out = nullptr;  // a multi-channel stream step: channel 0's workgroup 0 copies the history
  fir_poly_tile<TapT, InT, Shape, VEC, MODE, SH, TileStreamed>(pc, tile);
}

// ------------------------------------------------------------------------------------------------
// Kernel 2: contiguous-window kernel for small D (D = 1 in particular).
//   IC = taps per chunk (a multiple of R*D).
// ------------------------------------------------------------------------------------------------
template <class TapT, class InT, int D, int R, int IC, int WG, bool VEC, int MODE, int SH = 0>
__global__ __launch_bounds__(WG) void k_fir_contig(FirParams p) {
  using Geo = TileGeo<InT, D, R, WG>;
  using OutT = typename Product<TapT, InT>::type;
  constexpr int G = Geo::G;
  static_assert(IC % (R * D) == 0, "chunk taps must be whole thread segments");
  constexpr int W = (R - 1) * D + IC;  // window samples
  constexpr int NWIN = (W + G - 1) / G;

  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const InT* __restrict__ in = reinterpret_cast<const InT*>(p.in);
  const HistSample<InT> hist = stream_history_load<InT>(p);

  const uint64_t out0 = (uint64_t)blockIdx.x * p.tile_stride;
  const uint64_t S0 = out0 * D;
  const uint32_t span = p.nch * IC;
  const uint32_t NG = ((Geo::KT - 1) * D + span + G - 1) / G;

  if constexpr (MODE == kModeFir) {
    stage_tile<InT, Geo, WG, VEC, false, false, SH>(lds, in, S0, NG, p, MixNone{});
  } else {
    stage_tile<InT, Geo, WG, VEC, false, false, SH>(lds, in, S0, NG, p, MixAbsolute<InT, MODE, WG>(p, S0));
  }
  __syncthreads();
  stream_history_store<InT>(p, hist);

  OutT acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) set_zero(acc[r]);

  const uint32_t t = threadIdx.x;
  for (uint32_t c = 0; c < p.nch; ++c) {
    const float4* __restrict__ seg = lds + (t + c * (IC / (R * D))) * Geo::SGP;
    const TapBuf tb = tap_window<TapT>(p.taps, p.T, c * IC);
    TapT tvs[IC];
#pragma unroll
    for (int i = 0; i < IC; ++i) tvs[i] = tap_at<TapT>(tb, i);
    float4 win[NWIN];
#pragma unroll
    for (int q = 0; q < NWIN; ++q) win[q] = seg[q + Geo::PAD * (q / Geo::SG)];
#pragma unroll
    for (int i = 0; i < IC; ++i) {
      const TapT tv = tvs[i];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int s = r * D + i;
        mac(acc[r], granule_sample<typename LdsSample<InT>::type>(win[s / G], s % G), tv);
      }
    }
  }

  if (!all_finite(acc)) ascending_fixup<TapT, InT, Geo, true, R>(lds, p, D, t * R, acc);

  float2* xs = reinterpret_cast<float2*>(lds + Geo::padded(NG - 1) + 1);
  tile_epilogue<MODE, OutT, R, WG>(p, out0, acc, xs);
}

// ------------------------------------------------------------------------------------------------
// Kernel 2r: runtime-decimation tile kernel, for decimations without a compile-time shape. The tile's
// input span is staged into LDS unpadded (NCO applied once per sample, as in the other tiled kernels)
// and thread t computes output t of the tile from LDS, one sample read per tap (ds_read with the tap
// as an immediate offset), in ascending tap order like the generic kernel. No register window (D is
// not known at compile time), so it is bound by LDS reads (~T * sample bytes per output), which
// still beats re-reading every sample T / D times through L1/L2.
// PAIR (even D): two consecutive samples per LDS read (complex: ds_read_b128, real: ds_read_b64), still
// multiplied in ascending tap order. One sample a read puts lane t at bank 2Dt mod 64 (complex), which
// for D = 2^k m (m odd) touches only 64 / 2^k of the banks: 2-way conflicts at D = 50, 4-way at 100
// (PMC: 42 % of LDS cycles at D = 50, profiles/r01_pmc_fir_rt_d50_d13.txt). ds_read_b128 serves 16
// lanes a cycle with lane groups whose indices cover every residue mod 16, so lane starts 4(D/2)t mod 64
// are distinct for D = 2 mod 4 (conflict-free) and 2-way at D = 4 mod 8; half the read instructions too.
// ------------------------------------------------------------------------------------------------
template <class LdsT>
struct LdsPair;
template <>
struct LdsPair<float> {
  using type = float2;
  __device__ static float lo(float2 v) { return v.x; }
  __device__ static float hi(float2 v) { return v.y; }
};
template <>
struct LdsPair<float2> {
  using type = float4;
  __device__ static float2 lo(float4 v) { return make_float2(v.x, v.y); }
  __device__ static float2 hi(float4 v) { return make_float2(v.z, v.w); }
};

// N separate ds_read_b64 of the 8-byte values at p[0..N): the compiler merges adjacent 8-byte LDS loads
// into ds_read2_b64, which takes 16 LDS cycles per 16 bytes against 4 for two ds_read_b64 (and banks
// mod 32), so at odd D the one-sample-a-read loop ran at a quarter of the LDS rate. The reads and their
// wait are ONE asm statement with early-clobber outputs, so no register is taken as written before the
// s_waitcnt that fills it (a copy scheduled between separate read and wait statements would
// have read a register the load had not filled yet).
#define GSDR_R8(i) "ds_read_b64 %" #i ", %[a] offset:" #i "*8\n\t"
template <int N>
__device__ __forceinline__ void lds_read_b64_n(const float2* p, float2 (&out)[N]);
template <>
__device__ __forceinline__ void lds_read_b64_n<8>(const float2* p, float2 (&out)[8]) {
  const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float2*)p;
  gsdr_f32x2 r0, r1, r2, r3, r4, r5, r6, r7;
  asm volatile(GSDR_R8(0) GSDR_R8(1) GSDR_R8(2) GSDR_R8(3) GSDR_R8(4) GSDR_R8(5) GSDR_R8(6) GSDR_R8(7)
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
               : [a] "v"(a)
               : "memory");
  const gsdr_f32x2 r[8] = {r0, r1, r2, r3, r4, r5, r6, r7};
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = make_float2(r[i].x, r[i].y);
}
template <>
__device__ __forceinline__ void lds_read_b64_n<16>(const float2* p, float2 (&out)[16]) {
  const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float2*)p;
  gsdr_f32x2 r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15;
  asm volatile(GSDR_R8(0) GSDR_R8(1) GSDR_R8(2) GSDR_R8(3) GSDR_R8(4) GSDR_R8(5) GSDR_R8(6) GSDR_R8(7)
               GSDR_R8(8) GSDR_R8(9) GSDR_R8(10) GSDR_R8(11) GSDR_R8(12) GSDR_R8(13) GSDR_R8(14) GSDR_R8(15)
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7),
                 "=&v"(r8), "=&v"(r9), "=&v"(r10), "=&v"(r11), "=&v"(r12), "=&v"(r13), "=&v"(r14), "=&v"(r15)
               : [a] "v"(a)
               : "memory");
  const gsdr_f32x2 r[16] = {r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15};
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = make_float2(r[i].x, r[i].y);
}
#undef GSDR_R8

template <class TapT, class InT, int IC, int WG, bool VEC, int MODE, bool PAIR = false>
__global__ __launch_bounds__(WG) void k_fir_rt(FirParams p) {
  using OutT = typename Product<TapT, InT>::type;
  using LdsT = typename LdsSample<InT>::type;
  constexpr int G = SampleT<InT>::kPerGranule;
  // granules in flight per lane while staging: the tile (D * WG samples) bounds the resident workgroups to
  // 1-2 waves a SIMD at large D, so each lane keeps 16 loads (256 B) in flight (4: D = 50 FC 125 us)
  constexpr int SB = 16;

  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const InT* __restrict__ in = reinterpret_cast<const InT*>(p.in);
  const uint32_t D = p.D;
  const uint64_t out0 = (uint64_t)blockIdx.x * p.tile_stride;
  const uint64_t S0 = out0 * D;
  const uint32_t span = p.nch * IC;
  const uint32_t NG = ((WG - 1) * D + span + G - 1) / G;
  const uint32_t tid = threadIdx.x;
  for (uint32_t g0 = 0; g0 < NG; g0 += SB * WG) {
    float4 v[SB];
#pragma unroll
    for (int k = 0; k < SB; ++k) {
      const uint32_t g = g0 + k * WG + tid;
      v[k] = g < NG ? load_granule<InT, VEC>(in, S0 + (uint64_t)g * G, p.L) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < SB; ++k) {
      const uint32_t g = g0 + k * WG + tid;
      if (g < NG) lds[g] = stage_transform<InT, MODE>(v[k], (uint32_t)(S0 + (uint64_t)g * G), p);
    }
  }
  __syncthreads();

  OutT acc;
  set_zero(acc);
  const LdsT* __restrict__ xs = reinterpret_cast<const LdsT*>(lds) + tid * D;
  for (uint32_t c = 0; c < p.nch; ++c) {
    const TapBuf tb = tap_window<TapT>(p.taps, p.T, c * IC);
    TapT tv[IC];
#pragma unroll
    for (int i = 0; i < IC; ++i) tv[i] = tap_at<TapT>(tb, i);
    const LdsT* __restrict__ xc = xs + c * IC;
    if constexpr (PAIR) {
      static_assert(IC % 2 == 0, "pairs of taps");
      using P = LdsPair<LdsT>;
      const typename P::type* __restrict__ xp = reinterpret_cast<const typename P::type*>(xc);  // D even: aligned
      typename P::type v[IC / 2];
      if constexpr (std::is_same<typename P::type, float2>::value) {
        lds_read_b64_n<IC / 2>(xp, v);  // real samples: 8-byte pairs, kept apart from ds_read2_b64
      } else {
#pragma unroll
        for (int i = 0; i < IC / 2; ++i) v[i] = xp[i];
      }
#pragma unroll
      for (int i = 0; i < IC / 2; ++i) {
        mac(acc, P::lo(v[i]), tv[2 * i]);
        mac(acc, P::hi(v[i]), tv[2 * i + 1]);
      }
    } else if constexpr (std::is_same<LdsT, float2>::value && std::is_same<TapT, float>::value) {
      // (complex taps keep the compiler's loads: their two packed FMAs a tap hide the merged reads, and the
      // asm reads' common wait measured 5 % slower there at D = 9)
      float2 v[IC];
      lds_read_b64_n<IC>(xc, v);
#pragma unroll
      for (int i = 0; i < IC; ++i) mac(acc, v[i], tv[i]);
    } else {
#pragma unroll
      for (int i = 0; i < IC; ++i) mac(acc, xc[i], tv[i]);
    }
  }
  OutT accs[1] = {acc};
  if (!finite_out(acc)) ascending_fixup<TapT, InT, NoPad, false, 1>(lds, p, D, tid, accs);
  float2* ex = reinterpret_cast<float2*>(lds + NG);
  tile_epilogue<MODE, OutT, 1, WG>(p, out0, accs, ex);
}

// ------------------------------------------------------------------------------------------------
// Kernel 3: generic fallback (any D, any T, any alignment): one output per thread straight from
// global memory (L1/L2 absorb the overlap). Used only where the tiled kernels do not apply.
// In FM mode each thread also computes the next FIR output.
// ------------------------------------------------------------------------------------------------
template <class TapT, class InT, int MODE>
__device__ __forceinline__ typename Product<TapT, InT>::type fir_point(const FirParams& p, uint64_t k) {
  using OutT = typename Product<TapT, InT>::type;
  const InT* __restrict__ in = reinterpret_cast<const InT*>(p.in);
  const TapT* __restrict__ taps = reinterpret_cast<const TapT*>(p.taps);
  OutT acc;
  set_zero(acc);
  const uint64_t s0 = k * p.D;
  for (uint32_t i = 0; i < p.T; ++i) {
    auto x = to_lds_sample(in[s0 + i]);
    if constexpr (MODE != kModeFir) {
      x = nco_mix(x, p.nco_n0 + (uint32_t)(s0 + i), p.nco_inc);
    }
    mac(acc, x, taps[i]);
  }
  return acc;
}

template <class TapT, class InT, int MODE>
__global__ __launch_bounds__(256) void k_fir_generic(FirParams p) {
  using OutT = typename Product<TapT, InT>::type;
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= p.N) return;
  if constexpr (MODE == kModeFir || MODE == kModeIq) {
    reinterpret_cast<OutT*>(p.out)[k] = fir_point<TapT, InT, MODE>(p, k);
  } else if constexpr (MODE == kModeAm) {
    reinterpret_cast<float*>(p.out)[k] = am_env(fir_point<TapT, InT, MODE>(p, k));
  } else {
    const float2 y0 = fir_point<TapT, InT, MODE>(p, k);
    const float2 y1 = fir_point<TapT, InT, MODE>(p, k + 1);
    reinterpret_cast<float*>(p.out)[k] = fm_disc(y0, y1, p.fm_gain);
  }
}

// ------------------------------------------------------------------------------------------------
// Kernel 1y: the same tile on the matrix cores (FIR mode, real taps, complex input, D = 4), an
// alternative core kept as a tuning variant (gsdrxFirFCVariant 13).
// v_mfma_f32_4x4x1_16b_f32 is 16 independent 4x4 outer products per wave instruction: block b of a
// wave holds lanes 4b..4b+3, A[i] comes from lane 4b+i, B[j] from lane 4b+j and D[i][j] lands in
// VGPR i of lane 4b+j. With
//     A[i] = t[kappa - D*i]                  (the tap row i needs at step kappa),
//     B[j] = x[D*(k0 + 4L) + kappa], L = 4b+j (lane L's own input stream),
// accumulator C[i] of lane L sums t[kappa - D*i] * x[D*(k0 + 4L + i) + (kappa - D*i)] over
// kappa = 0 .. 3D+T-1: output k0 + 4L + i with its taps in ascending order (zero outside [0, T)).
// f32 MFMA is an exact fmaf chain, so the outputs are bit-identical to the oracle's and the generic
// kernel's ascending-tap fmaf loop. Each lane reads its window sequentially from LDS (one
// ds_read_b128 per two steps); re and im are two accumulator chains. The taps need no memory
// traffic in the loop: the A operand of block ABID can be broadcast to all 16 blocks (CBSZ = 4) and
// every block needs the same taps, so one VGPR carries the taps of 16 consecutive steps: lane 4b+i
// of tap register c holds t[16c + b - D*i], and step 16c + b runs with ABID = b. MAXSEG registers
// cover 16*MAXSEG steps (3D + T of them are needed). Staging, tile geometry and epilogue are the
// polyphase kernel's (R = 4 outputs per lane).
// ------------------------------------------------------------------------------------------------
typedef float gsdr_mf4 __attribute__((ext_vector_type(4)));

// steps 2g and 2g + 1 of a segment (granule g): ABID must be an immediate
template <int G>
__device__ __forceinline__ void mfma_bc_granule(float tv, const float4& w, gsdr_mf4& cre, gsdr_mf4& cim) {
  cre = __builtin_amdgcn_mfma_f32_4x4x1f32(tv, w.x, cre, 4, 2 * G, 0);
  cim = __builtin_amdgcn_mfma_f32_4x4x1f32(tv, w.y, cim, 4, 2 * G, 0);
  cre = __builtin_amdgcn_mfma_f32_4x4x1f32(tv, w.z, cre, 4, 2 * G + 1, 0);
  cim = __builtin_amdgcn_mfma_f32_4x4x1f32(tv, w.w, cim, 4, 2 * G + 1, 0);
}
template <int... G>
__device__ __forceinline__ void mfma_bc_segment(float tv, const float4 (&w)[8], gsdr_mf4& cre, gsdr_mf4& cim,
                                                std::integer_sequence<int, G...>) {
  (mfma_bc_granule<G>(tv, w[G], cre, cim), ...);
}

template <int WG, int MAXSEG, bool VEC, bool NT, int ABL = 0>
__global__ __launch_bounds__(WG) void k_fir_mfma_bc(FirParams p) {
  constexpr int D = 4, R = 4;
  using Geo = TileGeo<float2, D, R, WG>;
  static_assert(Geo::SG == 8 && Geo::PAD == 1, "lane stream layout: 16 steps per 9-granule segment");
  extern __shared__ __attribute__((aligned(16))) float4 lds[];
  const float2* __restrict__ in = reinterpret_cast<const float2*>(p.in);
  const uint64_t out0 = (uint64_t)blockIdx.x * p.tile_stride;
  const uint64_t S0 = out0 * D;
  const uint32_t nk = 3u * D + p.T;             // steps that meet a tap
  const uint32_t nseg = (nk + 15u) / 16u;       // <= MAXSEG (checked by the launcher)
  const uint32_t NG = (D * (Geo::KT - R) + 16u * nseg) / 2;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const float* __restrict__ taps = reinterpret_cast<const float*>(p.taps);
  float tv[MAXSEG];
#pragma unroll
  for (int c = 0; c < MAXSEG; ++c) {
    const uint32_t i = 16u * c + (lane >> 2) - D * (lane & 3u);  // wraps (>= T) below zero
    tv[c] = i < p.T ? taps[i] : 0.0f;
  }
  if constexpr (ABL != 2) stage_tile<float2, Geo, WG, VEC, NT>(lds, in, S0, NG, p, MixNone{});
  __syncthreads();

  const float4* __restrict__ seg = lds + tid * Geo::SGP;
  gsdr_mf4 cre = {0.f, 0.f, 0.f, 0.f}, cim = cre;
#pragma unroll
  for (int c = 0; c < MAXSEG; ++c) {
    if ((uint32_t)c < nseg) {
      float4 w[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) w[g] = seg[c * Geo::SGP + g];
      mfma_bc_segment(tv[c], w, cre, cim, std::make_integer_sequence<int, 8>{});
    }
  }
  float2 acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = make_float2(cre[r], cim[r]);
  if constexpr (ABL == 0) {
    if (!all_finite(acc)) ascending_fixup<float, float2, Geo, true, R>(lds, p, D, tid * R, acc);
  }
  tile_epilogue<kModeFir, float2, R, WG, NT>(p, out0, acc, nullptr);
}

}  // namespace gsdr
