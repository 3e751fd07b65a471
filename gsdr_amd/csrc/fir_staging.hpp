// gsdr-mi355x, FIR engine: a tile's input span staged from HBM into the padded LDS layout, mixed on the way in.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fir_nco.hpp"
#include "fir_plan.hpp"
#include "fir_samples.hpp"

namespace gsdr {

// ------------------------------------------------------------------------------------------------
// Tile geometry
// ------------------------------------------------------------------------------------------------
template <class InT, int D, int R, int WG>
struct TileGeo {
  static constexpr int G = SampleT<InT>::kPerGranule;
  static_assert((R * D) % G == 0, "a thread segment must be whole granules");
  static constexpr int SG = firplan::tile_sg(G, D, R);  // granules per thread segment
  static constexpr int PAD = firplan::tile_pad(SG);     // odd lane stride -> conflict-free ds_read_b128
  static constexpr int SGP = SG + PAD;
  static constexpr int KT = WG * R;                     // outputs per tile
  static constexpr int ROUT = R;                        // outputs per segment
  __host__ __device__ static constexpr uint32_t padded(uint32_t g) { return firplan::tile_padded(g, SG); }
};

// 16 bytes = G consecutive samples starting at s; samples at or past L read as zero.
template <class InT, bool VEC>
__device__ __forceinline__ float4 load_granule(const InT* __restrict__ in, uint64_t s, uint64_t L) {
  constexpr int G = SampleT<InT>::kPerGranule;
  // (an anchored chain's first tile starts before the call's first sample: its local indices below 0 arrive
  // wrapped, and those granules -- whole granules, since tiles start at even samples -- read as zero)
  if ((int64_t)s < 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if constexpr (std::is_same<InT, Iq8>::value) {
    if (VEC && s + 2 <= L) return iq8x2_granule(*reinterpret_cast<const uint32_t*>(in + s));
    float2 a = make_float2(0.0f, 0.0f), b = a;
    if (s < L) a = to_lds_sample(in[s]);
    if (s + 1 < L) b = to_lds_sample(in[s + 1]);
    return make_float4(a.x, a.y, b.x, b.y);
  } else if (VEC && s + G <= L) {
    return *reinterpret_cast<const float4*>(in + s);
  }
  float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if constexpr (G == 2) {
    if (s < L) {
      const float2 a = reinterpret_cast<const float2*>(in)[s];
      r.x = a.x;
      r.y = a.y;
    }
    if (s + 1 < L) {
      const float2 b = reinterpret_cast<const float2*>(in)[s + 1];
      r.z = b.x;
      r.w = b.y;
    }
  } else {
    const float* f = reinterpret_cast<const float*>(in);
    if (s < L) r.x = f[s];
    if (s + 1 < L) r.y = f[s + 1];
    if (s + 2 < L) r.z = f[s + 2];
    if (s + 3 < L) r.w = f[s + 3];
  }
  return r;
}

// granules per staging batch: the largest divisor of the per-thread count that is at most 8
constexpr int staging_batch(int bpt) {
  for (int b = 8; b > 1; --b) {
    if (bpt % b == 0) return b;
  }
  return 1;
}

// Tile body by LDS-DMA (global_load_lds_dwordx4: HBM -> LDS with no VGPR round trip and no ds_write).
// One wave instruction fills 64 consecutive LDS slots; the padded layout is kept by choosing each
// lane's SOURCE granule (slot s holds granule s - s / SGP of its segment; pad slots are skipped with
// the lane masked off). Returns false when the tile does not qualify (then nothing was issued): only unmixed
// complex samples do (MIXED: the tile has an NCO mixer).
template <class InT, class Geo, int WG, bool MIXED, bool NT>
__device__ __forceinline__ bool stage_body_dma(float4* __restrict__ lds, const InT* __restrict__ in, uint64_t S0) {
  if constexpr (!std::is_same<InT, float2>::value || MIXED) {
    return false;
  } else {
    constexpr int BODY = Geo::SG * (Geo::KT / Geo::ROUT);  // body granules
    constexpr int SLOTS = BODY / Geo::SG * Geo::SGP;
    static_assert(SLOTS % 64 == 0 && (SLOTS / 64) % (WG / 64) == 0, "body slots must split into wave instructions");
    constexpr int PER_WAVE = SLOTS / 64 / (WG / 64);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(in + S0);
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const uint32_t base = (uint32_t)(i * (WG / 64) + w) * 64u;  // wave-uniform first slot
      const uint32_t sl = base + lane;
      const uint32_t within = sl % Geo::SGP;
      if (within < (uint32_t)Geo::SG) {
        const uint32_t g = (sl / Geo::SGP) * Geo::SG + within;
        __builtin_amdgcn_global_load_lds((const void*)(src + g), (void __attribute__((address_space(3)))*)(lds + base),
                                         16, 0, NT ? 2 : 0);
      }
    }
    return true;
  }
}

// The next history of a streaming call, copied by workgroup 0 (it writes the stream's spare buffer, which no
// tile reads). Split so that it costs the workgroup no round trip of its own: each thread loads its sample
// before the tile's loads are issued (stream_history_load) and stores it after the staging, whose waits
// have covered that load (stream_history_store). Histories longer than the workgroup (T + D > WG samples)
// copy the rest there with a plain loop.
template <class InT>
struct HistSample {
  InT v;
  bool on;
};
template <class InT>
__device__ __forceinline__ HistSample<InT> stream_history_load(const FirParams& p) {
  HistSample<InT> h{};
  h.on = p.hist_out != nullptr && blockIdx.x == 0 && threadIdx.x < p.hist_n;
  if (h.on) {
    const int64_t i = p.hist_from + (int64_t)threadIdx.x;  // chunk offset
    h.v = i < 0 ? reinterpret_cast<const InT*>(p.hist)[(int64_t)p.hist_len + i]
                : reinterpret_cast<const InT*>(p.in)[i - p.in_off];
  }
  return h;
}
template <class InT>
__device__ __forceinline__ void stream_history_store(const FirParams& p, const HistSample<InT>& h) {
  if (p.hist_out == nullptr || blockIdx.x != 0) return;
  InT* __restrict__ dst = reinterpret_cast<InT*>(p.hist_out);
  if (h.on) dst[threadIdx.x] = h.v;
  for (uint64_t j = threadIdx.x + blockDim.x; j < p.hist_n; j += blockDim.x) {
    const int64_t i = p.hist_from + (int64_t)j;
    dst[j] = i < 0 ? reinterpret_cast<const InT*>(p.hist)[(int64_t)p.hist_len + i]
                   : reinterpret_cast<const InT*>(p.in)[i - p.in_off];
  }
}

// The first halo granule of a tile, loaded ahead of the body's loads so that both arrive in one round trip (after
// the body, it was a second dependent round trip per tile: what a short call's few tiles wait for). The load is
// one predicated instruction with the raw word(s) kept until the body has been staged: a bounds-checked
// load_granule there made the compiler wait for it on the spot (its branches merge through register copies).
template <class InT>
struct HaloRaw {
  using type = float4;
};
template <>
struct HaloRaw<Iq8> {
  using type = uint32_t;
};
template <class InT, bool VEC>
struct HaloPre {
  // (left indeterminate where nothing is loaded -- get() never returns it then. A zero there, or
  // __builtin_nondeterministic_value, which the compiler also materialises as zero, cost a register copy right
  // behind the load, i.e. a wait for it)
  typename HaloRaw<InT>::type raw;
  uint64_t s;
  uint32_t g;
  bool fast;
  __device__ __forceinline__ HaloPre(uint64_t S0, uint32_t g0, uint32_t NG, uint64_t L)
      : s(S0 + (uint64_t)g0 * SampleT<InT>::kPerGranule), g(g0) {
    fast = VEC && g0 < NG && (int64_t)s >= 0 && s + SampleT<InT>::kPerGranule <= L;
  }
  // issued right after the body's first batch of loads (issued before them, it drew a full wait ahead of them)
  __device__ __forceinline__ void issue(const InT* __restrict__ in) {
    if (fast) raw = *reinterpret_cast<const typename HaloRaw<InT>::type*>(in + s);
  }
  // the granule (only for g < NG). The empty asm re-defines the raw registers here, so the register copies the
  // allocator makes of the loaded value come after this point and the wait for the load with them, not right
  // behind the load.
  __device__ __forceinline__ float4 get(const InT* __restrict__ in, uint64_t L) const {
    typename HaloRaw<InT>::type r = raw;
    if constexpr (std::is_same<InT, Iq8>::value) {
      asm volatile("" : "+v"(r));
      return fast ? iq8x2_granule(r) : load_granule<InT, VEC>(in, s, L);
    } else {
      gsdr_f32x4 q{r.x, r.y, r.z, r.w};
      asm volatile("" : "+v"(q));
      return fast ? make_float4(q[0], q[1], q[2], q[3]) : load_granule<InT, VEC>(in, s, L);
    }
  }
};

// One staging batch: SB granules WG apart from granule g0 of an aligned base (int8 I/Q words or 16-byte quads, plain
// or non-temporal), all loaded before the first is converted.
template <class InT, int SB, int WG, bool NT>
__device__ __forceinline__ void load_batch(float4 (&v)[SB], const InT* __restrict__ base, uint32_t g0) {
  if constexpr (std::is_same<InT, Iq8>::value) {
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(base);
    uint32_t w[SB];
#pragma unroll
    for (int k = 0; k < SB; ++k) w[k] = NT ? __builtin_nontemporal_load(src + g0 + k * WG) : src[g0 + k * WG];
#pragma unroll
    for (int k = 0; k < SB; ++k) v[k] = iq8x2_granule(w[k]);
  } else {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(base);
#pragma unroll
    for (int k = 0; k < SB; ++k) {
      if constexpr (NT) {
        v[k] = load16_nt(src + g0 + k * WG);
      } else {
        v[k] = src[g0 + k * WG];
      }
    }
  }
}

// The same batch for body rows row0 .. row0 + SB - 1 of an aligned, wholly readable tile of 16-byte quads (granule
// (row0 + k) WG + tid): each row's address is a wave-uniform 64-bit base (scalar adds) plus the thread's one 32-bit
// byte offset, the same register for every row (global_load ... vgpr, sgpr pair). Rows are WG * 16 bytes apart,
// past the 12-bit immediate offset, and written as base[g0 + k WG] the compiler adds k WG * 16 to the thread's 64-bit
// address in VALU pairs (v_add_co, a wait state, v_addc) row by row. The empty asm keeps each row base a scalar of
// its own.
typedef __attribute__((address_space(1))) gsdr_f32x4 GlobalQuad;
typedef __attribute__((address_space(1))) char GlobalByte;
template <int SB, int WG, bool NT>
__device__ __forceinline__ void load_rows(float4 (&v)[SB], const float4* __restrict__ base, int row0, uint32_t tid) {
  const uint32_t boff = tid * 16u;  // the thread's byte offset in every row
#pragma unroll
  for (int k = 0; k < SB; ++k) {
    // (the row base goes through the asm as an integer and comes back as a global-memory pointer: a laundered
    // generic pointer would make these flat loads)
    uint64_t rb = reinterpret_cast<uint64_t>(base + (row0 + k) * WG);
    asm("" : "+s"(rb));
    const GlobalQuad* __restrict__ g = reinterpret_cast<const GlobalQuad*>(reinterpret_cast<const GlobalByte*>(rb) + boff);
    const gsdr_f32x4 q = NT ? __builtin_nontemporal_load(g) : *g;
    v[k] = make_float4(q.x, q.y, q.z, q.w);
  }
}

// A streaming call's first tile, which reaches into the stream's history (only that tile: the history is shorter
// than one window). Local sample s (counted from output 0's window start, `in` = chunk + in_off) is chunk sample
// s + in_off; the ones before the chunk come from the history, samples at or past L read as zero. Sample by sample,
// in batches of 8 granules a thread whose loads are all issued before the first is used (one granule at a time, this
// tile had waited on every load in turn and ran ~1 us longer than the call's other tiles).
template <class InT, class Geo, int WG, class Mix>
__device__ __forceinline__ void stage_history(float4* __restrict__ lds, const InT* __restrict__ in, uint64_t S0,
                                              uint32_t NG, const FirParams& p, Mix& m) {
  constexpr int G = Geo::G;
  const uint32_t tid = threadIdx.x;
  constexpr int B = 8;
  const InT* __restrict__ hist = reinterpret_cast<const InT*>(p.hist);
  for (uint32_t g0 = 0; g0 < NG; g0 += B * WG) {
    InT v[B][G];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const uint32_t g = g0 + (uint32_t)b * WG + tid;
#pragma unroll
      for (int c = 0; c < G; ++c) {
        const uint64_t s = S0 + (uint64_t)g * G + (uint64_t)c;
        const int64_t i = (int64_t)s + p.in_off;
        if (g < NG && s < p.L) {
          v[b][c] = i < 0 ? hist[(int64_t)p.hist_len + i] : in[s];
        } else {
          set_zero(v[b][c]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const uint32_t g = g0 + (uint32_t)b * WG + tid;
      if (g >= NG) break;
      float4 w;
      if constexpr (G == 2) {
        const float2 a = to_lds_sample(v[b][0]), c = to_lds_sample(v[b][1]);
        w = make_float4(a.x, a.y, c.x, c.y);
      } else {
        w = make_float4(v[b][0], v[b][1], v[b][2], v[b][3]);
      }
      lds[Geo::padded(g)] = m.next(w, S0 + (uint64_t)g * G, g0 + (uint32_t)b * WG > 0);
    }
  }
}

// Stage granules [0, NG) of the tile starting at global sample S0 into LDS (padded layout), each mixed by `m` on
// the way in. The first SG*WG granules (the tile body) are loaded fully unrolled so every HBM load is in flight
// before the first LDS write; the remaining halo granules follow in a short strided loop.
// SH (complex or int8 I/Q samples): the input is one sample off its aligned granule load (complex: 8 bytes
// off 16; int8 I/Q: 2 bytes off 4) at every tile start. The tile body is then loaded as aligned 16-byte granules
// starting one sample early, and each loaded pair is split over two LDS granules (second half of slot g - 1, first
// half of slot g); the halo re-writes the body's last slot whole.
template <class InT, class Geo, int WG, bool VEC, bool NT = false, bool DMA = false, int SH = 0, class Mix>
__device__ __forceinline__ void stage_tile(float4* __restrict__ lds, const InT* __restrict__ in, uint64_t S0,
                                           uint32_t NG, const FirParams& p, Mix m) {
  constexpr int G = Geo::G;
  constexpr bool MIXED = !std::is_same<Mix, MixNone>::value;
  static_assert(!MIXED || G == 2, "NCO modes take complex samples");
  // tile body granules per staging thread (Geo::KT / R output segments of SG granules over WG threads)
  constexpr int BPT = Geo::SG * (Geo::KT / Geo::ROUT) / WG;
  static_assert(BPT * WG == Geo::SG * (Geo::KT / Geo::ROUT), "tile body must split evenly over the threads");
  // at most 8 granules (128 B) in flight per lane: bounds the staging registers for large segments
  constexpr int SB = staging_batch(BPT);
  static_assert(BPT % SB == 0, "segment granules must split into whole staging batches");
  // the halo from tile granule g on, a granule at a time
  auto stage_halo = [&](uint32_t g) __attribute__((always_inline)) {
    for (; g < NG; g += WG) {
      const uint64_t s = S0 + (uint64_t)g * G;
      lds[Geo::padded(g)] = m.next(load_granule<InT, VEC>(in, s, p.L), s);
    }
  };
  if (p.hist != nullptr && (int64_t)S0 + p.in_off < 0) {  // uniform: the tile starts in the stream's history
    stage_history<InT, Geo, WG>(lds, in, S0, NG, p, m);
    return;
  }
  const uint32_t tid = threadIdx.x;
  // wave-uniform: is the whole staged span readable? (not the first tile of an anchored call starting inside its
  // cell, not the last tile)
  const bool whole = VEC && (int64_t)S0 >= 0 && (S0 + (uint64_t)NG * G <= p.L);
  if constexpr (SH != 0 && std::is_same<InT, float>::value) {
    // real samples SH (1..3) floats off 16-byte alignment (4-byte aligned): aligned 16-byte loads from
    // SH samples early; loaded quad g holds the last SH samples of granule g - 1 and the first 4 - SH of
    // granule g, written as two partial-granule LDS stores (8-byte aligned pieces). The halo re-writes
    // the body's last granule whole, as for complex input.
    static_assert(!VEC && SH > 0 && SH < 4, "shifted real staging: 1..3 floats off 16-byte alignment");
    // (a tile less than SH samples past the start of the caller's buffer would load samples before it --
    // inside its first 16-byte block, so it cannot fault, but it is out of bounds: that tile takes the
    // per-granule loads below instead. The buffer starts at `in - in_off` on the streaming path.)
    if ((int64_t)S0 + p.in_off >= (int64_t)SH && S0 + (uint64_t)NG * G <= p.L) {
      float* __restrict__ l1 = reinterpret_cast<float*>(lds);
#pragma unroll
      for (int b0 = 0; b0 < BPT; b0 += SB) {
        float4 v[SB];
        load_batch<InT, SB, WG, NT>(v, in + S0 - SH, b0 * WG + tid);  // 16-byte aligned
#pragma unroll
        for (int k = 0; k < SB; ++k) {
          const uint32_t g = (b0 + k) * WG + tid;
          float* __restrict__ lo = l1 + 4 * Geo::padded(g);  // granule g
          if constexpr (SH == 2) {
            if (g > 0) *reinterpret_cast<float2*>(l1 + 4 * Geo::padded(g - 1) + 2) = make_float2(v[k].x, v[k].y);
            *reinterpret_cast<float2*>(lo) = make_float2(v[k].z, v[k].w);
          } else if constexpr (SH == 1) {
            if (g > 0) l1[4 * Geo::padded(g - 1) + 3] = v[k].x;
            *reinterpret_cast<float2*>(lo) = make_float2(v[k].y, v[k].z);
            lo[2] = v[k].w;
          } else {
            if (g > 0) {
              float* __restrict__ pv = l1 + 4 * Geo::padded(g - 1);
              pv[1] = v[k].x;
              *reinterpret_cast<float2*>(pv + 2) = make_float2(v[k].y, v[k].z);
            }
            lo[0] = v[k].w;
          }
        }
      }
      stage_halo(BPT * WG - 1 + tid);
      return;
    }
  } else if constexpr (SH != 0) {
    static_assert((std::is_same<InT, float2>::value || std::is_same<InT, Iq8>::value) && !VEC && SH == 1,
                  "shifted staging is for 8-byte-aligned complex or 2-byte-aligned int8 I/Q input");
    // (a tile starting at the caller's buffer, chunk = in - in_off, would load the sample before it)
    if ((int64_t)S0 + p.in_off >= 1 && S0 + (uint64_t)NG * G <= p.L) {
      auto prev = m.begin_shifted();
      float2* __restrict__ l2 = reinterpret_cast<float2*>(lds);
#pragma unroll
      for (int b0 = 0; b0 < BPT; b0 += SB) {
        float4 v[SB];
        load_batch<InT, SB, WG, NT>(v, in + S0 - 1, b0 * WG + tid);  // complex: 16-byte aligned, int8 I/Q: 4-byte
#pragma unroll
        for (int k = 0; k < SB; ++k) {
          const uint32_t g = (b0 + k) * WG + tid;
          const float4 w = m.shifted_row(v[k], b0 + k, prev);
          if (g > 0) l2[2 * Geo::padded(g - 1) + 1] = make_float2(w.x, w.y);
          l2[2 * Geo::padded(g)] = make_float2(w.z, w.w);
        }
      }
      m.shifted_halo(prev);
      stage_halo(BPT * WG - 1 + tid);  // (its first granule rewrites the body's last slot whole)
      return;
    }
  }
  if constexpr (DMA) {
    if (whole && stage_body_dma<InT, Geo, WG, MIXED, NT>(lds, in, S0)) {
      stage_halo(BPT * WG + tid);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      return;
    }
  }
  HaloPre<InT, VEC> halo(S0, BPT * WG + tid, NG, p.L);
  const uint32_t pbase = Geo::padded(tid);
  m.per_parity([&](auto odd) {
#pragma unroll
    for (int b0 = 0; b0 < BPT; b0 += SB) {
      float4 v[SB];
      if (whole) {
        if constexpr (!std::is_same<InT, Iq8>::value) {
          load_rows<SB, WG, NT>(v, reinterpret_cast<const float4*>(in + S0), b0, tid);
        } else {
          load_batch<InT, SB, WG, NT>(v, in + S0, b0 * WG + tid);
        }
      } else {
#pragma unroll
        for (int k = 0; k < SB; ++k) {
          v[k] = load_granule<InT, VEC>(in, S0 + (uint64_t)((b0 + k) * WG + tid) * G, p.L);
        }
      }
      if (b0 == 0) halo.issue(in);
#pragma unroll
      for (int k = 0; k < SB; ++k) {
        const uint32_t g = (b0 + k) * WG + tid;
        // padded(k * WG + tid) = padded(tid) + k * padded(WG) when whole segments fit a workgroup's row of
        // granules: a per-thread base plus an immediate offset per granule
        const uint32_t slot = (WG % Geo::SG == 0) ? pbase + (uint32_t)(b0 + k) * Geo::padded(WG) : Geo::padded(g);
        lds[slot] = m.row(v[k], b0 + k, odd);
      }
    }
  });
  if (halo.g < NG) lds[Geo::padded(halo.g)] = m.next(halo.get(in, p.L), halo.s);
  stage_halo(halo.g + WG);
}

// Wave-owned staging of a whole, aligned, unmixed tile of 16-byte quads (FIR mode; every tile of a long call but the
// last). stage_tile's map hands thread tid the granules k WG + tid, so every wave loads a share of every body row and
// no wave may read the tile before the slowest wave's last load has landed: a workgroup barrier. But wave w reads only
// the segments of its own 64 threads and the tap span after them -- tile granules [w B, w B + B + H), B = 64 SG its
// body share, H = NG - WG SG the tile's halo length. Here it stages exactly those, into the slots stage_tile would put
// them in: SG row-base loads a lane for its body share (load_rows on the wave's base) and one predicated load for the
// H granules that follow, issued with them, so that all arrive in one round trip. For the last wave those H are the
// tile's halo; for the others they are also the head of wave w + 1's body share, and both waves write them, the same
// bits to the same slots. A wave reads a slot only after its own write to it (wave_staged), so it never depends on its
// neighbour, and a neighbour's write under a read changes nothing. Private copies would need LDS for H more granules
// a wave, and the tile's size sets the occupancy. The following granules are read again soon after -- by the next wave,
// or as the next tile's body -- so theirs is a plain load, as the halo's always was, while the body's loads stream (NT).
// Returns false, with nothing issued, where this does not apply (uniform over the workgroup): a history tile, a tile
// that is not wholly readable, a tap span longer than one load a lane. The caller then stages with stage_tile.
template <class Geo, int WG, bool NT>
__device__ __forceinline__ bool stage_tile_wave(float4* __restrict__ lds, const float2* __restrict__ in, uint64_t S0,
                                                uint32_t NG, const FirParams& p) {
  constexpr int SG = Geo::SG, B = 64 * SG;
  static_assert(Geo::G == 2 && WG % 64 == 0 && 64 % SG == 0, "whole segments per wave row");
  if (p.hist != nullptr && (int64_t)S0 + p.in_off < 0) return false;
  if ((int64_t)S0 < 0 || S0 + (uint64_t)NG * Geo::G > p.L) return false;
  const uint32_t H = NG - (uint32_t)(WG * SG);
  if (H > 64u) return false;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float4* __restrict__ wb = reinterpret_cast<const float4*>(in + S0) + w * B;  // wave-uniform
  float4 v[SG];
  load_rows<SG, 64, NT>(v, wb, 0, lane);
  const bool follow = lane < H;
  float4 f[1];  // (left indeterminate where nothing is loaded, as HaloPre::raw)
  if (follow) load_rows<1, 64, false>(f, wb + B, 0, lane);
  float4* __restrict__ dst = lds + w * (64 * Geo::SGP) + Geo::padded(lane);
#pragma unroll
  for (int k = 0; k < SG; ++k) dst[k * (64 / SG) * Geo::SGP] = v[k];
  if (follow) dst[64 * Geo::SGP] = f[0];
  return true;
}

// The wave's own wait behind stage_tile_wave: its LDS writes are done, and no LDS read is moved above this point.
__device__ __forceinline__ void wave_staged() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace gsdr
