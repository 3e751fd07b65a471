// gsdr-mi355x: 256-point constellation modulate / demodulate.
// Replaces reference src/qpsk256.cu (tables :25-71, modulate :74-151, demodulate :154-259,
// wrappers :262-431; header qpsk256.h:125-230).
//
// Tables are built on the host (qpsk256_tables.hpp), in float, with exactly the reference's expressions, and
// uploaded per device on the caller's stream. Each workgroup copies the 2 KiB table it needs into LDS, so
// lookups are LDS reads rather than divergent constant-cache accesses. The demodulation decision -- the
// reference's own rule, bit for bit -- is qpsk256_decide.hpp.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "awgn.hpp"
#include "gsdr/gsdr_ext.h"
#include "gsdr/qpsk256.h"
#include "launch.hpp"
#include "qpsk256_decide.hpp"
#include "qpsk256_tables.hpp"

namespace gsdr {

constexpr int kCBlock = 256;
constexpr int kCSym = 16;  // symbols per thread

// [0] rectangular, [1] circular; per device (module globals are per-device copies).
__constant__ float2 c_qpsk256_tables[2][256];

// the circular table's candidate lists (qpsk256_tables.hpp), built by gsdrQpsk256InitConstellation
__device__ CircCells g_circ_cells;

using C256Streams = StreamPtrs<4>;

__device__ __forceinline__ void load_table(float2* lds_tab, uint32_t type) {
  const float2* src = c_qpsk256_tables[type == 0 ? 0 : 1];
  for (uint32_t i = threadIdx.x; i < 256; i += kCBlock) lds_tab[i] = src[i];
  __syncthreads();
}

__global__ __launch_bounds__(kCBlock) void k_c256_mod(C256Streams st, uint32_t n, uint32_t type) {
  __shared__ float2 tab[256];
  load_table(tab, type);
  const uint8_t* __restrict__ in = reinterpret_cast<const uint8_t*>(st.in[blockIdx.y]);
  float2* __restrict__ out = reinterpret_cast<float2*>(st.out[blockIdx.y]);
  // a full, aligned block: lane t of slot q handles symbol pair q * kCBlock + t (coalesced 1 KB stores)
  const uint64_t base = (uint64_t)blockIdx.x * kCBlock * kCSym;
  if (base + kCBlock * kCSym <= n && (reinterpret_cast<uintptr_t>(in) & 1u) == 0 &&
      (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    const uint16_t* pin = reinterpret_cast<const uint16_t*>(in + base);
    float4* o = reinterpret_cast<float4*>(out + base);
    uint32_t pr[kCSym / 2];
#pragma unroll
    for (int q = 0; q < kCSym / 2; ++q) pr[q] = pin[q * kCBlock + threadIdx.x];
#pragma unroll
    for (int q = 0; q < kCSym / 2; ++q) {
      const float2 p0 = tab[pr[q] & 0xffu];
      const float2 p1 = tab[pr[q] >> 8];
      o[q * kCBlock + threadIdx.x] = make_float4(p0.x, p0.y, p1.x, p1.y);
    }
    return;
  }
  const uint64_t s0 = base + (uint64_t)threadIdx.x * kCSym;
  if (s0 >= n) return;
  if (s0 + kCSym <= n && (reinterpret_cast<uintptr_t>(in + s0) & 15u) == 0 &&
      (reinterpret_cast<uintptr_t>(out + s0) & 15u) == 0) {
    const uint4 w = *reinterpret_cast<const uint4*>(in + s0);
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    float4* o = reinterpret_cast<float4*>(out + s0);
#pragma unroll
    for (int q = 0; q < kCSym / 2; ++q) {
      const uint32_t word = words[q / 2];
      const float2 p0 = tab[(word >> (16 * (q & 1))) & 0xffu];
      const float2 p1 = tab[(word >> (16 * (q & 1) + 8)) & 0xffu];
      o[q] = make_float4(p0.x, p0.y, p1.x, p1.y);
    }
  } else {
    for (int k = 0; k < kCSym; ++k) {
      if (s0 + k < n) out[s0 + k] = tab[in[s0 + k]];
    }
  }
}

// Modulate + counter-based AWGN (gsdrxQpsk256ModulateAwgn; awgn.hpp). One Philox block serves three
// symbols, so a lane takes six consecutive symbols a step: two blocks when the first absolute index is a
// multiple of 3 (R3 = firstSymbolIndex % 3, uniform, a template parameter so every slot and block index
// is a compile-time constant), three otherwise. A wave's 384 noisy symbols (3 KB) go through LDS so that
// each of its three 16-byte store instructions writes 1 KB contiguous: stored straight from the lanes
// (48-byte lane stride) they ran at about half the copy rate, which bound the kernel once the normals
// were cheap (the write-heavy maps of section 3.6 showed the same).
constexpr int kAwgnSym = 6;    // symbols per lane per step
constexpr int kAwgnSteps = 3;  // steps per workgroup (1, 2 and 6 measured slower)
constexpr uint32_t kAwgnWaveSyms = 64u * kAwgnSym;
constexpr uint32_t kAwgnBlockSyms = kCBlock * kAwgnSym * kAwgnSteps;

// LDS hand-off between the lanes of one wave: without it the compiler, reasoning per thread, may
// forward a lane's own earlier LDS store to its later load past another lane's store.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// This lane's six symbols of a step as loaded (a 4-byte and a 2-byte load), kept so until the step needs them:
// nothing waits for the loads before then.
struct SymRaw {
  uint32_t lo;     // symbols 0..3
  uint32_t hi;     // symbols 4, 5 (low 16 bits)
  uint32_t shift;  // bytes to drop (the last symbols of the input, loaded from an address moved back)
};

// The symbols are loaded one step AHEAD: step 0's with the tables, step it + 1's before step it's stores. Vector
// loads and stores share one in-order counter, so a load issued after a step's stores could only be waited for
// together with them (an HBM write's whole latency, each step); and issued before the Philox blocks, a step's
// loads are in flight while they are computed. To keep the compiler's wait counts exact the loads have no branch
// around them: every lane loads 6 bytes from min(s, n - 6) (so no load leaves the input; unaligned loads are
// fine on this part) and drops the bytes before s. SMALL (n < 6, chosen by the launcher): byte loads.
// DEMOD (gsdrxQpsk256ModulateAwgnDemodulate, rectangular table): the same kernel also demodulates every noisy symbol
// it writes, from the registers that hold it -- the decision of gsdrQpsk256Demodulate's rectangular kernel on the
// same float values, bit for bit -- and writes the decisions to `dec`: the round trip in one pass, without reading
// the 134 MB of noisy symbols back.
// firstBlk = firstSymbolIndex / 3: with every lane's first symbol a multiple of 6 from the launch's first, its
// first Philox block is firstBlk + s / 3 (no 64-bit division per lane).
template <int R3, bool SMALL, bool DEMOD = false>
__global__ __launch_bounds__(kCBlock) __attribute__((amdgpu_waves_per_eu(8))) void k_c256_mod_awgn(const uint8_t* __restrict__ in, float2* __restrict__ out,
                                                            uint32_t n, uint32_t type, float sigma, uint64_t seed,
                                                            uint64_t firstBlk, uint8_t* __restrict__ dec = nullptr) {
  __shared__ float2 tab[256];
  __shared__ AwgnLds ntab;
  __shared__ float4 stage[kCBlock / 64][kAwgnWaveSyms / 2];  // per wave: 384 symbols as 192 float4
  __shared__ float levp[DEMOD ? kRectLevels : 1];  // DEMOD: the demodulator's padded level arrays
  constexpr int NB = R3 == 0 ? 2 : 3;  // Philox blocks touched by six symbols starting at slot R3
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  float4* __restrict__ st = stage[wv];
  // 16-byte aligned output: the wave's stores can be whole float4s (every wave step starts at a multiple
  // of 384 symbols from `out`)
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const uint64_t base = (uint64_t)blockIdx.x * kAwgnBlockSyms;
  auto wave_first = [&](int it) { return base + (uint64_t)kAwgnWaveSyms * ((uint32_t)it * (kCBlock / 64) + wv); };
  auto load_syms = [&](int it) {
    SymRaw r;
    const uint64_t s = wave_first(it) + (uint64_t)kAwgnSym * lane;
    if constexpr (SMALL) {
      uint32_t b[kAwgnSym];
#pragma unroll
      for (int j = 0; j < kAwgnSym; ++j) b[j] = s + j < n ? in[s + j] : 0u;
      r.lo = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      r.hi = b[4] | (b[5] << 8);
      r.shift = 0;
    } else {
      const uint64_t sl = s < (uint64_t)n - kAwgnSym ? s : (uint64_t)n - kAwgnSym;
      __builtin_memcpy(&r.lo, in + sl, 4);
      uint16_t h;
      __builtin_memcpy(&h, in + sl + 4, 2);
      r.hi = h;
      r.shift = (uint32_t)min<uint64_t>(s - sl, kAwgnSym);
    }
    return r;
  };
  const AwgnRegs treg = awgn_fetch_table();
  const float2 trow = c_qpsk256_tables[type == 0 ? 0 : 1][threadIdx.x];
  SymRaw raw = load_syms(0);
  awgn_store_table(ntab, treg);
  tab[threadIdx.x] = trow;
  float lim = -1.0f, scale = 0.0f;
  if constexpr (DEMOD) {  // k_c256_demod<0>'s decider
    rect_fill_levels(levp, c_qpsk256_tables[0]);
    rect_limits(c_qpsk256_tables[0][255].x, lim, scale);
  }
  __syncthreads();  // publishes the tables
  // DEMOD: k_c256_demod<0>'s decisions of a lane's six noisy symbols (the reference's cuCabsf argmin, bit for
  // bit): the quick per-axis decision inline for all six, then -- for the ~1e-4 of symbols within its margin of a
  // decision boundary, beyond 4|a| or NaN -- the careful path one symbol at a time (unrolled six times over, its
  // 3 x 3 search had held the kernel at 5 waves a SIMD)
  auto decide6 = [&](const float2 (&y)[kAwgnSym], uint32_t (&d)[kAwgnSym]) {
    uint32_t slow = 0;
#pragma unroll
    for (int j = 0; j < kAwgnSym; ++j) slow |= demod_rect_quick(y[j], lim, scale, d[j]) ? 0u : 1u << j;
    if (__builtin_expect(slow != 0, 0)) {
#pragma unroll 1
      for (int j = 0; j < kAwgnSym; ++j) {
        if (!((slow >> j) & 1u)) continue;
        float2 r = y[0];
#pragma unroll
        for (int i = 1; i < kAwgnSym; ++i) r = j == i ? y[i] : r;  // (a select chain: y stays in registers)
        uint32_t k = demod_rect_fast(levp, levp + kRectLyp, r, lim, scale);
        if (k >= 256u) {  // demod_exhaustive's loop, inline: its call (the ABI's saved registers) cost 17 VGPRs
          float best = INFINITY;
          k = 0;
#pragma unroll 1
          for (uint32_t i = 0; i < 256; ++i) rank_step(ref_dist(r, tab[i]), i, best, k);
        }
#pragma unroll
        for (int i = 0; i < kAwgnSym; ++i) d[i] = j == i ? k : d[i];
      }
    }
  };
  // the noisy symbols of step it (the lane's six, from `raw`)
  auto step_outputs = [&](int it, float2 (&y)[kAwgnSym]) {
    // (first + s) / 3 with s = base + 384 (it * waves + wv) + 6 lane, every term a multiple of 3
    const uint32_t s3 = (uint32_t)blockIdx.x * (kAwgnBlockSyms / 3u) + (kAwgnWaveSyms / 3u) * ((uint32_t)it * (kCBlock / 64) + wv) +
                        2u * lane;
    const uint64_t b0 = firstBlk + s3;
    uint8_t sym[kAwgnSym];
    {
      uint32_t w[NB][4];
#pragma unroll
      for (int b = 0; b < NB; ++b) awgn_block_words(seed, b0 + b, w[b]);
      const uint64_t v6 = ((uint64_t)raw.hi << 32 | raw.lo) >> (8u * raw.shift);
#pragma unroll
      for (int j = 0; j < kAwgnSym; ++j) sym[j] = (uint8_t)(v6 >> (8 * j));
#pragma unroll
      for (int j = 0; j < kAwgnSym; ++j) {
        const float2 g = awgn_slot_main(ntab, w[(R3 + j) / 3], (R3 + j) % 3);
        const float2 p = tab[sym[j]];
        y[j] = make_float2(p.x + sigma * g.x, p.y + sigma * g.y);
      }
    }
    // a lane whose blocks hold a tail component (~4e-4 of the lanes: its outputs hold a NaN, awgn.hpp) redoes
    // them exactly, regenerating its blocks (so they do not stay live in the common path)
    if (__builtin_expect(awgn_has_tail(y), 0)) {
      uint32_t w[NB][4];
#pragma unroll
      for (int b = 0; b < NB; ++b) awgn_block_words(seed, b0 + b, w[b]);
#pragma unroll
      for (int j = 0; j < kAwgnSym; ++j) {
        const float2 g = awgn_slot(ntab, w[(R3 + j) / 3], (R3 + j) % 3, seed, b0 + (R3 + j) / 3);
        const float2 p = tab[sym[j]];
        y[j] = make_float2(p.x + sigma * g.x, p.y + sigma * g.y);
      }
    }
    // the next step's symbols, before this step's stores
    if (it + 1 < kAwgnSteps) raw = load_syms(it + 1);
  };
  // Whole wave steps to an aligned output: a wave's 384 noisy symbols go through LDS so each of its three store
  // instructions writes 1 KB. (Their own loop: with the per-symbol stores of the other steps in the same loop,
  // the compiler's wait for the next step's symbols had to cover this step's stores as well.)
  // Step 0 is peeled off the loop, so that the loop is entered as its back edge enters it -- the next symbols' two
  // loads, then the three stores -- and the wait for the symbols leaves the stores in flight.
  auto fast_step = [&](int it) {
    const uint64_t ws = wave_first(it);  // wave's first
    float2 y[kAwgnSym];
    step_outputs(it, y);
#pragma unroll
    for (int q = 0; q < kAwgnSym / 2; ++q) {
      st[lane * 3 + q] = make_float4(y[2 * q].x, y[2 * q].y, y[2 * q + 1].x, y[2 * q + 1].y);
    }
    wave_sync();
    float4* __restrict__ o = reinterpret_cast<float4*>(out + ws);
#pragma unroll
    for (int q = 0; q < kAwgnSym / 2; ++q) o[q * 64 + lane] = st[q * 64 + lane];
    wave_sync();  // the next step's LDS writes come after every lane's reads
    if constexpr (DEMOD) {  // the lane's six decisions: three 2-byte stores (s even, dec 2-byte aligned)
      uint32_t d[kAwgnSym];
      decide6(y, d);
      uint16_t* __restrict__ d2 = reinterpret_cast<uint16_t*>(dec + ws + (uint64_t)kAwgnSym * lane);
#pragma unroll
      for (int q = 0; q < kAwgnSym / 2; ++q) d2[q] = (uint16_t)(d[2 * q] | (d[2 * q + 1] << 8));
    }
  };
  const bool dec_even = !DEMOD || (reinterpret_cast<uintptr_t>(dec) & 1u) == 0;
  auto fast = [&](int it) { return aligned && dec_even && wave_first(it) + kAwgnWaveSyms <= n; };  // wave-uniform
  int it = 0;
  if (fast(0)) {
    fast_step(0);
#pragma unroll 1
    for (it = 1; it < kAwgnSteps && fast(it); ++it) fast_step(it);
  }
  // the rest (the input's last, partial wave step; an output only 8-byte aligned): one store a symbol
#pragma unroll 1
  for (; it < kAwgnSteps; ++it) {
    const uint64_t ws = wave_first(it);
    if (ws >= n) break;
    const uint64_t s = ws + (uint64_t)kAwgnSym * lane;  // this lane's first symbol (a multiple of 6)
    float2 y[kAwgnSym];
    step_outputs(it, y);
    uint32_t d[kAwgnSym] = {};
    if constexpr (DEMOD) decide6(y, d);
#pragma unroll
    for (int j = 0; j < kAwgnSym; ++j) {
      if (s + j < n) {
        out[s + j] = y[j];
        if constexpr (DEMOD) dec[s + j] = (uint8_t)d[j];
      }
    }
  }
}


// TYPE 0: rectangular table (per-axis fast path); TYPE 1: circular table (per-cell candidate lists).
// Both fall back to the exhaustive search for inputs their fast path does not cover.
template <int TYPE>
__global__ __launch_bounds__(kCBlock) void k_c256_demod(C256Streams st, uint32_t n) {
  // the rectangular levels, padded with +inf (demod_rect_fast), at the start of the table's LDS block: their
  // reads then need no base add (ds_read2_b32 offsets reach 1 KB)
  __shared__ float2 tab_lev[kRectLevels / 2 + 256];
  float* const levp = reinterpret_cast<float*>(tab_lev);
  float2* const tab = tab_lev + kRectLevels / 2;
  // the circular cell lists: an LDS image of g_circ_cells (cell words and the distinct lists)
  __shared__ uint4 ccells[TYPE == 0 ? 1 : sizeof(CircCells) / 16];
  const uint16_t* cword = reinterpret_cast<const CircCells*>(ccells)->cell;
  const uint8_t* clists = reinterpret_cast<const CircCells*>(ccells)->lists;
  // circular full tiles: the tile's decisions, and per wave the symbols whose search is not finished
  // after the first four candidates (see below)
  __shared__ uint16_t otile[TYPE == 0 ? 1 : kCBlock * kCSym / 2];
  __shared__ uint16_t cq[TYPE == 0 ? 1 : kCBlock / 64][TYPE == 0 ? 1 : 64 * kCSym];
  const float2* tsrc = c_qpsk256_tables[TYPE];
  for (uint32_t i = threadIdx.x; i < 256; i += kCBlock) tab[i] = tsrc[i];
  if constexpr (TYPE == 0) rect_fill_levels(levp, tsrc);
  if (TYPE != 0 && g_circ_cells.R > 0.0f) {  // the circular candidate lists, into LDS
    // 16-byte copies, all issued before the first LDS store (22.5 KB: six loads a lane; a per-entry
    // 2-byte copy loop waited on each load in turn and cost ~5 % of the kernel)
    constexpr uint32_t kWords = sizeof(CircCells) / 16, kFull = kWords / kCBlock;
    const uint4* src = reinterpret_cast<const uint4*>(&g_circ_cells);
    uint4 w[kFull], wt = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t it = kFull * kCBlock + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < kFull; ++k) w[k] = src[k * kCBlock + threadIdx.x];
    if (it < kWords) wt = src[it];
#pragma unroll
    for (uint32_t k = 0; k < kFull; ++k) ccells[k * kCBlock + threadIdx.x] = w[k];
    if (it < kWords) ccells[it] = wt;
  }
  __syncthreads();
  const float2* __restrict__ in = reinterpret_cast<const float2*>(st.in[blockIdx.y]);
  uint8_t* __restrict__ out = reinterpret_cast<uint8_t*>(st.out[blockIdx.y]);
  float lim = -1.0f, scale = 0.0f, cR = 0.0f, inv_cs = 0.0f;
  if constexpr (TYPE == 0) {
    rect_limits(tab[255].x, lim, scale);
  } else {
    cR = g_circ_cells.R;
    inv_cs = g_circ_cells.inv_cs;
  }
  auto demod = [&](float2 r) -> uint32_t {
    if constexpr (TYPE == 0) {
      uint32_t k;
      if (demod_rect_quick(r, lim, scale, k)) return k;
      k = demod_rect_fast(levp, levp + kRectLyp, r, lim, scale);
      return k < 256u ? k : demod_exhaustive(tab, r);
    } else {
      uint32_t wc;
      if (circ_cell(cword, cR, inv_cs, r, wc)) return circ_decide(clists, tab, r, wc);
      return demod_exhaustive(tab, r);
    }
  };
  // circular, first step: a cell whose candidate list holds a single point decides the symbol without
  // any distance; false for longer lists and outside the grid
  auto circ_first = [&](float2 r, uint32_t& idx) -> bool {
    uint32_t wc;
    if (!circ_cell(cword, cR, inv_cs, r, wc)) return false;
    idx = wc & 0xffu;  // the point of a one-point cell; the low byte of an offset otherwise (overwritten)
    return (wc >> 12) == 1u;
  };
  // grid-stride over 4096-symbol tiles, so the LDS tables are staged once per workgroup
  const uint32_t tiles = (uint32_t)((n + (uint64_t)kCBlock * kCSym - 1) / ((uint64_t)kCBlock * kCSym));
  const bool aligned = (reinterpret_cast<uintptr_t>(in) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 1u) == 0;
  // rectangular: one tile per workgroup (the launcher starts `tiles` workgroups), so the loop ends after
  // its first pass and nothing stays live around it (91 -> 79 VGPRs); circular: grid-stride, so the cell
  // lists are staged into LDS once per workgroup
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += (TYPE == 0 ? tiles : gridDim.x)) {
    const uint64_t base = (uint64_t)tile * kCBlock * kCSym;
    if (TYPE == 1 && aligned && base + kCBlock * kCSym <= n) {
      // Circular full tile. The candidate lists average 1.6 entries but the longest list in a wave is
      // 8-9, so walking each symbol's list in lockstep leaves most lanes idle. Here every symbol first
      // looks up its cell (single-point cells are decided there); the wave's other symbols go to a
      // wave queue in LDS, which its 64 lanes then drain one symbol each (whole list or exhaustive).
      const float4* src = reinterpret_cast<const float4*>(in + base);
      float4 v[kCSym / 2];
#pragma unroll
      for (int q = 0; q < kCSym / 2; ++q) v[q] = src[q * kCBlock + threadIdx.x];
      const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
      uint16_t* qw = cq[TYPE == 0 ? 0 : w];
      uint32_t qn = 0;  // wave-uniform
#pragma unroll
      for (int q = 0; q < kCSym / 2; ++q) {
        const uint32_t pair = q * kCBlock + threadIdx.x;
        uint32_t i0 = 0, i1 = 0;
        const bool d0 = circ_first(make_float2(v[q].x, v[q].y), i0);
        const bool d1 = circ_first(make_float2(v[q].z, v[q].w), i1);
        otile[pair] = (uint16_t)(i0 | (i1 << 8));
        const uint64_t m0 = __ballot(!d0), m1 = __ballot(!d1);
        const uint64_t below = (1ull << lane) - 1ull;
        if (!d0) qw[qn + __popcll(m0 & below)] = (uint16_t)(2u * pair);
        qn += (uint32_t)__popcll(m0);
        if (!d1) qw[qn + __popcll(m1 & below)] = (uint16_t)(2u * pair + 1u);
        qn += (uint32_t)__popcll(m1);
      }
      wave_sync();  // the queue and the first-step decisions come from other lanes of the wave
      uint8_t* ob = reinterpret_cast<uint8_t*>(otile);
      for (uint32_t i = lane; i < qn; i += 64) {
        const uint32_t pos = qw[i];
        ob[pos] = (uint8_t)demod(in[base + pos]);
      }
      wave_sync();
      uint16_t* dst = reinterpret_cast<uint16_t*>(out + base);
#pragma unroll
      for (int q = 0; q < kCSym / 2; ++q) dst[q * kCBlock + threadIdx.x] = otile[q * kCBlock + threadIdx.x];
    } else if (aligned && base + kCBlock * kCSym <= n) {
      // full, aligned tile: lane t of slot q reads symbol pair q * kCBlock + t (coalesced 1 KB loads)
      const float4* src = reinterpret_cast<const float4*>(in + base);
      uint16_t* dst = reinterpret_cast<uint16_t*>(out + base);
      float4 v[kCSym / 2];
#pragma unroll
      for (int q = 0; q < kCSym / 2; ++q) v[q] = src[q * kCBlock + threadIdx.x];
#pragma unroll
      for (int q = 0; q < kCSym / 2; ++q) {
        const uint32_t i0 = demod(make_float2(v[q].x, v[q].y));
        const uint32_t i1 = demod(make_float2(v[q].z, v[q].w));
        dst[q * kCBlock + threadIdx.x] = (uint16_t)(i0 | (i1 << 8));
      }
    } else {
      // last tile or misaligned pointers: one symbol at a time, thread t owning symbols s0 .. s0 + 15
      const uint64_t s0 = base + (uint64_t)threadIdx.x * kCSym;
      for (int k = 0; k < kCSym; ++k) {
        if (s0 + k < n) out[s0 + k] = (uint8_t)demod(in[s0 + k]);
      }
    }
  }
}

// circular demodulation workgroups per stream (grid-stride): 4 resident per CU x 256 CUs (37 KB LDS)
constexpr uint32_t kCircBlocks = 1024;

static hipError_t c256_launch(bool modulate, const C256Streams& st, int nstreams, uint32_t n, uint32_t type,
                              int32_t device, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!streams_non_null(st, nstreams)) return hipErrorInvalidValue;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  const uint32_t blocks = symbol_blocks(n, kCSym, kCBlock);
  const dim3 grid(blocks, (uint32_t)nstreams);
  if (modulate) {
    k_c256_mod<<<grid, dim3(kCBlock), 0, stream>>>(st, n, type);
  } else {
    // rectangular: one workgroup per tile; circular: one resident round of workgroups (cell lists,
    // decision tile and wave queues take 37 KB of LDS, 4 workgroups per CU) striding over the tiles
    const dim3 dgrid(type == 0 ? blocks : std::min<uint32_t>(blocks, kCircBlocks), (uint32_t)nstreams);
    if (type == 0) {
      k_c256_demod<0><<<dgrid, dim3(kCBlock), 0, stream>>>(st, n);
    } else {
      k_c256_demod<1><<<dgrid, dim3(kCBlock), 0, stream>>>(st, n);
    }
  }
  return launch_status();
}

}  // namespace gsdr

GSDR_C_LINKAGE hipError_t gsdrQpsk256InitConstellation(uint32_t constellationType, float amplitude,
                                                       int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  gsdr::DeviceScope scope(cudaDevice);
  if (scope.status() != hipSuccess) return scope.status();
  float2 table[256];
  gsdr::build_table(constellationType, amplitude, table);
  const size_t offset = (constellationType == 0 ? 0 : 1) * sizeof(table);
  hipError_t st = hipMemcpyToSymbolAsync(HIP_SYMBOL(gsdr::c_qpsk256_tables), table, sizeof(table), offset,
                                         hipMemcpyHostToDevice, cudaStream);
  if (st != hipSuccess) return st;
  static thread_local gsdr::CircCells cells;  // host staging (~38 KiB): waited for below
  if (constellationType != 0) {
    try {
      gsdr::build_cells(table, &cells);
    } catch (...) {  // allocation failure: no lookup, the exhaustive search stays exact
      cells.R = 0.0f;
    }
    st = hipMemcpyToSymbolAsync(HIP_SYMBOL(gsdr::g_circ_cells), &cells, sizeof(cells), 0, hipMemcpyHostToDevice,
                                cudaStream);
  }
  // the host table lives on this stack frame: wait for the copies before returning -- on every path
  // once the first copy was issued, so a failed second copy cannot leave the first reading a dead frame
  const hipError_t sync = hipStreamSynchronize(cudaStream);
  return st != hipSuccess ? st : sync;
}

GSDR_C_LINKAGE hipError_t gsdrQpsk256Modulate(const uint8_t* inputBytes, hipFloatComplex* output, uint32_t numSymbols,
                                              float amplitude, uint32_t constellationType, int32_t cudaDevice,
                                              hipStream_t cudaStream) GSDR_NO_EXCEPT {
  (void)amplitude;  // scale is fixed by InitConstellation, as in the reference (qpsk256.cu:74-101)
  return gsdr::c256_launch(true, {{inputBytes}, {output}}, 1, numSymbols, constellationType, cudaDevice, cudaStream);
}

namespace gsdr {
// gsdrxQpsk256ModulateAwgn, and with dec != nullptr the fused round trip of gsdrxQpsk256ModulateAwgnDemodulate
// (rectangular table only; the caller checks)
static hipError_t mod_awgn_launch(const uint8_t* inputBytes, hipFloatComplex* output, uint8_t* dec, uint32_t numSymbols,
                                  uint32_t constellationType, float sigma, uint64_t seed, uint64_t firstSymbolIndex,
                                  hipStream_t cudaStream) {
  const uint32_t blocks = (uint32_t)ceil_div<uint64_t>(numSymbols, kAwgnBlockSyms);
  float2* out = reinterpret_cast<float2*>(output);
  const uint64_t blk = firstSymbolIndex / 3u;
  using Kernel = void (*)(const uint8_t*, float2*, uint32_t, uint32_t, float, uint64_t, uint64_t, uint8_t*);
  static constexpr Kernel kKernels[2][3][2] = {  // [DEMOD][R3][SMALL]
      {{k_c256_mod_awgn<0, false, false>, k_c256_mod_awgn<0, true, false>},
       {k_c256_mod_awgn<1, false, false>, k_c256_mod_awgn<1, true, false>},
       {k_c256_mod_awgn<2, false, false>, k_c256_mod_awgn<2, true, false>}},
      {{k_c256_mod_awgn<0, false, true>, k_c256_mod_awgn<0, true, true>},
       {k_c256_mod_awgn<1, false, true>, k_c256_mod_awgn<1, true, true>},
       {k_c256_mod_awgn<2, false, true>, k_c256_mod_awgn<2, true, true>}}};
  const Kernel kernel = kKernels[dec != nullptr][firstSymbolIndex % 3u][numSymbols < (uint32_t)kAwgnSym];
  kernel<<<dim3(blocks), dim3(kCBlock), 0, cudaStream>>>(inputBytes, out, numSymbols, constellationType, sigma, seed, blk,
                                                         dec);
  return launch_status();
}
}  // namespace gsdr

GSDR_C_LINKAGE hipError_t gsdrxQpsk256ModulateAwgn(const uint8_t* inputBytes, hipFloatComplex* output,
                                                    uint32_t numSymbols, uint32_t constellationType, float sigma,
                                                    uint64_t seed, uint64_t firstSymbolIndex, int32_t cudaDevice,
                                                    hipStream_t cudaStream) GSDR_NO_EXCEPT {
  if (numSymbols == 0) return hipSuccess;
  if (inputBytes == nullptr || output == nullptr || !(sigma >= 0.0f) || !(sigma < INFINITY)) {
    return hipErrorInvalidValue;
  }
  gsdr::DeviceScope scope(cudaDevice);
  if (scope.status() != hipSuccess) return scope.status();
  return gsdr::mod_awgn_launch(inputBytes, output, nullptr, numSymbols, constellationType, sigma, seed, firstSymbolIndex,
                               cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxQpsk256ModulateAwgnDemodulate(const uint8_t* inputBytes, hipFloatComplex* noisySymbols,
                                                              uint8_t* outputBytes, uint32_t numSymbols,
                                                              uint32_t constellationType, float sigma, uint64_t seed,
                                                              uint64_t firstSymbolIndex, int32_t cudaDevice,
                                                              hipStream_t cudaStream) GSDR_NO_EXCEPT {
  if (numSymbols == 0) return hipSuccess;
  if (inputBytes == nullptr || noisySymbols == nullptr || outputBytes == nullptr || !(sigma >= 0.0f) ||
      !(sigma < INFINITY)) {
    return hipErrorInvalidValue;
  }
  if (constellationType != 0) {  // circular table: the two calls (the cell lists do not fit beside the AWGN tables)
    const hipError_t e = gsdrxQpsk256ModulateAwgn(inputBytes, noisySymbols, numSymbols, constellationType, sigma, seed,
                                                  firstSymbolIndex, cudaDevice, cudaStream);
    if (e != hipSuccess) return e;
    return gsdrQpsk256Demodulate(noisySymbols, outputBytes, numSymbols, constellationType, cudaDevice, cudaStream);
  }
  gsdr::DeviceScope scope(cudaDevice);
  if (scope.status() != hipSuccess) return scope.status();
  return gsdr::mod_awgn_launch(inputBytes, noisySymbols, outputBytes, numSymbols, 0, sigma, seed, firstSymbolIndex,
                               cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrQpsk256Demodulate(const hipFloatComplex* input, uint8_t* outputBytes,
                                                uint32_t numSymbols, uint32_t constellationType, int32_t cudaDevice,
                                                hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::c256_launch(false, {{input}, {outputBytes}}, 1, numSymbols, constellationType, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrQpsk256Modulate4x(const uint8_t* inputBytes0, const uint8_t* inputBytes1,
                                                const uint8_t* inputBytes2, const uint8_t* inputBytes3,
                                                hipFloatComplex* output0, hipFloatComplex* output1,
                                                hipFloatComplex* output2, hipFloatComplex* output3,
                                                uint32_t numSymbols, float amplitude, uint32_t constellationType,
                                                int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  (void)amplitude;
  return gsdr::c256_launch(true, {{inputBytes0, inputBytes1, inputBytes2, inputBytes3}, {output0, output1, output2, output3}},
                           4, numSymbols, constellationType, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrQpsk256Demodulate4x(const hipFloatComplex* input0, const hipFloatComplex* input1,
                                                  const hipFloatComplex* input2, const hipFloatComplex* input3,
                                                  uint8_t* outputBytes0, uint8_t* outputBytes1, uint8_t* outputBytes2,
                                                  uint8_t* outputBytes3, uint32_t numSymbols,
                                                  uint32_t constellationType, int32_t cudaDevice,
                                                  hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::c256_launch(false, {{input0, input1, input2, input3},
                                   {outputBytes0, outputBytes1, outputBytes2, outputBytes3}},
                           4, numSymbols, constellationType, cudaDevice, cudaStream);
}
