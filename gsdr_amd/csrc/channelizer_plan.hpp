// gsdr-mi355x: what one channelizer call (channelizer.hip) launches, as a pure function of the bank's shape and the
// call's size: no HIP, so it can be compiled and checked on the host alone.
//
// M = channels (a power of two in [2, 64]), D = decimation, T = taps. Output time m reads input[m D, m D + T). The
// tile's samples sit in LDS as float2 whatever the sample format (int8 I/Q is converted while it is staged), so the
// plan does not depend on the format: the two formats run the same tiles and give the same bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gsdr {
namespace channelizer {

constexpr uint32_t kMinChannels = 2, kMaxChannels = 64;
constexpr uint32_t kMaxWG = 256, kMinWG = 64;     // k_channelizer_tile: one output time per thread, KT = WG
constexpr uint32_t kGenericWG = 256;              // k_channelizer_generic: one output time per thread
constexpr uint64_t kLdsBudget = 64 * 1024;        // per workgroup, the FIR engine's (fir_dispatch.hpp kMaxTileLds)
constexpr uint64_t kLdsSample = 8;                // a staged sample: float2
constexpr uint64_t kMaxLaunchThreads = 0xffffffffull;  // blocks * threads of one launch stay within 32 bits

enum Route { kRouteTile = 0, kRouteGeneric = 1 };

struct Plan {
  int route;
  uint32_t wg;         // threads per workgroup
  uint32_t kt;         // output times per workgroup
  uint32_t span;       // tile route: input samples of a full tile, (kt - 1) D + T
  uint32_t lds_bytes;  // tile route: dynamic LDS of the launch (the padded span)
  uint64_t blocks;     // workgroups, covering [0, N) in order
};

constexpr uint64_t ceil_div64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
constexpr uint64_t round16(uint64_t bytes) { return (bytes + 15) / 16 * 16; }

constexpr bool valid_channels(uint64_t M) {
  return M >= kMinChannels && M <= kMaxChannels && (M & (M - 1)) == 0;
}

// LDS rows of D samples are one sample apart when D is even: lane l of a wave reads sample l D + i, 2 D banks from
// its neighbour (a D-way conflict of ds_read_b64's 32-lane groups); with the pad the lane stride is 2 (D + 1) banks
// and D + 1 is odd, so the 32 lanes of a group fall on the 32 distinct bank pairs. D = 1 is conflict-free as it is.
constexpr uint32_t row_pad(uint32_t D) { return D % 2 == 0 ? 1u : 0u; }
constexpr uint64_t padded(uint64_t j, uint32_t D) { return j + j / D * row_pad(D); }  // LDS index of tile sample j

// The tiled kernel exists for the critically sampled and the 2x oversampled bank.
constexpr bool tile_shape(uint64_t M, uint64_t D) { return D == M || 2 * D == M; }

// The span and LDS bytes of a tile of kt output times; false when the tiled kernel cannot hold it.
inline bool tile_fits(uint64_t D, uint64_t T, uint32_t kt, uint32_t* span, uint32_t* lds_bytes) {
  if (T > kLdsBudget / kLdsSample) return false;
  const uint64_t s = (uint64_t)(kt - 1) * D + T;  // kt <= 256, D <= 64: no overflow
  if (s == 0) {
    *span = 0;
    *lds_bytes = 0;
    return true;
  }
  const uint64_t bytes = round16((padded(s - 1, (uint32_t)D) + 1) * kLdsSample);
  if (bytes > kLdsBudget) return false;
  *span = (uint32_t)s;
  *lds_bytes = (uint32_t)bytes;
  return true;
}

// The route and tile of a bank: a function of (M, D, T) alone, so every cut of one stream into calls runs the same
// kernel. The largest workgroup whose tile fits (D = 64 or long taps shrink it), else the generic kernel.
inline void route_of(uint64_t M, uint64_t D, uint64_t T, Plan* p) {
  if (tile_shape(M, D)) {
    for (uint32_t wg = kMaxWG; wg >= kMinWG; wg /= 2) {
      if (tile_fits(D, T, wg, &p->span, &p->lds_bytes)) {
        p->route = kRouteTile;
        p->wg = wg;
        p->kt = wg;
        return;
      }
    }
  }
  p->route = kRouteGeneric;
  p->wg = kGenericWG;
  p->kt = kGenericWG;
  p->span = 0;
  p->lds_bytes = 0;
}

// M valid, D >= 1, n >= 1 output times. False: refused (more workgroups than one launch takes).
inline bool plan(uint64_t M, uint64_t D, uint64_t T, uint64_t n, Plan* p) {
  route_of(M, D, T, p);
  p->blocks = ceil_div64(n, p->kt);
  return p->blocks <= kMaxLaunchThreads / p->wg;
}

// (n - 1) D + T input samples and M n outputs; false when either does not fit in 63 bits.
inline bool extents(uint64_t M, uint64_t D, uint64_t T, uint64_t n, uint64_t* need) {
  uint64_t a = 0, b = 0;
  if (n == 0 || __builtin_mul_overflow(n - 1, D, &a) || __builtin_add_overflow(a, T, &a) || (a >> 63) != 0 ||
      __builtin_mul_overflow(n, M, &b) || (b >> 63) != 0) {
    return false;
  }
  *need = a;
  return true;
}

}  // namespace channelizer
}  // namespace gsdr
