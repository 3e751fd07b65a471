// gsdr-mi355x: what one rational-resampler call (resample.hip) launches, as a pure function of the filter's shape
// and the call's size: no HIP, so it can be compiled and checked on the host alone.
//
// L = interpolation, M = decimation, T = taps. Output m's window starts at s(m) = q + m M of the zero-stuffed
// stream and its first real sample is input[ceil(s(m) / L)]; it reads at most ceil(T / L) samples from there.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gsdr {
namespace resample {

constexpr uint32_t kR = 8;                        // outputs per thread of k_resample_tile (independent fmaf chains)
constexpr uint32_t kMaxWG = 256, kMinWG = 64;     // its workgroup sizes: a tile is KT = kR * WG outputs
constexpr uint32_t kGenericWG = 256;              // k_resample_generic: one output per thread
constexpr uint64_t kLdsBudget = 64 * 1024;        // per workgroup, the FIR engine's (fir_dispatch.hpp kMaxTileLds)
constexpr uint64_t kMaxLaunchThreads = 0xffffffffull;  // blocks * threads of one launch stay within 32 bits

enum Route { kRouteTile = 0, kRouteGeneric = 1 };

struct Plan {
  int route;
  uint32_t wg;         // threads per workgroup
  uint32_t kt;         // outputs per workgroup
  uint32_t span;       // tile route: input samples a tile may need, for the worst tile start
  uint32_t lds_bytes;  // tile route: dynamic LDS of the launch
  uint64_t blocks;     // workgroups, covering [0, N) in order
};

constexpr uint64_t ceil_div64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
constexpr uint64_t round16(uint64_t bytes) { return (bytes + 15) / 16 * 16; }

// The span and LDS bytes of a tile of kt outputs; false when the tiled kernel cannot hold it.
//   * ceil((s + (kt-1) M) / L) - ceil(s / L) <= ceil((kt-1) M / L) for every s, and the last output reads
//     ceil(T / L) samples at most;
//   * the samples are staged at their offset inside a 16-byte granule of global memory (so whole granules move with
//     16-byte loads whatever the pointer's alignment): up to granule - 1 samples of slack in front; the same for the
//     taps (up to 3 floats);
//   * the kernel's per-output index r0 + k M (r0 < L, k < kt) is formed in 32 bits.
inline bool tile_fits(uint64_t L, uint64_t M, uint64_t T, size_t sample_bytes, uint32_t kt, uint32_t* span,
                      uint32_t* lds_bytes) {
  if (L >= (1ull << 31) || M >= (1ull << 31) || (uint64_t)kt * M >= (1ull << 31)) return false;
  if (T > kLdsBudget / sizeof(float)) return false;
  const uint64_t s = ceil_div64((uint64_t)(kt - 1) * M, L) + ceil_div64(T, L);
  const uint64_t per_granule = 16 / sample_bytes;
  if (s > kLdsBudget / sample_bytes) return false;
  const uint64_t bytes = round16((s + per_granule - 1) * sample_bytes) + round16((T + 3) * sizeof(float));
  if (bytes > kLdsBudget) return false;
  *span = (uint32_t)s;
  *lds_bytes = (uint32_t)bytes;
  return true;
}

// The route and tile of a filter shape: a function of (L, M, T, sample type) alone, so every cut of one stream
// into calls runs the same kernel. The largest tile that fits, else the generic kernel. (Preferring tiles within
// 32 KB, for more workgroups a CU, was measured slower: DESIGN.md section 3.9.)
inline void route_of(uint64_t L, uint64_t M, uint64_t T, size_t sample_bytes, Plan* p) {
  for (uint32_t wg = kMaxWG; wg >= kMinWG; wg /= 2) {
    if (tile_fits(L, M, T, sample_bytes, kR * wg, &p->span, &p->lds_bytes)) {
      p->route = kRouteTile;
      p->wg = wg;
      p->kt = kR * wg;
      return;
    }
  }
  p->route = kRouteGeneric;
  p->wg = kGenericWG;
  p->kt = kGenericWG;
  p->span = 0;
  p->lds_bytes = 0;
}

// L, M >= 1, n >= 1 outputs. False: refused (more workgroups than one launch takes).
inline bool plan(uint64_t L, uint64_t M, uint64_t T, size_t sample_bytes, uint64_t n, Plan* p) {
  route_of(L, M, T, sample_bytes, p);
  p->blocks = ceil_div64(n, p->kt);
  return p->blocks <= kMaxLaunchThreads / p->wg;
}

// phase + (n - 1) M + T, the zero-stuffed samples the call spans; false when it does not fit in 63 bits.
inline bool stuffed_extent(uint64_t phase, uint64_t M, uint64_t T, uint64_t n, uint64_t* extent) {
  uint64_t a = 0;
  if (n == 0 || __builtin_mul_overflow(n - 1, M, &a) || __builtin_add_overflow(a, phase, &a) ||
      __builtin_add_overflow(a, T, &a) || (a >> 63) != 0) {
    return false;
  }
  *extent = a;
  return true;
}

}  // namespace resample
}  // namespace gsdr
