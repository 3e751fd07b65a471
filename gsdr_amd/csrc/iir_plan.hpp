// gsdr-mi355x: what one IIR call (iir.hip) launches and where its workspace lives, as a pure function of the
// call's size: no HIP, so it can be compiled and checked on the host alone.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gsdr {
namespace iir {

constexpr int kChunk = 32;  // samples per level-0 chunk (>= the largest P)
constexpr int kGroup = 64;  // scan elements per group = one wave, one element per lane
constexpr int kMaxLevels = 8;
constexpr uint64_t kTileSampleBytes = 128 * kChunk * sizeof(float);  // chunk-pass tile: 128 real / 64 complex chunks
constexpr int kRestGroups = 16;        // a level with at most this many groups joins the single-workgroup kernel
constexpr uint64_t kUpperE2 = 4 * 64;  // level-2 elements k_iir_scan_upper scans in every workgroup

struct ScanPlan {
  // level k has E[k] elements: E[0] chunks, E[k+1] = ceil(E[k] / kGroup), until one group remains (level `levels`)
  int levels;
  uint64_t E[kMaxLevels + 1];
  // workspace, byte offsets: per level the elements (tails / aggregates) and their start states, the tables
  // T[level][r] = M_level^r (table_bytes each), the entry state (the history buffers are rewritten at the end) and
  // the tails pass's copy of the caller's input history for the final pass
  size_t elems[kMaxLevels + 1], starts[kMaxLevels + 1];
  size_t tables, table_bytes, s0, xh_copy, bytes;
  uint64_t ntiles;  // chunk-pass tiles, one workgroup each
  // route: levels [lowest, rest) take a launch per sweep (lowest = 1 when level 0 is fused into the chunk passes) and
  // levels [rest, levels] one single-workgroup launch (k_iir_scan_rest); or, with `upper`, level 1's up-sweep and
  // then k_iir_scan_upper (levels >= 2 and level 1's down-sweep; it reads the tables of levels 1..3)
  int lowest, rest;
  bool upper;
};

// P = compiled state size, acc_bytes = sizeof(double or double2), sample_bytes = sizeof(float or float2), fused =
// level 0 of the scan runs inside the chunk passes. False: refused (too many levels, or tiles for one grid).
inline bool scan_plan(uint64_t n, int P, size_t acc_bytes, size_t sample_bytes, bool fused, ScanPlan* p) {
  p->levels = 0;
  p->E[0] = (n + kChunk - 1) / kChunk;
  for (; p->E[p->levels] > kGroup; ++p->levels) {
    if (p->levels == kMaxLevels) return false;
    p->E[p->levels + 1] = (p->E[p->levels] + kGroup - 1) / kGroup;
  }
  const uint64_t ts = kTileSampleBytes / sample_bytes;
  p->ntiles = (n + ts - 1) / ts;
  if (p->ntiles >= 0x7fffffffull) return false;
  size_t bytes = 0;
  for (int k = 0; k <= p->levels; ++k) {
    p->elems[k] = bytes;
    p->starts[k] = bytes + p->E[k] * P * acc_bytes;
    bytes += 2 * p->E[k] * P * acc_bytes;
  }
  p->tables = bytes;
  p->table_bytes = (size_t)kGroup * P * P * sizeof(double);
  p->s0 = p->tables + (p->levels + 1) * p->table_bytes;
  p->xh_copy = p->s0 + P * acc_bytes;
  p->bytes = p->xh_copy + (P * sample_bytes + 15) / 16 * 16;
  p->lowest = p->rest = fused ? 1 : 0;
  while (p->rest <= p->levels && (p->E[p->rest] + kGroup - 1) / kGroup > (uint64_t)kRestGroups) ++p->rest;
  p->upper = fused && p->levels >= 2 && p->E[2] <= kUpperE2;
  return true;
}

}  // namespace iir
}  // namespace gsdr
