// gsdr-mi355x: what gsdrQpsk256InitConstellation computes on the host -- the 256-point table and the circular
// table's per-cell candidate lists. HIP-free (tests/test_qpsk256_tables.py compiles it into a host program), so
// it is templated on the point type P, two floats x, y: float2 in qpsk256.hip.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <vector>

namespace gsdr {

// Circular table: per-cell candidate lists over a kCellGrid^2 grid covering [-R, R)^2, built on the
// host by gsdrQpsk256InitConstellation. A point is listed for a cell when its distance to the cell is
// at most the smallest worst-case distance of any table point over the cell (plus a margin for float
// rounding), so every point that can win the argmin anywhere in the cell -- ties included -- is on the
// list, and the argmin over the list in index order is the exhaustive one -- for the squared distance
// and, with the near-tie re-ranking of the demodulation kernel, for the reference's cuCabsf rule.
// R == 0 disables the lookup.
// One 16-bit word per cell: length (bits 12-15) and, for a one-point list, the point itself (bits
// 0-11), else the offset of the list in `lists` (ascending indices). Neighbouring cells mostly share
// their lists, which are stored once: the circular table at any amplitude has 2,863 one-point cells
// and 6,353 longer lists of which 1,078 are distinct (3,293 bytes), so one cell lookup decides 87 % of
// noisy symbols with a single LDS load and the whole structure is 22.5 KB of LDS.
constexpr int kCellGrid = 96;
constexpr int kCellListBytes = 4096;  // 12-bit offsets
constexpr double kCellSpan = 1.3;  // grid half-width R = 1.3 * max |c|: noisy symbols stay on the grid
struct alignas(16) CircCells {
  float R;
  float inv_cs;  // kCellGrid / (2 R)
  uint16_t cell[kCellGrid * kCellGrid];
  uint8_t lists[kCellListBytes];
};

constexpr float kPiF = 3.14159265358979323846f;

// Host construction, float arithmetic in the reference's evaluation order (qpsk256.cu:33-34, 54-56, 64-67).
template <class P>
void build_table(uint32_t type, float amplitude, P* t) {
  static_assert(sizeof(P) == 2 * sizeof(float), "a point is two floats, x then y");
  if (type == 0) {
    for (int i = 0; i < 16; ++i) {
      for (int q = 0; q < 16; ++q) {
        const float I = ((float)i - 7.5f) / 7.5f * amplitude;
        const float Q = ((float)q - 7.5f) / 7.5f * amplitude;
        t[i * 16 + q] = P{I, Q};
      }
    }
    return;
  }
  static const int kPoints[8] = {1, 8, 16, 24, 32, 40, 48, 56};
  static const float kRadii[8] = {0.0f, 0.3f, 0.6f, 0.85f, 1.1f, 1.35f, 1.6f, 1.85f};
  int idx = 0;
  for (int c = 0; c < 8 && idx < 256; ++c) {
    const int points = kPoints[c] < 256 - idx ? kPoints[c] : 256 - idx;
    const float radius = kRadii[c] * amplitude;
    for (int p = 0; p < points && idx < 256; ++p) {
      const float angle = 2.0f * kPiF * (float)p / (float)points + ((float)c * 0.5f);
      t[idx++] = P{radius * cosf(angle), radius * sinf(angle)};
    }
  }
  while (idx < 256) {
    const float angle = 2.0f * kPiF * (float)idx / 256.0f;
    const float radius = amplitude * 0.95f;
    t[idx] = P{radius * cosf(angle), radius * sinf(angle)};
    ++idx;
  }
}

// Candidate lists for the circular table (see CircCells). Distances in double on the float table.
// Leaves cc->R == 0 (no lookup: the exhaustive search stays exact) for a degenerate table and for lists
// that do not fit the encoding.
template <class P>
void build_cells(const P* t, CircCells* cc) {
  double rmax = 0.0;
  for (int i = 0; i < 256; ++i) rmax = std::max(rmax, std::hypot((double)t[i].x, (double)t[i].y));
  cc->R = 0.0f;
  if (!(rmax > 0.0) || !std::isfinite(rmax)) return;  // degenerate table
  const float R = (float)(rmax * kCellSpan);
  const float inv_cs = (float)kCellGrid / (2.0f * R);
  const double cs = 1.0 / (double)inv_cs;
  const double margin = 1e-4 * rmax;  // >> float rounding of positions and distances
  int n = 0;
  std::map<std::vector<uint8_t>, int> seen;  // distinct lists -> offset
  std::vector<uint8_t> list;
  for (int iy = 0; iy < kCellGrid; ++iy) {
    for (int ix = 0; ix < kCellGrid; ++ix) {
      const double x0 = -(double)R + ix * cs, x1 = x0 + cs, y0 = -(double)R + iy * cs, y1 = y0 + cs;
      // smallest worst-case squared distance of a point over the cell
      double bound2 = std::numeric_limits<double>::infinity();
      for (int q = 0; q < 256; ++q) {
        const double dx = std::max(std::fabs(t[q].x - x0), std::fabs(t[q].x - x1));
        const double dy = std::max(std::fabs(t[q].y - y0), std::fabs(t[q].y - y1));
        bound2 = std::min(bound2, dx * dx + dy * dy);
      }
      const double bound = std::sqrt(bound2) + margin;
      const double lim2 = bound * bound;
      list.clear();
      for (int p = 0; p < 256; ++p) {
        const double dx = std::max({x0 - t[p].x, 0.0, t[p].x - x1});
        const double dy = std::max({y0 - t[p].y, 0.0, t[p].y - y1});
        if (dx * dx + dy * dy <= lim2) list.push_back((uint8_t)p);
      }
      const int len = (int)list.size();  // >= 1: the point defining the bound is always listed
      if (len < 1 || len > 15) return;  // does not fit the cell word
      int field = list[0];
      if (len > 1) {
        auto it = seen.find(list);
        if (it == seen.end()) {
          if (n + len > kCellListBytes) return;  // does not fit the list bytes
          std::copy(list.begin(), list.end(), cc->lists + n);
          it = seen.emplace(list, n).first;
          n += len;
        }
        field = it->second;
      }
      cc->cell[iy * kCellGrid + ix] = (uint16_t)((len << 12) | field);
    }
  }
  cc->R = R;
  cc->inv_cs = inv_cs;
}

}  // namespace gsdr
