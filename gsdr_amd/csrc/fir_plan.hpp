// gsdr-mi355x: what one call of the FIR engine launches -- which kernel, which tile, how many workgroups, how much LDS,
// which staging -- as a pure function of the call's description: no HIP, so it is compiled and checked on the host
// alone (tests/test_fir_plan.py). fir_dispatch.hpp instantiates what the plan says and computes none of this itself;
// the kernels (fir_engine.hpp, fir_i8_mfma.hpp) read their tile geometry from the same definitions.
// Routes, and the status contract the stream object and the multi-channel entry points branch on: DESIGN.md
// section 3.1, "FIR launch plan". kInvalidValue and kNotSupported mean that nothing is launched.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSDR_PLAN_HD __host__ __device__
#else
#define GSDR_PLAN_HD
#endif

namespace gsdr {

// kModeIq: the chains' NCO + FIR stage with the complex output stored (gsdrxXlatingFir, xlate.hip)
enum Mode : int { kModeFir = 0, kModeFm = 1, kModeAm = 2, kModeIq = 3 };

// LDS byte offset of sample idx of an int8 matrix-core plane (bf16): 16 bytes of pad every P samples
// (fir_i8_mfma.hpp).
template <uint32_t P>
GSDR_PLAN_HD constexpr uint32_t i8_addr(uint32_t idx) {
  return idx * 2u + (idx / P) * 16u;
}

namespace firplan {

constexpr uint64_t ceil_div64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------------------------------------
// Sample kinds. per_granule: samples per 16-byte LDS granule. src_align: bytes one staging load moves from HBM per
// granule (the alignment the vector path needs).
// ------------------------------------------------------------------------------------------------
enum Sample : int { kSampleReal = 0, kSampleComplex = 1, kSampleIq8 = 2 };
enum Taps : int { kTapsReal = 0, kTapsComplex = 1, kTapsAny = 2 };
constexpr int per_granule(int sample) { return sample == kSampleReal ? 4 : 2; }
constexpr int src_align(int sample) { return sample == kSampleIq8 ? 4 : 16; }
constexpr int sample_bytes(int sample) { return sample == kSampleReal ? 4 : (sample == kSampleComplex ? 8 : 2); }

// LDS budget per workgroup for the tiled kernels (keeps >= 2 workgroups per CU on 160 KiB).
constexpr uint64_t kMaxTileLds = 64 * 1024;
constexpr uint64_t kMaxGrid = 0x7fffffffull;     // workgroups of one launch
constexpr uint64_t kMaxTiledTaps = 1u << 26;     // the tiled kernels address taps through a 32-bit buffer descriptor
constexpr uint64_t kMaxTapSpan = 0x40000000ull;  // padded tap span of a tile, samples

// ------------------------------------------------------------------------------------------------
// Tile geometry (TileGeo, fir_staging.hpp): a thread's segment is SG granules; when SG is even a one-granule pad
// follows each segment, so the per-lane stride is odd (conflict-free ds_read_b128).
// ------------------------------------------------------------------------------------------------
constexpr int tile_sg(int G, int D, int R) { return R * D / G; }
constexpr int tile_pad(int sg) { return (sg % 2 == 0) ? 1 : 0; }
GSDR_PLAN_HD constexpr uint32_t tile_padded(uint32_t g, int sg) { return g + (uint32_t)tile_pad(sg) * (g / (uint32_t)sg); }

// Dynamic LDS of a k_fir_poly / k_fir_contig tile whose taps span span_samples (chains add the exchange row).
constexpr uint64_t poly_lds_bytes(int G, int D, int R, int WG, uint32_t span_samples, int mode) {
  const uint32_t NG = ((uint32_t)(WG * R - 1) * (uint32_t)D + span_samples + (uint32_t)G - 1) / (uint32_t)G;
  uint64_t bytes = (uint64_t)(tile_padded(NG - 1, tile_sg(G, D, R)) + 1) * 16u;
  if (mode != kModeFir) bytes += ((uint64_t)WG * 8 + 15) / 16 * 16;
  return bytes;
}
// k_fir_rt: wg outputs a tile, runtime D, no pad
constexpr uint64_t rt_lds_bytes(int G, uint32_t D, uint32_t span_samples, int wg, int mode) {
  uint64_t bytes = (uint64_t)(((uint32_t)(wg - 1) * D + span_samples + (uint32_t)G - 1) / (uint32_t)G) * 16u;
  if (mode != kModeFir) bytes += ((uint64_t)wg * 8 + 15) / 16 * 16;
  return bytes;
}
// k_fir_mfma_bc: complex samples, D = 4, R = 4
constexpr uint64_t mfma_bc_lds_bytes(int WG, uint32_t T) {
  const uint32_t nseg = (12u + T + 15u) / 16u;
  const uint32_t NG = (4u * (uint32_t)(WG * 4 - 4) + 16u * nseg) / 2;
  return (uint64_t)(tile_padded(NG - 1, tile_sg(2, 4, 4)) + 1) * 16u;
}

// FM tiles overlap by one FIR output (the discriminator pairs y[m] with y[m + 1]). With odd D that stride would put
// every other tile off the staging alignment (and all of them on the per-sample load path), so those tiles overlap by
// two outputs instead. (k_fir_contig, k_fir_rt; the anchored polyphase tiles overlap by one thread's R outputs.)
constexpr uint32_t fm_tile_stride(int sample, uint32_t kt, uint64_t D) {
  return ((uint64_t)(kt - 1) * D * (uint64_t)sample_bytes(sample)) % (uint64_t)src_align(sample) == 0 ? kt - 1 : kt - 2;
}

// ------------------------------------------------------------------------------------------------
// The int8 matrix-core kernels' tiles (I8Mfma, I8ChainMfma: fir_i8_mfma.hpp). 256 threads; NCT C tiles per wave and
// tile; NS 32-sample K steps.
// ------------------------------------------------------------------------------------------------
constexpr int kI8WG = 256;
constexpr int i8_fir_kt(int nct) { return (kI8WG / 64) * nct * 128; }           // outputs per tile
constexpr int i8_fir_maxt(int D, int ns) { return 32 * ns - 15 * D; }           // 15 D + T <= 32 NS
constexpr int i8_fir_span(int D, int ns, int nct) { return (i8_fir_kt(nct) - 16) * D + 32 * ns; }
constexpr int kI8ChainD = 4, kI8ChainNs = 5;
constexpr int i8_chain_kt(int nct) { return (kI8WG / 64) * nct * 64; }          // y' per tile
constexpr int i8_chain_stride(int mode, int nct) { return mode == kModeFm ? i8_chain_kt(nct) - 16 : i8_chain_kt(nct); }
constexpr int kI8ChainMaxT = 32 * kI8ChainNs - 7 * kI8ChainD;                    // 132
constexpr int i8_chain_span(int nct) { return (i8_chain_kt(nct) - 8) * kI8ChainD + 32 * kI8ChainNs; }
// Q plane offset: = 128 (mod 256), so the Q columns' bank groups interleave the I columns'
template <uint32_t P>
constexpr uint32_t i8_plane(uint32_t span) {
  return (i8_addr<P>(span) + 255u) / 256u * 256u + 128u;
}
template <uint32_t P>
constexpr uint32_t i8_lds_bytes(uint32_t span) {
  return i8_plane<P>(span) + i8_addr<P>(span);
}
// the chains' default shape (probe builds override it for A/B timing)
#ifndef GSDR_CHAIN_NCT
#define GSDR_CHAIN_NCT 4
#endif
#ifndef GSDR_CHAIN_BPC
#define GSDR_CHAIN_BPC 3
#endif
// D = 4 float calls of at most one 256-output tile for every second slot take the R 1 shape (kRows)
#ifndef GSDR_SHORT_R1
#define GSDR_SHORT_R1 1
#endif

// ------------------------------------------------------------------------------------------------
// The shape table: every compile-time tile shape, once. The plan searches the constexpr table built from it and the
// launcher's switch is generated from it (fir_dispatch.hpp), so the two cannot drift. Each row is
//   X(name, samples per granule (4: real; 2: complex and int8 I/Q, which share their rows), taps the row serves,
//     D, kernel, R, chunk (JC rows of D taps for kPoly, IC taps for kContig), WG, SUBS, role)
// kDefault: the shape of that decimation. kShort: a D = 4 short-call shape, a sub-tile of the default tile (SUBS of
// them make one NCO cell, and the per-output MAC order depends only on (D, chunk): the same outputs bit for bit).
// kMulti: a default row the grouped multi-channel kernel runs too -- a subset of this table, not a second list.
// (Complex D = 4: WG 256, R 4 measured fastest for a whole channel at T = 127. Contiguous kernel: every tap chunk
// costs one scalar tap-load wait, hence 20-40. Complex taps on real samples at D = 1: R 16 spilled to scratch. Large
// even D: one output a thread, odd padded lane stride, where k_fir_rt's stride of D samples hits one LDS bank.)
// ------------------------------------------------------------------------------------------------
enum Kernel : int { kPoly = 0, kContig = 1 };
enum Role : int { kDefault = 1, kShort = 2, kMulti = 4 };

#define GSDR_FIR_ROWS(X)                                       \
  X(C1, 2, kTapsAny, 1, kContig, 8, 16, 256, 1, kDefault)      \
  X(C2, 2, kTapsAny, 2, kPoly, 8, 16, 128, 1, kDefault | kMulti) \
  X(C3, 2, kTapsAny, 3, kContig, 4, 24, 256, 1, kDefault)      \
  X(C4, 2, kTapsAny, 4, kPoly, 4, 16, 256, 1, kDefault | kMulti) \
  X(C4R2, 2, kTapsAny, 4, kPoly, 2, 16, 256, 2, kShort)        \
  X(C4R1, 2, kTapsAny, 4, kPoly, 1, 16, 256, 4, kShort)        \
  X(C5, 2, kTapsAny, 5, kContig, 4, 20, 128, 1, kDefault)      \
  X(C6, 2, kTapsAny, 6, kPoly, 2, 8, 256, 1, kDefault)         \
  X(C7, 2, kTapsAny, 7, kContig, 4, 28, 128, 1, kDefault)      \
  X(C8, 2, kTapsAny, 8, kPoly, 2, 8, 256, 1, kDefault | kMulti) \
  X(C10, 2, kTapsAny, 10, kPoly, 2, 8, 256, 1, kDefault)       \
  X(C12, 2, kTapsAny, 12, kPoly, 2, 8, 256, 1, kDefault)       \
  X(C16, 2, kTapsAny, 16, kPoly, 2, 8, 128, 1, kDefault)       \
  X(C20, 2, kTapsAny, 20, kPoly, 1, 8, 256, 1, kDefault)       \
  X(C24, 2, kTapsAny, 24, kPoly, 1, 8, 256, 1, kDefault)       \
  X(C32, 2, kTapsAny, 32, kPoly, 1, 8, 128, 1, kDefault)       \
  X(C40, 2, kTapsAny, 40, kPoly, 1, 8, 128, 1, kDefault)       \
  X(C48, 2, kTapsAny, 48, kPoly, 1, 8, 128, 1, kDefault)       \
  X(C64, 2, kTapsAny, 64, kPoly, 1, 8, 64, 1, kDefault)        \
  X(R1, 4, kTapsReal, 1, kContig, 16, 32, 256, 1, kDefault)    \
  X(R1C, 4, kTapsComplex, 1, kContig, 8, 16, 256, 1, kDefault) \
  X(R2, 4, kTapsAny, 2, kContig, 8, 16, 256, 1, kDefault)      \
  X(R3, 4, kTapsAny, 3, kContig, 4, 36, 256, 1, kDefault)      \
  X(R4, 4, kTapsAny, 4, kPoly, 8, 8, 128, 1, kDefault)         \
  X(R5, 4, kTapsAny, 5, kContig, 4, 40, 128, 1, kDefault)      \
  X(R6, 4, kTapsAny, 6, kContig, 2, 36, 256, 1, kDefault)      \
  X(R7, 4, kTapsAny, 7, kContig, 4, 28, 128, 1, kDefault)      \
  X(R8, 4, kTapsAny, 8, kPoly, 8, 8, 128, 1, kDefault)         \
  X(R10, 4, kTapsAny, 10, kContig, 2, 40, 256, 1, kDefault)    \
  X(R12, 4, kTapsAny, 12, kPoly, 4, 8, 128, 1, kDefault)       \
  X(R16, 4, kTapsAny, 16, kPoly, 4, 8, 128, 1, kDefault)       \
  X(R20, 4, kTapsAny, 20, kPoly, 1, 8, 256, 1, kDefault)       \
  X(R24, 4, kTapsAny, 24, kPoly, 1, 8, 256, 1, kDefault)       \
  X(R32, 4, kTapsAny, 32, kPoly, 1, 8, 256, 1, kDefault)       \
  X(R40, 4, kTapsAny, 40, kPoly, 1, 8, 256, 1, kDefault)       \
  X(R48, 4, kTapsAny, 48, kPoly, 1, 8, 128, 1, kDefault)       \
  X(R64, 4, kTapsAny, 64, kPoly, 1, 8, 128, 1, kDefault)

// Tile-shape variants of the headline case (real taps, complex samples, FIR mode, D = 4), selectable through
// gsdrxFirFCVariant for tuning sweeps, and the ones whose staging is generic over the sample type, which
// gsdrxFirFCInt8Variant takes too:
//   X(variant, int8 too, R, JC, WG, NT non-temporal streaming, XM XCD-aware tile order,
//     CST tile stored through LDS (1 plain, 2 streaming stores), DMA tile body staged by LDS-DMA)
// Not tile shapes, so not rows: 7 the generic kernel (both); 13 the f32 matrix-core core (k_fir_mfma_bc, T <= 132);
// int8 only: 40 / 41 the matrix-core FIR with 2 / 3 workgroups a CU (41 = the D = 4 default), 42 1,024-output
// tiles at every size, 43 512-output tiles, 44 the same with 4 workgroups a CU, 45 / 46 = 43 / 44 with two tiles in
// flight a workgroup. Variants >= 100 are the ablation probes of the probes library (fir.hip).
#define GSDR_FIR_D4_VARIANTS(X)        \
  X(0, 1, 4, 16, 256, 1, 0, 0, 0)      \
  X(1, 1, 8, 16, 128, 1, 0, 0, 0)      \
  X(3, 1, 8, 16, 64, 1, 0, 0, 0)       \
  X(4, 1, 8, 32, 128, 1, 0, 0, 0)      \
  X(5, 1, 4, 8, 256, 1, 0, 0, 0)       \
  X(8, 0, 4, 16, 256, 0, 0, 0, 0)      \
  X(9, 0, 4, 16, 256, 1, 1, 0, 0)      \
  X(10, 0, 4, 16, 256, 1, 0, 1, 0)     \
  X(11, 0, 4, 16, 256, 1, 0, 2, 0)     \
  X(14, 0, 4, 16, 256, 1, 0, 0, 1)     \
  X(24, 1, 4, 16, 64, 1, 0, 0, 0)      \
  X(25, 0, 2, 16, 256, 1, 0, 0, 0)     \
  X(26, 0, 1, 16, 256, 1, 0, 0, 0)     \
  X(28, 1, 4, 16, 128, 1, 0, 0, 0)

// The instantiations of the int8 matrix-core FIR (k_fir_i8_mfma at D = 4): X(NS, BPC, NCT, PF). NS: K steps the
// fragments hold (6 covers T <= 132 with fewer registers than 8); BPC: workgroups per CU; NCT: C tiles per wave and
// tile; PF: tiles in flight a workgroup.
#define GSDR_I8_FIR_SHAPES(X) \
  X(6, 3, 4, 1)               \
  X(6, 3, 1, 1)               \
  X(8, 3, 4, 1)               \
  X(8, 3, 1, 1)               \
  X(6, 2, 4, 1)               \
  X(8, 2, 4, 1)               \
  X(6, 3, 2, 1)               \
  X(6, 4, 1, 1)               \
  X(6, 3, 1, 2)               \
  X(6, 4, 1, 2)

struct Row {
  int cls, taps, D, kernel, R, chunk, WG, SUBS, role;
};
#define GSDR_FIR_ROW_ENTRY(NAME, CLS, TAPS, D, KERN, R, CH, WG, SUBS, ROLE) {CLS, TAPS, D, KERN, R, CH, WG, SUBS, ROLE},
constexpr Row kRows[] = {GSDR_FIR_ROWS(GSDR_FIR_ROW_ENTRY)};
#undef GSDR_FIR_ROW_ENTRY
#define GSDR_FIR_ROW_ID(NAME, CLS, TAPS, D, KERN, R, CH, WG, SUBS, ROLE) kRow##NAME,
enum RowId : int { GSDR_FIR_ROWS(GSDR_FIR_ROW_ID) kRowCount };
#undef GSDR_FIR_ROW_ID

struct Variant {
  int variant, int8_too, R, JC, WG, NT, XM, CST, DMA;
};
#define GSDR_FIR_VARIANT_ENTRY(V, I8, R, JC, WG, NT, XM, CST, DMA) {V, I8, R, JC, WG, NT, XM, CST, DMA},
constexpr Variant kD4Variants[] = {GSDR_FIR_D4_VARIANTS(GSDR_FIR_VARIANT_ENTRY)};
#undef GSDR_FIR_VARIANT_ENTRY
constexpr int kD4VariantCount = (int)(sizeof(kD4Variants) / sizeof(kD4Variants[0]));

constexpr bool row_serves(int cls, int taps, int sample, int tap_kind) {
  return cls == per_granule(sample) && (taps == kTapsAny || taps == tap_kind);
}

// Tap chunks of a tile whose taps lie in rows of `row` taps, rows_per_chunk rows a chunk (the polyphase kernels: rows
// of D, JC a chunk; the contiguous-window kernel: IC single taps a chunk), and the samples they span.
constexpr uint64_t tap_chunks(uint64_t T, uint64_t row, uint64_t rows_per_chunk) {
  return ceil_div64(ceil_div64(T, row), rows_per_chunk);
}
constexpr uint64_t row_tap_span(const Row& r, uint64_t T) {
  const uint64_t row = r.kernel == kPoly ? (uint64_t)r.D : 1u;
  return tap_chunks(T, row, (uint64_t)r.chunk) * (uint64_t)r.chunk * row;
}

// A row whose tile does not fit the LDS budget at the headline tap count would silently run the generic kernel:
// reject that at compile time (the FM layout is the largest), with a segment that is not whole granules.
constexpr bool rows_fit_at_t127() {
  for (int i = 0; i < kRowCount; ++i) {
    const Row& r = kRows[i];
    if ((r.R * r.D) % r.cls != 0) return false;
    if (poly_lds_bytes(r.cls, r.D, r.R, r.WG, (uint32_t)row_tap_span(r, 127), kModeFm) > kMaxTileLds) return false;
  }
  return true;
}
static_assert(rows_fit_at_t127(), "a tiled shape exceeds the LDS budget at T = 127 or splits a granule");

// ------------------------------------------------------------------------------------------------
// The call and its plan
// ------------------------------------------------------------------------------------------------
// Which entry point asks. kEntryFir: the routed call (launch_fir, stream_step_tiled; launch_multi_chain when
// `group` > 0). The others name their kernel: the generic kernel (the chains' T = 0 case) and the int8 matrix-core
// stream steps. (The probes name an explicit tile shape: plan_shape, plan_mfma_bc.)
enum Entry : int { kEntryFir = 0, kEntryGeneric, kEntryI8Fir, kEntryI8Chain };

struct Call {
  int entry = kEntryFir;
  int taps = kTapsReal;
  int sample = kSampleComplex;
  int mode = kModeFir;
  uint64_t D = 1, T = 0, N = 0;
  int variant = -1;
  bool stream_tiled = false;
  uint32_t group = 0;        // channels of a grouped launch, 0 = single
  uint64_t in = 0, out = 0;  // addresses (only their residues matter); `in` as FirParams takes it
  uint32_t out_phase = 0;
  uint64_t q0 = 0;
  int64_t in_off = 0;  // a stream step's chunk offset (the int8 matrix-core kernels' tile starts)
  int cus = 0;         // compute units, 0 = the query failed
};

enum Status : int { kOk = 0, kInvalidValue, kNotSupported, kNoCuCount };
enum Family : int {
  kFamNone = 0,
  kFamPoly,
  kFamPolyGrouped,
  kFamContig,
  kFamRt,
  kFamGeneric,
  kFamMfmaBc,
  kFamI8Fir,
  kFamI8Chain,
  kFamProbe  // variant >= 100: launch_fc_probe decides (it comes back through plan_shape / plan_mfma_bc)
};

struct Plan {
  int status = kOk;
  int family = kFamNone;
  int row = -1;       // kRows index (tiled families reached through the table)
  int variant = -1;   // kD4Variants' variant number (tiled family reached through a variant)
  Row shape{};        // tiled families: a row's, a variant's or a probe's tile shape
  bool vec = false;   // staging: aligned vector loads
  int sh = 0;         // else shifted aligned loads by sh samples (0: per-sample loads)
  uint32_t nch = 0;   // tap chunks
  uint64_t lds = 0;   // dynamic LDS bytes
  uint32_t tile_stride = 0, tile_shift = 0, cell_sub0 = 0;
  uint64_t tiles = 0;
  uint32_t grid = 0, wg = 0;
  bool paired = false;  // runtime-D: paired LDS reads (even D)
  // int8 matrix-core kernels: NS (template), G / LM staging granule and load mode, OA aligned output pairs, NCT, BPC, PF
  // and the kernels' ns argument
  int NS = 0, G = 0, LM = 0, NCT = 0, BPC = 0, PF = 1;
  bool OA = false;
  uint32_t ns = 0;
};

inline Plan refused(int status) {
  Plan p;
  p.status = status;
  return p;
}

inline Plan plan_generic(const Call& c) {
  if (c.stream_tiled) return refused(kNotSupported);
  Plan p;
  p.family = kFamGeneric;
  p.tiles = ceil_div64(c.N, 256);
  if (p.tiles > kMaxGrid) return refused(kInvalidValue);
  p.grid = (uint32_t)p.tiles;
  p.wg = 256;
  return p;
}

// The staging of a tiled launch whose tiles start every tile_samples samples from `in`: aligned vector loads when the
// pointer and the tile stride allow; else shifted aligned loads when the pointer is whole samples off and every tile
// start equally so (complex 8 bytes off 16, int8 I/Q 2 bytes off 4: sh = 1; real 1..3 floats off 16: sh = the
// offset); else per-sample loads.
inline void plan_staging(const Call& c, uint64_t tile_samples, Plan* p) {
  const uint64_t A = (uint64_t)src_align(c.sample);
  p->vec = c.in % A == 0 && (tile_samples * (uint64_t)sample_bytes(c.sample)) % A == 0;
  p->sh = 0;
  if (p->vec) return;
  if (c.sample == kSampleComplex) {
    if (c.in % 16 == 8 && tile_samples % 2 == 0) p->sh = 1;
  } else if (c.sample == kSampleIq8) {
    if (c.in % 4 == 2 && tile_samples % 2 == 0) p->sh = 1;
  } else if (c.in % 4 == 0 && c.in % 16 != 0 && tile_samples % 4 == 0) {
    p->sh = (int)((c.in % 16) / 4);
  }
}

// A tiled launch of an explicit shape. Polyphase tile grid, FIR: tile t = outputs [t KT, (t + 1) KT). Chains (anchored
// NCO, fir_nco.hpp MixAnchored): tiles on an absolute output grid of stride S -- KT for AM and IQ; KT - R for FM,
// whose tiles overlap by one thread's outputs so that every discriminator pairs two outputs of one tile -- output 0
// (absolute index q0) sits at tile_shift = q0 mod S in tile 0, which is sub-tile cell_sub0 of its NCO cell of SUBS
// tiles (CELL = SUBS S outputs). The contiguous-window tiles start at output 0 (fm_tile_stride). A tap span that does
// not fit: the generic kernel, or kNotSupported for a grouped call.
inline Plan plan_shape(const Call& c, const Row& s) {
  const int G = per_granule(c.sample);
  const bool poly = s.kernel == kPoly;
  const uint64_t row = poly ? (uint64_t)s.D : 1u;
  const uint64_t n = tap_chunks(c.T, row, (uint64_t)s.chunk);
  const uint64_t span = n * (uint64_t)s.chunk * row;
  const uint64_t lds = span > kMaxTapSpan ? 0 : poly_lds_bytes(G, s.D, s.R, s.WG, (uint32_t)span, c.mode);
  if (span > kMaxTapSpan || lds > kMaxTileLds) return c.group > 0 ? refused(kNotSupported) : plan_generic(c);
  Plan p;
  p.family = poly ? (c.group > 0 ? kFamPolyGrouped : kFamPoly) : kFamContig;
  p.shape = s;
  p.nch = (uint32_t)n;
  p.lds = lds;
  p.wg = (uint32_t)s.WG;
  const uint32_t kt = (uint32_t)(s.WG * s.R);
  if (poly) {
    p.tile_stride = c.mode == kModeFm ? kt - (uint32_t)s.R : kt;
    if (c.mode != kModeFir) {
      p.tile_shift = (uint32_t)(c.q0 % p.tile_stride);
      p.cell_sub0 = (uint32_t)((c.q0 % ((uint64_t)p.tile_stride * (uint64_t)s.SUBS)) / p.tile_stride);
    }
  } else {
    p.tile_stride = c.mode == kModeFm ? fm_tile_stride(c.sample, kt, c.D) : kt;
  }
  p.tiles = ceil_div64(c.N + p.tile_shift, p.tile_stride);
  if (c.group > 0) {
    // the C channels of an input tile grouped on one XCD: tiles rounded up to the 8 XCDs, times the channels
    const uint64_t blocks = ceil_div64(p.tiles, 8) * 8 * c.group;
    if (blocks > kMaxGrid) return refused(kNotSupported);
    p.grid = (uint32_t)blocks;
  } else {
    if (p.tiles > kMaxGrid) return refused(kInvalidValue);
    p.grid = (uint32_t)p.tiles;
  }
  // (the anchored grid moves every tile start by tile_shift * D samples: a whole number of aligned units, D even)
  plan_staging(c, (uint64_t)p.tile_stride * (uint64_t)s.D, &p);
  return p;
}

inline Plan plan_row(const Call& c, int row) {
  Plan p = plan_shape(c, kRows[row]);
  if (p.family != kFamGeneric) p.row = row;
  return p;
}

// Matrix-core FIR with register-resident taps (k_fir_mfma_bc): FC, D = 4, 3 D + T <= 16 MAXSEG.
constexpr int kMfmaBcWG = 256, kMfmaBcMaxSeg = 9;
inline Plan plan_mfma_bc(const Call& c) {
  if (c.D != 4 || 12 + c.T > 16u * kMfmaBcMaxSeg) return refused(kInvalidValue);
  Plan p;
  p.family = kFamMfmaBc;
  p.shape = Row{2, kTapsReal, 4, kPoly, 4, 0, kMfmaBcWG, 1, 0};
  p.lds = mfma_bc_lds_bytes(kMfmaBcWG, (uint32_t)c.T);
  p.wg = kMfmaBcWG;
  p.tile_stride = kMfmaBcWG * 4;
  p.tiles = ceil_div64(c.N, p.tile_stride);
  if (p.tiles > kMaxGrid) return refused(kInvalidValue);
  p.grid = (uint32_t)p.tiles;
  p.vec = c.in % 16 == 0;
  return p;
}

// Runtime-decimation tile kernel (k_fir_rt) for decimations without a row, when taps overlap between outputs
// (T > D): the widest workgroup (256, 128 or 64 outputs a tile) whose tile fits the LDS budget; otherwise the generic
// kernel. (It has no shifted staging: both non-vector stagings load per sample.)
constexpr int kRtChunk = 16;
inline Plan plan_rt(const Call& c) {
  if (c.stream_tiled) return refused(kNotSupported);
  if (c.T <= c.D || c.D > 4096) return plan_generic(c);
  const int G = per_granule(c.sample);
  const uint32_t nch = (uint32_t)ceil_div64(c.T, kRtChunk), span = nch * kRtChunk;
  for (int wg = 256; wg >= 64; wg /= 2) {
    const uint64_t lds = rt_lds_bytes(G, (uint32_t)c.D, span, wg, c.mode);
    if (lds > kMaxTileLds) continue;
    Plan p;
    p.family = kFamRt;
    p.nch = nch;
    p.lds = lds;
    p.wg = (uint32_t)wg;
    p.tile_stride = c.mode == kModeFm ? fm_tile_stride(c.sample, (uint32_t)wg, c.D) : (uint32_t)wg;
    p.tiles = ceil_div64(c.N, p.tile_stride);
    if (p.tiles > kMaxGrid) return refused(kInvalidValue);
    p.grid = (uint32_t)p.tiles;
    plan_staging(c, (uint64_t)p.tile_stride * c.D, &p);
    p.sh = 0;
    p.paired = c.D % 2 == 0;
    return p;
  }
  return plan_generic(c);
}

// The persistent grid of the int8 matrix-core kernels: one workgroup per slot (CUs x workgroups per CU), at most one
// per tile; the tile grid starts at output -out_phase (the kernels' 16-output blocks are aligned to the absolute
// output index). With `short_nct`, a short call (fewer tiles than two rounds of slots) takes tiles of short_nct C
// tiles a wave: one large tile alone is ~10 us, so a call of a few hundred was one tile's latency on a third of the
// slots. Same outputs bit for bit (the summation order is per 16-output block).
inline void plan_persistent(const Call& c, uint64_t tile_outputs, uint64_t short_outputs, int short_nct, Plan* p) {
  const uint64_t outputs = c.N + (c.out_phase & 15u), slots = (uint64_t)c.cus * (uint64_t)p->BPC;
  p->tiles = ceil_div64(outputs, tile_outputs);
  if (short_nct > 0 && p->tiles < 2 * slots) {
    p->NCT = short_nct;
    p->tiles = ceil_div64(outputs, short_outputs);
  }
  p->grid = (uint32_t)(p->tiles < slots ? p->tiles : slots);
  p->wg = kI8WG;
}

// int8 I/Q FIR on the matrix cores (k_fir_i8_mfma, fir_i8_mfma.hpp): D = 4, T <= 196, 8-byte-aligned output. The
// staging granule and the output pairs are aligned per call from the pointers and the phase. `bpc` workgroups a CU;
// fixed_nct > 0: that tile size at every call size with NS = 6 (the tile-shape sweep), else 4 with the short-call
// switch to 1 (bpc = 3 only).
inline Plan plan_i8_fir(const Call& c, int bpc, int fixed_nct, int pf) {
  const uint64_t maxt = (uint64_t)i8_fir_maxt(4, fixed_nct > 0 ? 6 : 8);
  if (c.D != 4 || c.T < 1 || c.T > maxt || c.out % 8 != 0) return refused(kInvalidValue);
  Plan p;
  p.family = kFamI8Fir;
  p.NS = c.T <= (uint64_t)i8_fir_maxt(4, 6) ? 6 : 8;
  p.ns = (uint32_t)ceil_div64(15u * 4u + c.T, 32u);
  p.BPC = bpc;
  p.PF = pf;
  if (c.cus <= 0) return refused(kNoCuCount);
  const uint32_t phase = c.out_phase & 15u;
  if (fixed_nct > 0) {
    p.NCT = fixed_nct;  // (no grid refusal here: the kernel takes the low 32 bits of the tile count)
    plan_persistent(c, (uint64_t)i8_fir_kt(fixed_nct), 0, 0, &p);
  } else {
    p.NCT = 4;
    if (ceil_div64(c.N + phase, (uint64_t)i8_fir_kt(4)) > kMaxGrid) return refused(kInvalidValue);
    plan_persistent(c, (uint64_t)i8_fir_kt(4), (uint64_t)i8_fir_kt(1), bpc == 3 ? 1 : 0, &p);
  }
  // tile starts are at sample (j KT - phase) D + in_off: byte offset 2 D (j KT - phase) + 2 in_off
  const uint64_t in0 = c.in + (uint64_t)(2 * c.in_off) - 2u * 4u * phase;
  p.OA = (c.out - 8u * phase) % 16 == 0;
  if (in0 % 16 == 0) {
    p.G = 8, p.LM = 1;
  } else if (in0 % 8 == 0) {
    p.G = 4, p.LM = 1;
  } else if (in0 % 2 == 0) {
    p.G = 4, p.LM = 2;  // 2-byte aligned: shifted 8-byte loads
  } else {
    p.G = 8, p.LM = 0;
  }
  return p;
}

// int8 I/Q FM / AM chain on the matrix cores (k_chain_i8_mfma): D = 4, T <= 132 (the callers' conditions).
inline Plan plan_i8_chain(const Call& c) {
  Plan p;
  p.family = kFamI8Chain;
  p.NS = kI8ChainNs;
  p.ns = (uint32_t)ceil_div64(7u * 4u + c.T, 32u);
  p.BPC = GSDR_CHAIN_BPC;
  p.NCT = GSDR_CHAIN_NCT;
  const uint32_t phase = c.out_phase & 15u;
  if (ceil_div64(c.N + phase, (uint64_t)i8_chain_stride(c.mode, GSDR_CHAIN_NCT)) > kMaxGrid) return refused(kInvalidValue);
  if (c.cus <= 0) return refused(kNoCuCount);
  plan_persistent(c, (uint64_t)i8_chain_stride(c.mode, GSDR_CHAIN_NCT), (uint64_t)i8_chain_stride(c.mode, 1),
                  GSDR_CHAIN_NCT > 1 ? 1 : 0, &p);
  // tile starts are at sample 4 (j STRIDE - phase) + in_off: 8 (j STRIDE - phase) + 2 in_off bytes
  const uint64_t in0 = c.in + (uint64_t)(2 * c.in_off);
  p.G = 4;
  p.LM = in0 % 8 == 0 ? 1 : (in0 % 2 == 0 ? 2 : 0);  // 2: 2-byte aligned, shifted 8-byte loads
  return p;
}

// Decimation 4 (the headline shape, complex or int8 I/Q samples) with the tile sized to the call: a call of a few
// rounds of workgroup slots (a stream chunk) pays each round's latency on part of the chip. Kernel trace of the
// shapes (tools/short_call_shapes.py, profiles/r04_short_call_shapes.txt): at 2.1 M / 524 K / 131 K outputs WG 256 R 4
// took 24.5 / 9.0 / 6.3 us, WG 256 R 2 (512-output tiles) 22.0 / 8.5 / 5.4, WG 64 R 4 23.5 / 8.9 / 5.7, WG 256 R 1
// 29.2 / 9.9 / 5.1 -- so calls of fewer than three rounds of 1,024-output tiles take R 2. Calls of at most one
// 256-output tile for every second slot (2^19 input samples on 256 CUs) take R 1; measured per FM call
// (tools/short_call_floor.py): 2^16 / 2^18 samples 5.41 / 5.51 -> 4.74 / 4.89 us direct, 7.98 / 7.71 -> 5.95 / 5.96 us
// as a stream call; at 2^20 samples (one such tile a slot) 6.93 -> 8.39 us, so larger calls keep R 2. An unknown CU
// count takes the default tile.
inline int plan_d4_row(const Call& c) {
  if (c.cus > 0) {
    const uint64_t slots = (uint64_t)c.cus * 4;  // 38 KB tiles: 4 workgroups a CU
    if (GSDR_SHORT_R1 && 2 * ceil_div64(c.N, 256) <= slots) return kRowC4R1;
    if (ceil_div64(c.N, 1024) < 3 * slots) return kRowC4R2;
  }
  return kRowC4;
}

constexpr int default_row(int sample, int tap_kind, uint64_t D) {
  for (int i = 0; i < kRowCount; ++i) {
    if ((kRows[i].role & kDefault) && (uint64_t)kRows[i].D == D && row_serves(kRows[i].cls, kRows[i].taps, sample, tap_kind)) {
      return i;
    }
  }
  return -1;
}

// The CU count matters to the single-channel D = 4 calls on complex or int8 I/Q samples only; the launcher queries it
// for those.
constexpr bool wants_cus(const Call& c) {
  return c.entry == kEntryI8Fir || c.entry == kEntryI8Chain ||
         (c.entry == kEntryFir && c.group == 0 && c.D == 4 && c.sample != kSampleReal);
}

// The D = 4 tuning variants (real taps, FIR mode; complex samples, or int8 I/Q with the ones it shares)
inline Plan plan_d4_variant(const Call& c) {
  const bool i8 = c.sample == kSampleIq8;
  if (!i8 && c.variant >= 100) {
    Plan p;
    p.family = kFamProbe;
    return p;
  }
  for (int i = 0; i < kD4VariantCount; ++i) {
    const Variant& v = kD4Variants[i];
    if (v.variant != c.variant || (i8 && !v.int8_too)) continue;
    Plan p = plan_shape(c, Row{2, kTapsAny, 4, kPoly, v.R, v.JC, v.WG, 1, 0});
    if (p.family != kFamGeneric) p.variant = v.variant;
    return p;
  }
  if (c.variant == 7) return plan_generic(c);
  if (!i8) return c.variant == 13 ? plan_mfma_bc(c) : refused(kInvalidValue);
  switch (c.variant) {
    case 40: return plan_i8_fir(c, 2, 0, 1);
    case 41: return plan_i8_fir(c, 3, 0, 1);
    case 42: return plan_i8_fir(c, 3, 2, 1);
    case 43: return plan_i8_fir(c, 3, 1, 1);
    case 44: return plan_i8_fir(c, 4, 1, 1);
    case 45: return plan_i8_fir(c, 3, 1, 2);
    case 46: return plan_i8_fir(c, 4, 1, 2);
    default: return refused(kInvalidValue);
  }
}

// The plan of a call. Int8 I/Q takes the float-input rows wherever it does not run on the matrix cores, so int8 and
// float inputs of one decimation give bit-identical outputs there.
inline Plan plan(const Call& c) {
  switch (c.entry) {
    case kEntryGeneric: return plan_generic(c);
    case kEntryI8Fir: return plan_i8_fir(c, 3, 0, 1);
    case kEntryI8Chain: return plan_i8_chain(c);
    default: break;
  }
  const bool real_taps = c.taps == kTapsReal;
  if (c.group > 0) {
    // same D, chunk and NCO cell as the single-channel row -> identical per-output MAC order and phasors
    const int row = c.T > kMaxTiledTaps ? -1 : default_row(c.sample, c.taps, c.D);
    if (row < 0 || !(kRows[row].role & kMulti)) return refused(kNotSupported);
    return plan_row(c, row);
  }
  if (c.T > kMaxTiledTaps) return plan_generic(c);
  if (c.D == 4 && c.sample != kSampleReal) {
    if (c.mode == kModeFir && c.variant >= 0 && (real_taps || c.sample == kSampleIq8)) return plan_d4_variant(c);
    if (c.sample == kSampleIq8 && real_taps && !c.stream_tiled) {
      // FM / AM chains: the matrix-core kernel with the NCO folded into complex taps (normwise parity with the float
      // chains: DESIGN.md section 3.3); variant 0 keeps the exact path (streams). The frequency-translating FIR
      // (kModeIq) has no matrix-core form.
      if ((c.mode == kModeFm || c.mode == kModeAm) && c.variant < 0 && c.T <= (uint64_t)kI8ChainMaxT) {
        return plan_i8_chain(c);
      }
      // FIR: the matrix-core kernel (bf16-exact samples, exact three-part taps; normwise parity with the float path,
      // twice its speed), which needs an 8-byte-aligned output
      if (c.mode == kModeFir && c.T <= (uint64_t)i8_fir_maxt(4, 8) && c.out % 8 == 0) return plan_i8_fir(c, 3, 0, 1);
    }
    return plan_row(c, plan_d4_row(c));
  }
  const int row = default_row(c.sample, c.taps, c.D);
  return row >= 0 ? plan_row(c, row) : plan_rt(c);
}

}  // namespace firplan
}  // namespace gsdr
