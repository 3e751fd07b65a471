// gsdr-mi355x: the FIR engine's launcher (FIR, FM / AM chain, frequency-translating FIR): describe the call, ask the
// launch plan (fir_plan.hpp: which kernel, tile, grid, LDS and staging; HIP-free and tested on the host), and
// instantiate what the plan says. The tile shapes per decimation are the plan's table (GSDR_FIR_ROWS); the switches
// here are generated from it. Nothing in this file computes a tile count, a stride or an LDS size.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "fir_engine.hpp"
#include "fir_plan.hpp"
#include "launch.hpp"

namespace gsdr {

struct FirJob {
  const void* in = nullptr;
  const void* taps = nullptr;
  void* out = nullptr;
  size_t D = 1;
  size_t T = 0;
  size_t N = 0;  // outputs written
  size_t L = 0;  // input samples readable
  int mode = kModeFir;
  int variant = -1;  // FC / D=4 tile-shape override for tuning (-1 = default)
  uint32_t nco_inc = 0;
  uint32_t nco_n0 = 0;
  float fm_gain = 0.0f;
  uint32_t out_phase = 0;  // absolute index of output 0 mod 16 (fir_i8_mfma.hpp)
  uint64_t q0 = 0;         // chains: absolute index of output 0 (firstSampleIndex / D) -- the anchored
                           // polyphase tiles' NCO cell grid (fir_nco.hpp, MixAnchored)
  // a streaming step's operands (FirParams): `in` is then the chunk and L its length. All zero otherwise.
  StreamOperands step{};
  // the streaming object's one-launch path on the tiled kernels (stream_step_tiled): only the polyphase and
  // contiguous-window kernels take it; the others return hipErrorNotSupported before launching anything
  bool stream_tiled = false;

  void set_step(const StreamOperands& so) {
    step = so;
    in = so.chunk;
    L = so.chunk_len;
  }
};

// The fields every job has, FIR or chain: the filter, where the outputs go and how many there are.
inline FirJob fir_job(size_t D, const void* taps, size_t T, void* out, size_t N) {
  FirJob j;
  j.D = D;
  j.taps = taps;
  j.T = T;
  j.out = out;
  j.N = N;
  return j;
}

inline FirParams make_params(const FirJob& j, const firplan::Plan& pl) {
  FirParams p{};
  p.in = j.in;
  p.taps = j.taps;
  p.out = j.out;
  p.L = j.L;
  p.N = j.N;
  p.T = (uint32_t)j.T;
  p.nch = pl.nch;
  p.tile_stride = pl.tile_stride;
  p.D = (uint32_t)j.D;
  p.nco_inc = j.nco_inc;
  p.nco_n0 = j.nco_n0;
  p.fm_gain = j.fm_gain;
  p.out_phase = j.out_phase & 15u;
  p.tile_shift = pl.tile_shift;
  p.cell_sub0 = pl.cell_sub0;
  p.in_off = j.step.in_off;
  p.hist = j.step.hist;
  p.hist_len = j.step.hist_len;
  p.hist_out = j.step.hist_out;
  p.hist_from = j.step.hist_from;
  p.hist_n = j.step.hist_n;
  return p;
}

// The call as the plan takes it (the CU count apart: plan_job).
template <class TapT, class InT>
inline firplan::Call describe(const FirJob& j, int mode, int entry = firplan::kEntryFir, uint32_t group = 0) {
  firplan::Call c;
  c.entry = entry;
  c.taps = std::is_same<TapT, float>::value ? firplan::kTapsReal : firplan::kTapsComplex;
  c.sample = SampleKind<InT>::value;
  c.mode = mode;
  c.D = j.D;
  c.T = j.T;
  c.N = j.N;
  c.variant = j.variant;
  c.stream_tiled = j.stream_tiled;
  c.group = group;
  c.in = reinterpret_cast<uintptr_t>(j.in);
  c.out = reinterpret_cast<uintptr_t>(j.out);
  c.out_phase = j.out_phase;
  c.q0 = j.q0;
  c.in_off = j.step.in_off;
  return c;
}

// hipSuccess: launch `pl`. Otherwise nothing is to be launched (fir_plan.hpp, status contract); a failed CU query
// comes back with its own error.
inline hipError_t plan_status(const firplan::Plan& pl, hipError_t cu_error) {
  switch (pl.status) {
    case firplan::kOk: return hipSuccess;
    case firplan::kNotSupported: return hipErrorNotSupported;
    case firplan::kNoCuCount: return cu_error != hipSuccess ? cu_error : hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}

template <class TapT, class InT, int MODE>
inline hipError_t plan_job(const FirJob& j, int entry, uint32_t group, firplan::Plan* pl) {
  firplan::Call c = describe<TapT, InT>(j, MODE, entry, group);
  hipError_t cu_error = hipSuccess;
  if (firplan::wants_cus(c)) {
    int cus = 0;
    cu_error = current_device_cus(&cus);
    c.cus = cu_error == hipSuccess ? cus : 0;
  }
  *pl = firplan::plan(c);
  return plan_status(*pl, cu_error);
}

// Calls f(std::bool_constant<VEC>, std::integral_constant<int, SH>), which launches the kernel, with the plan's
// staging: aligned vector loads, shifted aligned loads (SH: 1 for complex / int8 I/Q samples, the float offset 1..3
// for real ones) or per-sample loads.
template <class InT, class F>
inline void with_staging(const firplan::Plan& pl, F&& f) {
  constexpr std::integral_constant<int, 0> kNoShift{};
  if (pl.vec) {
    f(std::true_type{}, kNoShift);
  } else if (pl.sh != 0) {
    if constexpr (std::is_same<InT, float>::value) {
      switch (pl.sh) {
        case 1: f(std::false_type{}, std::integral_constant<int, 1>{}); break;
        case 2: f(std::false_type{}, std::integral_constant<int, 2>{}); break;
        default: f(std::false_type{}, std::integral_constant<int, 3>{}); break;
      }
    } else {
      f(std::false_type{}, std::integral_constant<int, 1>{});
    }
  } else {
    f(std::false_type{}, kNoShift);
  }
}

template <class TapT, class InT, int MODE>
hipError_t launch_generic_kernel(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  k_fir_generic<TapT, InT, MODE><<<dim3(pl.grid), dim3(256), 0, s>>>(p);
  return launch_status();
}

template <class TapT, class InT, class Shape, int MODE, class Opts>
hipError_t launch_poly(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  with_staging<InT>(pl, [&](auto vec, auto sh) {
    k_fir_poly<TapT, InT, Shape, decltype(vec)::value, MODE, decltype(sh)::value, Opts>
        <<<dim3(pl.grid), dim3(Shape::WG), pl.lds, s>>>(p);
  });
  return launch_status();
}

template <class TapT, class InT, int D, int R, int IC, int WG, int MODE>
hipError_t launch_contig(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  with_staging<InT>(pl, [&](auto vec, auto sh) {
    k_fir_contig<TapT, InT, D, R, IC, WG, decltype(vec)::value, MODE, decltype(sh)::value>
        <<<dim3(pl.grid), dim3(WG), pl.lds, s>>>(p);
  });
  return launch_status();
}

// Multi-channel chain (k_fir_poly_grouped): one launch per group of <= kMaxMultiChannels channels, the single-channel
// polyphase tile with the C channels of an input tile grouped on one XCD (same staging choice as launch_poly, so each
// channel is that kernel's call bit for bit).
template <class TapT, class InT, class Shape, int MODE>
hipError_t launch_poly_grouped(const firplan::Plan& pl, const FirParams& p, const MultiParams& mp, hipStream_t s) {
  static_assert(!std::is_same<InT, float>::value, "complex or int8 I/Q samples: one shifted form");
  with_staging<InT>(pl, [&](auto vec, auto sh) {
    k_fir_poly_grouped<TapT, InT, Shape, decltype(vec)::value, MODE, decltype(sh)::value>
        <<<dim3(pl.grid), dim3(Shape::WG), pl.lds, s>>>(p, mp, (uint32_t)pl.tiles);
  });
  return launch_status();
}

// Matrix-core FIR with register-resident taps (k_fir_mfma_bc)
template <int ABL = 0>
hipError_t launch_mfma_bc(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  constexpr int WG = firplan::kMfmaBcWG, MAXSEG = firplan::kMfmaBcMaxSeg;
  const auto k = pl.vec ? k_fir_mfma_bc<WG, MAXSEG, true, true, ABL> : k_fir_mfma_bc<WG, MAXSEG, false, true, ABL>;
  k<<<dim3(pl.grid), dim3(WG), pl.lds, s>>>(p);
  return launch_status();
}

// Runtime-decimation tile kernel (k_fir_rt) with the plan's workgroup; paired LDS reads (even D): same products,
// same order.
template <class TapT, class InT, int MODE, int WG>
hipError_t launch_rt_wg(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  const dim3 grid(pl.grid), block(WG);
  auto go = [&](auto vec) {
    if (pl.paired) {
      k_fir_rt<TapT, InT, firplan::kRtChunk, WG, decltype(vec)::value, MODE, true><<<grid, block, pl.lds, s>>>(p);
    } else {
      k_fir_rt<TapT, InT, firplan::kRtChunk, WG, decltype(vec)::value, MODE><<<grid, block, pl.lds, s>>>(p);
    }
  };
  if (pl.vec) {
    go(std::true_type{});
  } else {
    go(std::false_type{});
  }
  return launch_status();
}

template <class TapT, class InT, int MODE>
hipError_t launch_rt(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  switch (pl.wg) {
    case 256: return launch_rt_wg<TapT, InT, MODE, 256>(pl, p, s);
    case 128: return launch_rt_wg<TapT, InT, MODE, 128>(pl, p, s);
    default: return launch_rt_wg<TapT, InT, MODE, 64>(pl, p, s);
  }
}

// The plan's row (pl.row) as its kernel instantiation: one case per row of GSDR_FIR_ROWS that serves this sample
// class and tap kind (default shapes stream their loads and stores: NT).
template <class TapT, class InT, int MODE>
hipError_t launch_row(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  using namespace firplan;
  constexpr int kTapKind = std::is_same<TapT, float>::value ? kTapsReal : kTapsComplex;
  switch (pl.row) {
#define GSDR_FIR_LAUNCH_ROW(NAME, CLS, TAPS, D, KERN, R, CH, WG, SUBS, ROLE)                                \
  case kRow##NAME:                                                                                          \
    if constexpr (row_serves(CLS, TAPS, SampleKind<InT>::value, kTapKind)) {                                \
      if constexpr (KERN == kPoly) {                                                                        \
        return launch_poly<TapT, InT, TileShape<D, R, CH, WG, SUBS>, MODE, TileStreamed>(pl, p, s);         \
      } else {                                                                                              \
        return launch_contig<TapT, InT, D, R, CH, WG, MODE>(pl, p, s);                                      \
      }                                                                                                     \
    }                                                                                                       \
    break;
    GSDR_FIR_ROWS(GSDR_FIR_LAUNCH_ROW)
#undef GSDR_FIR_LAUNCH_ROW
    default: break;
  }
  return hipErrorInvalidValue;  // (the plan names only rows that serve the call)
}

// The plan's D = 4 tuning variant (pl.variant, GSDR_FIR_D4_VARIANTS); int8 I/Q takes the ones marked for it.
template <class TapT, class InT, int MODE>
hipError_t launch_d4_variant(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  switch (pl.variant) {
#define GSDR_FIR_LAUNCH_VARIANT(V, I8, R, JC, WG, NT, XM, CST, DMA)                                                     \
  case V:                                                                                                               \
    if constexpr (I8 != 0 || !std::is_same<InT, Iq8>::value) {                                                          \
      return launch_poly<TapT, InT, TileShape<4, R, JC, WG>, MODE, TileOpts<NT != 0, XM != 0, CST, DMA != 0>>(pl, p, s); \
    }                                                                                                                   \
    break;
    GSDR_FIR_D4_VARIANTS(GSDR_FIR_LAUNCH_VARIANT)
#undef GSDR_FIR_LAUNCH_VARIANT
    default: break;
  }
  return hipErrorInvalidValue;
}

// The int8 matrix-core launchers and gsdrxFirFCInt8Variant's (fir_i8_dispatch.hpp). Templates, declared here and
// defined there, so their kernels are instantiated only in the units whose launch_plan reaches them -- those
// include that header (fir_int8.hip; fm_am.hip for the chains). A non-template launcher in this header would put its
// kernels' device code into every unit that includes it, with no host stub to launch them from.
template <class InT>
hipError_t launch_i8_fir(const firplan::Plan& pl, const FirParams& p, hipStream_t s);
template <class InT>
hipError_t launch_int8_variant(const firplan::Plan& pl, const FirParams& p, hipStream_t s);
template <int MODE>
hipError_t launch_i8_chain(const firplan::Plan& pl, const FirParams& p, hipStream_t s);

// Ablation probes (gsdrxFirFCVariant >= 100; fir.hip, compiled only into the probes library, `make probes`; the
// product library returns hipErrorInvalidValue for them).
hipError_t launch_fc_probe(const FirJob& j, hipStream_t s);

// Instantiate what the plan says.
template <class TapT, class InT, int MODE>
hipError_t launch_plan(const FirJob& j, const firplan::Plan& pl, hipStream_t s) {
  constexpr bool kRealTaps = std::is_same<TapT, float>::value, kInt8 = std::is_same<InT, Iq8>::value;
  constexpr bool kFc = kRealTaps && std::is_same<InT, float2>::value;
  if (pl.family == firplan::kFamProbe) return launch_fc_probe(j, s);
  const FirParams p = make_params(j, pl);
  if constexpr (kInt8 && MODE == kModeFir) {
    if (j.D == 4 && j.variant >= 0) return launch_int8_variant<InT>(pl, p, s);
    if (pl.family == firplan::kFamI8Fir) return launch_i8_fir<InT>(pl, p, s);
  }
  if constexpr (kInt8 && kRealTaps && (MODE == kModeFm || MODE == kModeAm)) {
    if (pl.family == firplan::kFamI8Chain) return launch_i8_chain<MODE>(pl, p, s);
  }
  if constexpr (kFc && MODE == kModeFir) {
    if (pl.family == firplan::kFamMfmaBc) return launch_mfma_bc<>(pl, p, s);
    if (pl.variant >= 0) return launch_d4_variant<TapT, InT, MODE>(pl, p, s);
  }
  switch (pl.family) {
    case firplan::kFamGeneric: return launch_generic_kernel<TapT, InT, MODE>(pl, p, s);
    case firplan::kFamRt: return launch_rt<TapT, InT, MODE>(pl, p, s);
    case firplan::kFamPoly:
    case firplan::kFamContig: return launch_row<TapT, InT, MODE>(pl, p, s);
    default: return hipErrorInvalidValue;
  }
}

template <class TapT, class InT, int MODE>
hipError_t launch_fir(const FirJob& j, hipStream_t s) {
  firplan::Plan pl;
  const hipError_t e = plan_job<TapT, InT, MODE>(j, firplan::kEntryFir, 0, &pl);
  return e != hipSuccess ? e : launch_plan<TapT, InT, MODE>(j, pl, s);
}

// The generic kernel whatever the shape (the chains' T = 0 case).
template <class TapT, class InT, int MODE>
hipError_t launch_generic(const FirJob& j, hipStream_t s) {
  firplan::Plan pl;
  const hipError_t e = plan_job<TapT, InT, MODE>(j, firplan::kEntryGeneric, 0, &pl);
  return e != hipSuccess ? e : launch_generic_kernel<TapT, InT, MODE>(pl, make_params(j, pl), s);
}

// An explicit tile shape (the probes): the plan's tile arithmetic for it, then the kernel. A tap span that does not
// fit runs the generic kernel, as for a row.
template <class TapT, class InT, class Shape, int MODE, class Opts>
hipError_t launch_poly_shape(const FirJob& j, hipStream_t s) {
  const firplan::Row shape{SampleT<InT>::kPerGranule, firplan::kTapsAny, Shape::D, firplan::kPoly, Shape::R, Shape::JC,
                           Shape::WG, 1, 0};
  const firplan::Plan pl = firplan::plan_shape(describe<TapT, InT>(j, MODE), shape);
  if (pl.status != firplan::kOk) return plan_status(pl, hipSuccess);
  const FirParams p = make_params(j, pl);
  if (pl.family == firplan::kFamGeneric) return launch_generic_kernel<TapT, InT, MODE>(pl, p, s);
  return launch_poly<TapT, InT, Shape, MODE, Opts>(pl, p, s);
}
template <int ABL>
hipError_t launch_mfma_bc_shape(const FirJob& j, hipStream_t s) {
  const firplan::Plan pl = firplan::plan_mfma_bc(describe<float, float2>(j, kModeFir));
  if (pl.status != firplan::kOk) return plan_status(pl, hipSuccess);
  return launch_mfma_bc<ABL>(pl, make_params(j, pl), s);
}

// Multi-channel chain: the grouped kernel on the multi-channel rows of the table. Returns hipErrorNotSupported, before
// launching anything, when the shape does not apply (the caller then runs the channels one by one).
template <class InT, int MODE>
hipError_t launch_multi_chain(const FirJob& j, const MultiParams& mp, hipStream_t s) {
  using namespace firplan;
  Plan pl;
  const hipError_t e = plan_job<float, InT, MODE>(j, kEntryFir, mp.count, &pl);
  if (e != hipSuccess) return e;
  const FirParams p = make_params(j, pl);
  switch (pl.row) {
#define GSDR_FIR_LAUNCH_MULTI(NAME, CLS, TAPS, D, KERN, R, CH, WG, SUBS, ROLE)        \
  case kRow##NAME:                                                                    \
    if constexpr (((ROLE) & kMulti) != 0 && CLS == SampleT<InT>::kPerGranule) {       \
      return launch_poly_grouped<float, InT, TileShape<D, R, CH, WG>, MODE>(pl, p, mp, s); \
    }                                                                                 \
    break;
    GSDR_FIR_ROWS(GSDR_FIR_LAUNCH_MULTI)
#undef GSDR_FIR_LAUNCH_MULTI
    default: break;
  }
  return hipErrorNotSupported;
}

// A streaming step as the tiled kernels take it (FirParams): `in` is output 0's window, not the chunk.
template <class InT>
inline void set_step_tiled(FirJob& j, const StreamOperands& so) {
  j.step = so;
  j.stream_tiled = true;
  j.in = static_cast<const InT*>(so.chunk) + so.in_off;  // (may precede the chunk)
  j.L = (uint64_t)((int64_t)so.chunk_len - so.in_off);   // samples readable from there
}

// The streaming object's one-launch step on the tiled kernels (stream.hip): outputs [0, N) of the call,
// output 0's window at chunk offset so.in_off (negative: it starts in the history so.hist of so.hist_len
// samples), the next history (chunk offsets [hist_from, + hist_n)) copied by workgroup 0 of the same
// launch. The kernels are the monolithic call's, tile for tile, so the outputs are bit-identical to it.
// hipErrorNotSupported (nothing launched) when the shape runs another kernel; the stream then takes its
// seam path.
template <class InT, int MODE>
hipError_t stream_step_tiled(FirJob j, const StreamOperands& so, hipStream_t s) {
  if (j.N == 0 || j.T == 0 || j.taps == nullptr) return hipErrorNotSupported;
  set_step_tiled<InT>(j, so);
  return launch_fir<float, InT, MODE>(j, s);
}

}  // namespace gsdr
