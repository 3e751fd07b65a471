// gsdr-mi355x: the launchers of the int8 I/Q matrix-core kernels (fir_i8_mfma.hpp) and of gsdrxFirFCInt8Variant's
// plans: what launch_plan (fir_dispatch.hpp) reaches for int8 I/Q samples. Included only by the units that launch
// these kernels -- fir_int8.hip (the FIR) and fm_am.hip (the FM / AM chains) -- and every launcher is a template, so a
// unit's code object holds exactly the kernels its host code can launch.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "fir_dispatch.hpp"
#include "fir_i8_mfma.hpp"

namespace gsdr {

// int8 I/Q FIR on the matrix cores (k_fir_i8_mfma): persistent workgroups (their tap fragments are built once), in
// the shape, staging (G, LM) and output alignment (OA) the plan chose.
template <int NS, int BPC, int NCT, int PF>
hipError_t launch_i8_fir_shape(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  auto go = [&](auto g, auto lm) {
    constexpr int G = decltype(g)::value, LM = decltype(lm)::value;
    if (pl.OA) {
      k_fir_i8_mfma<4, NS, G, LM, true, BPC, NCT, PF><<<dim3(pl.grid), dim3(pl.wg), 0, s>>>(p, pl.ns, (uint32_t)pl.tiles);
    } else {
      k_fir_i8_mfma<4, NS, G, LM, false, BPC, NCT, PF><<<dim3(pl.grid), dim3(pl.wg), 0, s>>>(p, pl.ns, (uint32_t)pl.tiles);
    }
  };
  using std::integral_constant;
  if (pl.G == 8 && pl.LM == 1) {
    go(integral_constant<int, 8>{}, integral_constant<int, 1>{});
  } else if (pl.LM == 1) {
    go(integral_constant<int, 4>{}, integral_constant<int, 1>{});
  } else if (pl.LM == 2) {
    go(integral_constant<int, 4>{}, integral_constant<int, 2>{});
  } else {
    go(integral_constant<int, 8>{}, integral_constant<int, 0>{});
  }
  return launch_status();
}

template <class InT>
hipError_t launch_i8_fir(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  static_assert(std::is_same<InT, Iq8>::value, "int8 I/Q samples");
#define GSDR_I8_LAUNCH_SHAPE(NS_, BPC_, NCT_, PF_) \
  if (pl.NS == NS_ && pl.BPC == BPC_ && pl.NCT == NCT_ && pl.PF == PF_) return launch_i8_fir_shape<NS_, BPC_, NCT_, PF_>(pl, p, s);
  GSDR_I8_FIR_SHAPES(GSDR_I8_LAUNCH_SHAPE)
#undef GSDR_I8_LAUNCH_SHAPE
  return hipErrorInvalidValue;
}

// What gsdrxFirFCInt8Variant's plans launch: the shared tile-shape variants, the generic kernel (7) and the matrix-core
// sweep (40-46).
template <class InT>
hipError_t launch_int8_variant(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  switch (pl.family) {
    case firplan::kFamI8Fir: return launch_i8_fir<InT>(pl, p, s);
    case firplan::kFamGeneric: return launch_generic_kernel<float, InT, kModeFir>(pl, p, s);
    default: return launch_d4_variant<float, InT, kModeFir>(pl, p, s);
  }
}

// int8 I/Q FM / AM chain on the matrix cores (k_chain_i8_mfma): D = 4, T <= 132
template <int MODE, int NCT>
hipError_t launch_i8_chain_nct(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  constexpr int BPC = GSDR_CHAIN_BPC;
  const dim3 grid(pl.grid), block(pl.wg);
  if (pl.LM == 1) {
    k_chain_i8_mfma<MODE, 1, BPC, NCT><<<grid, block, 0, s>>>(p, pl.ns, (uint32_t)pl.tiles);
  } else if (pl.LM == 2) {
    k_chain_i8_mfma<MODE, 2, BPC, NCT><<<grid, block, 0, s>>>(p, pl.ns, (uint32_t)pl.tiles);
  } else {
    k_chain_i8_mfma<MODE, 0, BPC, NCT><<<grid, block, 0, s>>>(p, pl.ns, (uint32_t)pl.tiles);
  }
  return launch_status();
}

template <int MODE>
hipError_t launch_i8_chain(const firplan::Plan& pl, const FirParams& p, hipStream_t s) {
  if (pl.NCT == 1) return launch_i8_chain_nct<MODE, 1>(pl, p, s);  // a short call
  return launch_i8_chain_nct<MODE, GSDR_CHAIN_NCT>(pl, p, s);
}

// The int8 matrix-core kernels whatever the route (the stream object's one-launch steps at decimation 4).
template <class InT = Iq8>
hipError_t launch_i8_mfma(const FirJob& j, hipStream_t s) {
  firplan::Plan pl;
  const hipError_t e = plan_job<float, InT, kModeFir>(j, firplan::kEntryI8Fir, 0, &pl);
  return e != hipSuccess ? e : launch_i8_fir<InT>(pl, make_params(j, pl), s);
}
template <int MODE>
hipError_t launch_chain_i8_mfma(const FirJob& j, hipStream_t s) {
  firplan::Plan pl;
  const hipError_t e = plan_job<float, Iq8, MODE>(j, firplan::kEntryI8Chain, 0, &pl);
  return e != hipSuccess ? e : launch_i8_chain<MODE>(pl, make_params(j, pl), s);
}

}  // namespace gsdr
