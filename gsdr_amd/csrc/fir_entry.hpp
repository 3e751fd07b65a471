// gsdr-mi355x: the common body of the gsdrFir* entry points (reference src/fir.cu:73-171): argument
// checks, the T = 0 case and the kernel dispatch. Each sample-type pair is instantiated in its own
// translation unit (fir.hip: FC, fir_ff.hip, fir_cc.hip, fir_cf.hip, fir_int8.hip) so they build in
// parallel, and each unit's code object holds only the kernels of its own pair: the int8 matrix-core and
// variant launchers live in fir_i8_dispatch.hpp, which of these five only fir_int8.hip includes.
#pragma once

#include <hip/hip_runtime.h>

#include "fir_dispatch.hpp"
#include "launch.hpp"

namespace gsdr {

template <class TapT, class InT>
inline hipError_t fir_entry(size_t decimation, const TapT* taps, size_t tapCount, const InT* input,
                            typename Product<TapT, InT>::type* output, size_t numOutputs, int32_t device,
                            hipStream_t stream, int variant, uint32_t out_phase = 0) {
  using OutT = typename Product<TapT, InT>::type;
  if (numOutputs == 0) return hipSuccess;
  if (decimation == 0 || output == nullptr) return hipErrorInvalidValue;
  GSDR_ON_DEVICE(device, ([&]() -> hipError_t {
                   if (tapCount == 0) {
                     // reference: the tap loop never runs, every output is zero<OUT_T>() (fir.cu:43-46)
                     const hipError_t st = hipMemsetAsync(output, 0, numOutputs * sizeof(OutT), stream);
                     return st != hipSuccess ? st : launch_status();
                   }
                   if (taps == nullptr || input == nullptr) return hipErrorInvalidValue;
                   FirJob job = fir_job(decimation, taps, tapCount, output, numOutputs);
                   job.in = input;
                   job.L = (numOutputs - 1) * decimation + tapCount;
                   job.variant = variant;
                   job.out_phase = out_phase;
                   return launch_fir<TapT, InT, kModeFir>(job, stream);
                 })());
}

// The streaming object's one-launch FIR step on the tiled kernels (stream.hip; stream_step_tiled): the exact
// path, as the monolithic call runs for those shapes.
template <class InT>
inline hipError_t fir_stream_step_tiled(size_t decimation, const float* taps, size_t tapCount, const StreamOperands& so,
                                        hipFloatComplex* output, size_t numOutputs, int32_t device,
                                        hipStream_t stream) {
  const FirJob job = fir_job(decimation, taps, tapCount, output, numOutputs);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return stream_step_tiled<InT, kModeFir>(job, so, stream);
}

}  // namespace gsdr
