// gsdr-mi355x: gsdrxFirFCInt8 / gsdrxFirFCInt8Variant: gsdrFirFC from interleaved int8 I/Q (gsdr_ext.h).
#include <hip/hip_runtime.h>

#include "fir_entry.hpp"
#include "fir_i8_dispatch.hpp"
#include "gsdr/fir.h"
#include "gsdr/gsdr_ext.h"

using gsdr::fir_entry;

GSDR_C_LINKAGE hipError_t gsdrxFirFCInt8(size_t decimation, const float* taps, size_t tapCount, const int8_t* input,
                                         hipFloatComplex* output, size_t numOutputs, int32_t cudaDevice,
                                         hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return fir_entry<float, gsdr::Iq8>(decimation, taps, tapCount, reinterpret_cast<const gsdr::Iq8*>(input), output,
                                     numOutputs, cudaDevice, cudaStream, -1);
}

GSDR_C_LINKAGE hipError_t gsdrxFirFCInt8Variant(int variant, size_t decimation, const float* taps, size_t tapCount,
                                                const int8_t* input, hipFloatComplex* output, size_t numOutputs,
                                                int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return fir_entry<float, gsdr::Iq8>(decimation, taps, tapCount, reinterpret_cast<const gsdr::Iq8*>(input), output,
                                     numOutputs, cudaDevice, cudaStream, variant < 0 ? -1 : variant);
}

namespace gsdr {
// The streaming object's int8 FIR on its seam path (stream.hip; stream_step.hpp).
hipError_t fir_int8_at(uint64_t outputIndex, size_t decimation, const float* taps, size_t tapCount,
                       const int8_t* input, hipFloatComplex* output, size_t numOutputs, int32_t device,
                       hipStream_t stream) {
  return fir_entry<float, Iq8>(decimation, taps, tapCount, reinterpret_cast<const Iq8*>(input), output, numOutputs,
                               device, stream, -1, (uint32_t)(outputIndex & 15u));
}

// The streaming object's one-launch step at decimation 4 (stream.hip): outputs [outputIndex, + N) of the
// stream, output 0's window at chunk offset inOff (negative: it starts in the history buffer), the next
// history copied by the same launch. Returns hipErrorNotSupported (nothing launched) for shapes that do
// not take the matrix-core kernel; the stream then takes its seam path.
hipError_t fir_int8_stream_step(uint64_t outputIndex, size_t decimation, const float* taps, size_t tapCount,
                                const StreamOperands& so, hipFloatComplex* output, size_t numOutputs, int32_t device,
                                hipStream_t stream) {
  if (decimation != 4 || numOutputs == 0 || tapCount == 0 || taps == nullptr ||
      tapCount > (size_t)I8Mfma<4, 8>::MAXT || (reinterpret_cast<uintptr_t>(output) % 8) != 0) {
    return hipErrorNotSupported;
  }
  FirJob job = fir_job(4, taps, tapCount, output, numOutputs);
  job.out_phase = (uint32_t)(outputIndex & 15u);
  job.set_step(so);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return launch_i8_mfma(job, stream);
}

// The same on the tiled kernels (decimations other than 4, or tap counts the matrix-core kernel does not
// take): the exact path, as the monolithic call runs for those shapes (stream_step_tiled).
hipError_t fir_int8_stream_step_tiled(size_t decimation, const float* taps, size_t tapCount, const StreamOperands& so,
                                      hipFloatComplex* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  return fir_stream_step_tiled<Iq8>(decimation, taps, tapCount, so, output, numOutputs, device, stream);
}
}  // namespace gsdr
