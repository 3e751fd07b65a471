// gsdr-mi355x: frequency-translating FIR -- NCO shift + low-pass FIR + decimation with the complex baseband output
// stored (gsdrxXlatingFir, gsdrxXlatingFirInt8, gsdrxXlatingFirMulti; include/gsdr/gsdr_ext.h). The FIR stage of
// gsdrAmDemod with the NCO's absolute phase kept: the chain kernels of fir_engine.hpp in mode kModeIq, whose
// epilogue is the FIR store (the anchored polyphase tiles first rotate their outputs back to the absolute phase,
// anchor_rotate). This file holds that mode's kernel instantiations; the jobs are built by chain_job.hpp.
#include <hip/hip_runtime.h>

#include "chain_job.hpp"
#include "fir_dispatch.hpp"
#include "gsdr/gsdr_ext.h"
#include "launch.hpp"

namespace gsdr {

static ChainSpec xlate_spec(float fs, float tune, uint32_t decimation, size_t firstSampleIndex, const float* taps,
                            size_t tapCount) {
  return ChainSpec{kModeIq, fs, tune, decimation, firstSampleIndex, taps, tapCount};
}

// The streaming object's one-launch steps on the tiled and grouped kernels (chain_job.hpp), in mode IQ (`dev` and
// `devs` are unused).
hipError_t xlate_stream_step_tiled(const ChainSpec& cs, bool int8, float chan, float dev, const StreamOperands& so,
                                   void* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  return chain_step_tiled<kModeIq>(cs, int8, chan, dev, so, output, numOutputs, device, stream);
}

hipError_t xlate_multi_stream_step(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                                   const StreamOperands& so, void* output, size_t outStride, size_t numOutputs,
                                   int32_t device, hipStream_t stream) {
  return chain_multi_step<kModeIq>(cs, chans, devs, count, so, output, outStride, numOutputs, device, stream);
}

}  // namespace gsdr

using gsdr::kModeIq;
using gsdr::xlate_spec;

GSDR_C_LINKAGE hipError_t gsdrxXlatingFir(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                          uint32_t decimation, size_t firstSampleIndex, const float* taps,
                                          size_t numTaps, const hipFloatComplex* input, hipFloatComplex* output,
                                          size_t numOutputs, int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry<float2, kModeIq>(
      xlate_spec(rfSampleRate, tuningFrequency, decimation, firstSampleIndex, taps, numTaps), channelFrequency, 1.0f,
      reinterpret_cast<const float2*>(input), output, numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxXlatingFirInt8(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                              uint32_t decimation, size_t firstSampleIndex, const float* taps,
                                              size_t numTaps, const int8_t* input, hipFloatComplex* output,
                                              size_t numOutputs, int32_t cudaDevice,
                                              hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry<gsdr::Iq8, kModeIq>(
      xlate_spec(rfSampleRate, tuningFrequency, decimation, firstSampleIndex, taps, numTaps), channelFrequency, 1.0f,
      reinterpret_cast<const gsdr::Iq8*>(input), output, numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxXlatingFirMulti(float rfSampleRate, float tuningFrequency,
                                               const float* channelFrequencies, uint32_t numChannels,
                                               uint32_t decimation, size_t firstSampleIndex, const float* taps,
                                               size_t numTaps, int sampleFormat, const void* input,
                                               hipFloatComplex* output, size_t numOutputs, int32_t cudaDevice,
                                               hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_multi_format<kModeIq>(
      xlate_spec(rfSampleRate, tuningFrequency, decimation, firstSampleIndex, taps, numTaps), channelFrequencies,
      nullptr, numChannels, sampleFormat, input, output, numOutputs, cudaDevice, cudaStream);
}
