// gsdr-mi355x: fused NCO + low-pass FIR + decimation + FM discriminator / AM envelope.
//   gsdrFmDemod  replaces reference src/fm.cu:181-218 (kernel k_Fm, fm.cu:21-69)
//   gsdrAmDemod  replaces reference src/am.cu:52-81  (kernel k_Am, am.cu:21-50)
// Both run the FIR engine of fir_engine.hpp with the NCO applied once per staged input sample
// (the reference recomputes it per tap, adjustFrequency.cu:36-55) and the demodulator fused into the
// epilogue, so the mixed and filtered intermediates never touch HBM.
#include <hip/hip_runtime.h>
#include <math.h>

#include "chain_job.hpp"
#include "fir_i8_dispatch.hpp"
#include "gsdr/am.h"
#include "gsdr/fm.h"
#include "gsdr/gsdr_ext.h"
#include "launch.hpp"

namespace gsdr {

// The streaming object's one-launch int8 chain step at decimation 4 (stream.hip; see fir_int8_stream_step).
hipError_t chain_int8_stream_step(const ChainSpec& cs, float chan, float dev, const StreamOperands& so, float* output,
                                  size_t numOutputs, int32_t device, hipStream_t stream) {
  if (cs.decimation != 4 || numOutputs == 0 || cs.tapCount == 0 || cs.taps == nullptr ||
      cs.tapCount > (size_t)firplan::kI8ChainMaxT) {
    return hipErrorNotSupported;
  }
  FirJob job;
  if (!chain_job(cs, chan, dev, output, numOutputs, &job)) return hipErrorInvalidValue;
  job.set_step(so);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return cs.mode == kModeFm ? launch_chain_i8_mfma<kModeFm>(job, stream) : launch_chain_i8_mfma<kModeAm>(job, stream);
}

// The streaming object's one-launch steps on the tiled and grouped kernels (chain_job.hpp), in modes FM and AM.
hipError_t chain_stream_step_tiled(const ChainSpec& cs, bool int8, float chan, float dev, const StreamOperands& so,
                                   void* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  return chain_step_tiled<kModeFm, kModeAm>(cs, int8, chan, dev, so, output, numOutputs, device, stream);
}

hipError_t chain_multi_stream_step(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                                   const StreamOperands& so, void* output, size_t outStride, size_t numOutputs,
                                   int32_t device, hipStream_t stream) {
  return chain_multi_step<kModeFm, kModeAm>(cs, chans, devs, count, so, output, outStride, numOutputs, device, stream);
}

}  // namespace gsdr

using gsdr::ChainSpec;
using gsdr::kModeAm;
using gsdr::kModeFm;

GSDR_C_LINKAGE hipError_t gsdrFmDemod(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                      float frequencyDeviation, uint32_t decimation, size_t firstSampleIndex,
                                      const float* lowPassTaps, size_t numLowPassTaps, const hipFloatComplex* input,
                                      float* output, size_t numOutputs, int32_t cudaDevice,
                                      hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry<float2, kModeFm, kModeAm>(
      ChainSpec{kModeFm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex, lowPassTaps, numLowPassTaps},
      channelFrequency, frequencyDeviation, reinterpret_cast<const float2*>(input), output, numOutputs, cudaDevice,
      cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrAmDemod(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                      uint32_t decimation, size_t firstSampleIndex, const float* lowPassTaps,
                                      size_t numLowPassTaps, const hipFloatComplex* input, float* output,
                                      size_t numElements, int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry<float2, kModeFm, kModeAm>(
      ChainSpec{kModeAm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex, lowPassTaps, numLowPassTaps},
      channelFrequency, 1.0f, reinterpret_cast<const float2*>(input), output, numElements, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxFmDemodInt8(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                           float frequencyDeviation, uint32_t decimation, size_t firstSampleIndex,
                                           const float* lowPassTaps, size_t numLowPassTaps, const int8_t* input,
                                           float* output, size_t numOutputs, int32_t cudaDevice,
                                           hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry<gsdr::Iq8, kModeFm, kModeAm>(
      ChainSpec{kModeFm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex, lowPassTaps, numLowPassTaps},
      channelFrequency, frequencyDeviation, reinterpret_cast<const gsdr::Iq8*>(input), output, numOutputs, cudaDevice,
      cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxAmDemodInt8(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                           uint32_t decimation, size_t firstSampleIndex, const float* lowPassTaps,
                                           size_t numLowPassTaps, const int8_t* input, float* output,
                                           size_t numElements, int32_t cudaDevice,
                                           hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry<gsdr::Iq8, kModeFm, kModeAm>(
      ChainSpec{kModeAm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex, lowPassTaps, numLowPassTaps},
      channelFrequency, 1.0f, reinterpret_cast<const gsdr::Iq8*>(input), output, numElements, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE uint32_t gsdrNcoPhaseIncrement(float rfSampleRate, float tuningFrequency,
                                              float channelFrequency) GSDR_NO_EXCEPT {
  uint32_t inc = 0;
  (void)gsdr::nco_increment(rfSampleRate, tuningFrequency, channelFrequency, &inc);
  return inc;
}

GSDR_C_LINKAGE const char* gsdrVersion(void) GSDR_NO_EXCEPT { return "gsdr-mi355x 0.1.0 (gfx950)"; }

GSDR_C_LINKAGE hipError_t gsdrxFmDemodMulti(float rfSampleRate, float tuningFrequency, const float* channelFrequencies,
                                            const float* frequencyDeviations, uint32_t numChannels,
                                            uint32_t decimation, size_t firstSampleIndex, const float* lowPassTaps,
                                            size_t numLowPassTaps, int sampleFormat, const void* input, float* output,
                                            size_t numOutputs, int32_t cudaDevice,
                                            hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_multi_format<kModeFm, kModeAm>(
      ChainSpec{kModeFm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex, lowPassTaps, numLowPassTaps},
      channelFrequencies, frequencyDeviations, numChannels, sampleFormat, input, output, numOutputs, cudaDevice,
      cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxAmDemodMulti(float rfSampleRate, float tuningFrequency, const float* channelFrequencies,
                                            uint32_t numChannels, uint32_t decimation, size_t firstSampleIndex,
                                            const float* lowPassTaps, size_t numLowPassTaps, int sampleFormat,
                                            const void* input, float* output, size_t numElements, int32_t cudaDevice,
                                            hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_multi_format<kModeFm, kModeAm>(
      ChainSpec{kModeAm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex, lowPassTaps, numLowPassTaps},
      channelFrequencies, nullptr, numChannels, sampleFormat, input, output, numElements, cudaDevice, cudaStream);
}
