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

template <class InT>
static hipError_t xlate_entry(const ChainSpec& cs, float chan, const InT* input, float2* output, size_t numOutputs,
                              int32_t device, hipStream_t stream) {
  if (numOutputs == 0) return hipSuccess;
  if (cs.decimation == 0 || output == nullptr || input == nullptr) return hipErrorInvalidValue;
  if (cs.tapCount > 0 && cs.taps == nullptr) return hipErrorInvalidValue;
  FirJob job;
  if (!chain_job(cs, chan, 1.0f, output, numOutputs, &job)) return hipErrorInvalidValue;
  job.in = input;
  job.L = chain_input_len(cs, numOutputs);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  // no taps: y == 0 everywhere, from the generic kernel (it touches neither taps nor input)
  if (cs.tapCount == 0) return launch_generic<float, InT, kModeIq>(job, stream);
  return launch_fir<float, InT, kModeIq>(job, stream);
}

template <class InT>
static hipError_t xlate_multi_entry(const ChainSpec& cs, const float* chans, uint32_t count, const InT* input,
                                    float2* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  if (numOutputs == 0 || count == 0) return hipSuccess;
  if (chans == nullptr) return hipErrorInvalidValue;
  if (cs.decimation == 0 || output == nullptr || input == nullptr) return hipErrorInvalidValue;
  if (cs.tapCount > 0 && cs.taps == nullptr) return hipErrorInvalidValue;
  for (uint32_t c0 = 0; c0 < count; c0 += kMaxMultiChannels) {
    const uint32_t n = count - c0 < (uint32_t)kMaxMultiChannels ? count - c0 : (uint32_t)kMaxMultiChannels;
    MultiParams mp;
    if (!chain_group(cs, chans, nullptr, c0, n, numOutputs, &mp)) return hipErrorInvalidValue;
    float2* out = output + (size_t)c0 * numOutputs;
    hipError_t e = hipErrorNotSupported;
    if (cs.tapCount > 0) {
      FirJob job = chain_job(cs, out, numOutputs);
      job.in = input;
      job.L = chain_input_len(cs, numOutputs);
      DeviceScope scope(device);
      if (scope.status() != hipSuccess) return scope.status();
      e = launch_multi_chain<InT, kModeIq>(job, mp, stream);
    }
    // hipErrorNotSupported comes back before anything is launched: one channel at a time through the
    // single-channel path
    if (e == hipErrorNotSupported) {
      e = hipSuccess;
      for (uint32_t c = 0; c < n && e == hipSuccess; ++c) {
        e = xlate_entry(cs, chans[c0 + c], input, out + (size_t)c * numOutputs, numOutputs, device, stream);
      }
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The streaming object's one-launch step on the tiled kernels (stream_step_tiled), complex float or int8 I/Q chunks.
hipError_t xlate_stream_step_tiled(const ChainSpec& cs, bool int8, float chan, const StreamOperands& so,
                                   hipFloatComplex* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  FirJob job;
  if (!chain_job(cs, chan, 1.0f, output, numOutputs, &job)) return hipErrorInvalidValue;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return int8 ? stream_step_tiled<Iq8, kModeIq>(job, so, stream) : stream_step_tiled<float2, kModeIq>(job, so, stream);
}

// The multi-channel streaming object's one-launch step on complex float chunks (as chain_multi_stream_step,
// fm_am.hip): channel c's outputs at output + c * outStride, counted in complex elements.
hipError_t xlate_multi_stream_step(const ChainSpec& cs, const float* chans, uint32_t count, const StreamOperands& so,
                                   hipFloatComplex* output, size_t outStride, size_t numOutputs, int32_t device,
                                   hipStream_t stream) {
  if (numOutputs == 0 || count == 0 || cs.tapCount == 0 || cs.taps == nullptr || cs.tapCount > (1u << 26)) {
    return hipErrorNotSupported;
  }
  if (cs.decimation != 2 && cs.decimation != 4 && cs.decimation != 8) return hipErrorNotSupported;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  for (uint32_t c0 = 0; c0 < count; c0 += kMaxMultiChannels) {
    const uint32_t n = count - c0 < (uint32_t)kMaxMultiChannels ? count - c0 : (uint32_t)kMaxMultiChannels;
    MultiParams mp;
    if (!chain_group(cs, chans, nullptr, c0, n, outStride, &mp)) return hipErrorInvalidValue;
    FirJob job = chain_job(cs, output + (size_t)c0 * outStride, numOutputs);
    set_step_tiled<float2>(job, so);
    if (c0 != 0) job.step.hist_out = nullptr;  // every group reads the old history; the first writes the next
    const hipError_t e = launch_multi_chain<float2, kModeIq>(job, mp, stream);
    if (e != hipSuccess) return e;  // hipErrorNotSupported only from the first group (same shape for all)
  }
  return hipSuccess;
}

}  // namespace gsdr

using gsdr::xlate_spec;

GSDR_C_LINKAGE hipError_t gsdrxXlatingFir(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                          uint32_t decimation, size_t firstSampleIndex, const float* taps,
                                          size_t numTaps, const hipFloatComplex* input, hipFloatComplex* output,
                                          size_t numOutputs, int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::xlate_entry(xlate_spec(rfSampleRate, tuningFrequency, decimation, firstSampleIndex, taps, numTaps),
                           channelFrequency, reinterpret_cast<const float2*>(input),
                           reinterpret_cast<float2*>(output), numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxXlatingFirInt8(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                              uint32_t decimation, size_t firstSampleIndex, const float* taps,
                                              size_t numTaps, const int8_t* input, hipFloatComplex* output,
                                              size_t numOutputs, int32_t cudaDevice,
                                              hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::xlate_entry(xlate_spec(rfSampleRate, tuningFrequency, decimation, firstSampleIndex, taps, numTaps),
                           channelFrequency, reinterpret_cast<const gsdr::Iq8*>(input),
                           reinterpret_cast<float2*>(output), numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxXlatingFirMulti(float rfSampleRate, float tuningFrequency,
                                               const float* channelFrequencies, uint32_t numChannels,
                                               uint32_t decimation, size_t firstSampleIndex, const float* taps,
                                               size_t numTaps, int sampleFormat, const void* input,
                                               hipFloatComplex* output, size_t numOutputs, int32_t cudaDevice,
                                               hipStream_t cudaStream) GSDR_NO_EXCEPT {
  const gsdr::ChainSpec cs = xlate_spec(rfSampleRate, tuningFrequency, decimation, firstSampleIndex, taps, numTaps);
  float2* out = reinterpret_cast<float2*>(output);
  if (sampleFormat == GSDRX_SAMPLES_CS8) {
    return gsdr::xlate_multi_entry(cs, channelFrequencies, numChannels, static_cast<const gsdr::Iq8*>(input), out,
                                   numOutputs, cudaDevice, cudaStream);
  }
  if (sampleFormat != GSDRX_SAMPLES_CF32) return hipErrorInvalidValue;
  return gsdr::xlate_multi_entry(cs, channelFrequencies, numChannels, static_cast<const float2*>(input), out,
                                 numOutputs, cudaDevice, cudaStream);
}
