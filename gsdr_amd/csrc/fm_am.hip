// gsdr-mi355x: fused NCO + low-pass FIR + decimation + FM discriminator / AM envelope.
//   gsdrFmDemod  replaces reference src/fm.cu:181-218 (kernel k_Fm, fm.cu:21-69)
//   gsdrAmDemod  replaces reference src/am.cu:52-81  (kernel k_Am, am.cu:21-50)
// Both run the FIR engine of fir_engine.hpp with the NCO applied once per staged input sample
// (the reference recomputes it per tap, adjustFrequency.cu:36-55) and the demodulator fused into the
// epilogue, so the mixed and filtered intermediates never touch HBM.
#include <hip/hip_runtime.h>
#include <math.h>

#include "chain_job.hpp"
#include "fir_dispatch.hpp"
#include "gsdr/am.h"
#include "gsdr/fm.h"
#include "gsdr/gsdr_ext.h"
#include "launch.hpp"

namespace gsdr {

template <class InT>
static hipError_t chain_entry(const ChainSpec& cs, float chan, float dev, const InT* input, float* output,
                              size_t numOutputs, int32_t device, hipStream_t stream) {
  if (numOutputs == 0) return hipSuccess;
  if (cs.decimation == 0 || output == nullptr || input == nullptr) return hipErrorInvalidValue;
  if (cs.tapCount > 0 && cs.taps == nullptr) return hipErrorInvalidValue;
  FirJob job;
  if (!chain_job(cs, chan, dev, output, numOutputs, &job)) return hipErrorInvalidValue;
  job.in = input;
  job.L = chain_input_len(cs, numOutputs);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  if (cs.tapCount == 0) {
    // y == 0 everywhere: the generic kernel evaluates the epilogue on zero without touching taps
    return cs.mode == kModeFm ? launch_generic<float, InT, kModeFm>(job, stream)
                              : launch_generic<float, InT, kModeAm>(job, stream);
  }
  return cs.mode == kModeFm ? launch_fir<float, InT, kModeFm>(job, stream)
                            : launch_fir<float, InT, kModeAm>(job, stream);
}

template <class InT>
static hipError_t chain_multi_entry(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                                    const InT* input, float* output, size_t numOutputs, int32_t device,
                                    hipStream_t stream) {
  if (numOutputs == 0 || count == 0) return hipSuccess;
  if (chans == nullptr || (cs.mode == kModeFm && devs == nullptr)) return hipErrorInvalidValue;
  if (cs.decimation == 0 || output == nullptr || input == nullptr) return hipErrorInvalidValue;
  if (cs.tapCount > 0 && cs.taps == nullptr) return hipErrorInvalidValue;
  for (uint32_t c0 = 0; c0 < count; c0 += kMaxMultiChannels) {
    const uint32_t n = count - c0 < (uint32_t)kMaxMultiChannels ? count - c0 : (uint32_t)kMaxMultiChannels;
    MultiParams mp;
    if (!chain_group(cs, chans, devs, c0, n, numOutputs, &mp)) return hipErrorInvalidValue;
    float* out = output + (size_t)c0 * numOutputs;
    hipError_t e = hipErrorNotSupported;
    // int8 I/Q at decimation 4: the single-channel default is the matrix-core chain, so each channel runs
    // it (bit-identical to gsdrxFmDemodInt8 / gsdrxAmDemodInt8 with that channel's frequency)
    bool grouped = cs.tapCount > 0;
    if constexpr (std::is_same<InT, Iq8>::value) {
      if (cs.decimation == 4 && cs.tapCount <= (size_t)I8ChainMfma<kModeFm>::MAXT) grouped = false;
    }
    if (grouped) {
      FirJob job = chain_job(cs, out, numOutputs);
      job.in = input;
      job.L = chain_input_len(cs, numOutputs);
      DeviceScope scope(device);
      if (scope.status() != hipSuccess) return scope.status();
      e = cs.mode == kModeFm ? launch_multi_chain<InT, kModeFm>(job, mp, stream)
                             : launch_multi_chain<InT, kModeAm>(job, mp, stream);
    }
    // launch_multi_chain returns hipErrorNotSupported before launching anything (so there is no
    // sticky launch error of ours to clear): one channel at a time through the single-channel path
    if (e == hipErrorNotSupported) {
      e = hipSuccess;
      for (uint32_t c = 0; c < n && e == hipSuccess; ++c) {
        e = chain_entry(cs, chans[c0 + c], cs.mode == kModeFm ? devs[c0 + c] : 1.0f, input,
                        out + (size_t)c * numOutputs, numOutputs, device, stream);
      }
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The streaming object's one-launch int8 chain step at decimation 4 (stream.hip; see fir_int8_stream_step).
hipError_t chain_int8_stream_step(const ChainSpec& cs, float chan, float dev, const StreamOperands& so, float* output,
                                  size_t numOutputs, int32_t device, hipStream_t stream) {
  if (cs.decimation != 4 || numOutputs == 0 || cs.tapCount == 0 || cs.taps == nullptr ||
      cs.tapCount > (size_t)I8ChainMfma<kModeFm>::MAXT) {
    return hipErrorNotSupported;
  }
  FirJob job;
  if (!chain_job(cs, chan, dev, output, numOutputs, &job)) return hipErrorInvalidValue;
  job.set_step(so);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return cs.mode == kModeFm ? launch_chain_i8_mfma<kModeFm>(job, stream) : launch_chain_i8_mfma<kModeAm>(job, stream);
}

// The streaming object's one-launch chain step on the tiled kernels (stream_step_tiled), complex float or
// int8 I/Q chunks.
hipError_t chain_stream_step_tiled(const ChainSpec& cs, bool int8, float chan, float dev, const StreamOperands& so,
                                   float* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  FirJob job;
  if (!chain_job(cs, chan, dev, output, numOutputs, &job)) return hipErrorInvalidValue;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  if (int8) {
    return cs.mode == kModeFm ? stream_step_tiled<Iq8, kModeFm>(job, so, stream)
                              : stream_step_tiled<Iq8, kModeAm>(job, so, stream);
  }
  return cs.mode == kModeFm ? stream_step_tiled<float2, kModeFm>(job, so, stream)
                            : stream_step_tiled<float2, kModeAm>(job, so, stream);
}

// The multi-channel streaming object's one-launch step (stream.hip, gsdrxStreamCreateMulti) on complex float
// chunks: the grouped kernel of gsdrxFmDemodMulti / gsdrxAmDemodMulti (up to kMaxMultiChannels channels a
// launch) with the single-channel stream step's operands -- output 0's window at chunk offset in_off, seam
// samples read from the shared input history, the next history copied by workgroup 0 of the first launch.
// Channel c's outputs go to output + c * outStride. Each workgroup runs the single-channel tile, so channel c
// is bit-identical to its own gsdrxStream (and to one monolithic call). hipErrorNotSupported (nothing
// launched): the shape has no grouped kernel; the stream then runs the channels one by one.
hipError_t chain_multi_stream_step(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                                   const StreamOperands& so, float* output, size_t outStride, size_t numOutputs,
                                   int32_t device, hipStream_t stream) {
  if (numOutputs == 0 || count == 0 || cs.tapCount == 0 || cs.taps == nullptr || cs.tapCount > (1u << 26)) {
    return hipErrorNotSupported;
  }
  if (cs.decimation != 2 && cs.decimation != 4 && cs.decimation != 8) return hipErrorNotSupported;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  for (uint32_t c0 = 0; c0 < count; c0 += kMaxMultiChannels) {
    const uint32_t n = count - c0 < (uint32_t)kMaxMultiChannels ? count - c0 : (uint32_t)kMaxMultiChannels;
    MultiParams mp;
    if (!chain_group(cs, chans, devs, c0, n, outStride, &mp)) return hipErrorInvalidValue;
    FirJob job = chain_job(cs, output + (size_t)c0 * outStride, numOutputs);
    set_step_tiled<float2>(job, so);
    if (c0 != 0) job.step.hist_out = nullptr;  // every group reads the old history; the first writes the next
    const hipError_t e = cs.mode == kModeFm ? launch_multi_chain<float2, kModeFm>(job, mp, stream)
                                            : launch_multi_chain<float2, kModeAm>(job, mp, stream);
    if (e != hipSuccess) return e;  // hipErrorNotSupported only from the first group (same shape for all)
  }
  return hipSuccess;
}

static hipError_t chain_multi_format(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                                     int sampleFormat, const void* input, float* output, size_t numOutputs,
                                     int32_t device, hipStream_t stream) {
  if (sampleFormat == GSDRX_SAMPLES_CS8) {
    return chain_multi_entry(cs, chans, devs, count, static_cast<const Iq8*>(input), output, numOutputs, device,
                             stream);
  }
  if (sampleFormat != GSDRX_SAMPLES_CF32) return hipErrorInvalidValue;
  return chain_multi_entry(cs, chans, devs, count, static_cast<const float2*>(input), output, numOutputs, device,
                           stream);
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
  return gsdr::chain_entry(ChainSpec{kModeFm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex,
                                      lowPassTaps, numLowPassTaps},
                           channelFrequency, frequencyDeviation, reinterpret_cast<const float2*>(input), output,
                           numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrAmDemod(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                      uint32_t decimation, size_t firstSampleIndex, const float* lowPassTaps,
                                      size_t numLowPassTaps, const hipFloatComplex* input, float* output,
                                      size_t numElements, int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry(ChainSpec{kModeAm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex,
                                      lowPassTaps, numLowPassTaps},
                           channelFrequency, 1.0f, reinterpret_cast<const float2*>(input), output, numElements,
                           cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxFmDemodInt8(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                           float frequencyDeviation, uint32_t decimation, size_t firstSampleIndex,
                                           const float* lowPassTaps, size_t numLowPassTaps, const int8_t* input,
                                           float* output, size_t numOutputs, int32_t cudaDevice,
                                           hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry(ChainSpec{kModeFm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex,
                                      lowPassTaps, numLowPassTaps},
                           channelFrequency, frequencyDeviation, reinterpret_cast<const gsdr::Iq8*>(input), output,
                           numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxAmDemodInt8(float rfSampleRate, float tuningFrequency, float channelFrequency,
                                           uint32_t decimation, size_t firstSampleIndex, const float* lowPassTaps,
                                           size_t numLowPassTaps, const int8_t* input, float* output,
                                           size_t numElements, int32_t cudaDevice,
                                           hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_entry(ChainSpec{kModeAm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex,
                                      lowPassTaps, numLowPassTaps},
                           channelFrequency, 1.0f, reinterpret_cast<const gsdr::Iq8*>(input), output, numElements,
                           cudaDevice, cudaStream);
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
  return gsdr::chain_multi_format(ChainSpec{kModeFm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex,
                                             lowPassTaps, numLowPassTaps},
                                  channelFrequencies, frequencyDeviations, numChannels, sampleFormat, input, output,
                                  numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxAmDemodMulti(float rfSampleRate, float tuningFrequency, const float* channelFrequencies,
                                            uint32_t numChannels, uint32_t decimation, size_t firstSampleIndex,
                                            const float* lowPassTaps, size_t numLowPassTaps, int sampleFormat,
                                            const void* input, float* output, size_t numElements, int32_t cudaDevice,
                                            hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::chain_multi_format(ChainSpec{kModeAm, rfSampleRate, tuningFrequency, decimation, firstSampleIndex,
                                             lowPassTaps, numLowPassTaps},
                                  channelFrequencies, nullptr, numChannels, sampleFormat, input, output, numElements,
                                  cudaDevice, cudaStream);
}
