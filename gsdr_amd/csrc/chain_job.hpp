// gsdr-mi355x: how a chain (NCO + FIR + epilogue: FM, AM or the complex output of the frequency-translating FIR)
// becomes a FirJob, and the host paths around that job: the single- and multi-channel entries and the streaming
// object's tiled and grouped steps. Each is written once, as a template over the sample type and the modes a
// translation unit serves; fm_am.hip instantiates them for {FM, AM}, xlate.hip for {IQ}, so each unit holds its own
// modes' kernels and the two build in parallel.
#pragma once

#include <math.h>

#include <type_traits>

#include "fir_dispatch.hpp"
#include "gsdr/gsdr_ext.h"
#include "launch.hpp"

namespace gsdr {

static constexpr float kPiF = 3.14159265358979323846f;

// inc = llround(df / fs * 2^32) mod 2^32, df = tuning - channel (fm.cu:204, am.cu:68).
inline bool nco_increment(float fs, float tune, float chan, uint32_t* inc) {
  if (!(fs > 0.0f) || !isfinite(fs)) return false;
  const float df = tune - chan;
  if (!isfinite(df)) return false;
  const double turns = (double)df / (double)fs;
  const double scaled = turns * 4294967296.0;
  // reduce to [-2^32, 2^32] before rounding so llround never overflows
  const double reduced = fmod(scaled, 4294967296.0);
  *inc = (uint32_t)(int64_t)llround(reduced);
  return true;
}

// One channel's NCO increment and FM discriminator gain (as reference src/fm.cu:203; 0 for AM and IQ).
inline bool chain_channel(const ChainSpec& cs, float chan, float dev, uint32_t* inc, float* gain) {
  if (!nco_increment(cs.fs, cs.tune, chan, inc)) return false;
  *gain = cs.mode == kModeFm ? cs.fs / (2.0f * kPiF * dev) : 0.0f;
  return true;
}

// The one place a chain becomes a job: everything but the input (in and L, or the stream operands) and the
// channel. q0, the absolute index of output 0, anchors the polyphase tiles' NCO cell grid and is kept in
// full: the FM tile strides do not divide 2^32. The int8 matrix-core chains align their 16-output blocks to
// it, so chunked calls reproduce one call bit for bit (fir_i8_mfma.hpp). `out` holds floats (FM, AM) or complex
// elements (IQ).
inline FirJob chain_job(const ChainSpec& cs, void* out, size_t n) {
  FirJob job = fir_job(cs.decimation, cs.taps, cs.tapCount, out, n);
  job.mode = cs.mode;
  job.nco_n0 = (uint32_t)cs.firstSampleIndex;
  job.q0 = cs.firstSampleIndex / cs.decimation;
  job.out_phase = (uint32_t)(job.q0 & 15u);
  return job;
}

inline bool chain_job(const ChainSpec& cs, float chan, float dev, void* out, size_t n, FirJob* job) {
  *job = chain_job(cs, out, n);
  return chain_channel(cs, chan, dev, &job->nco_inc, &job->fm_gain);
}

// Input samples a monolithic call of n outputs reads: FM needs n + 1 FIR outputs.
inline size_t chain_input_len(const ChainSpec& cs, size_t n) {
  return (cs.mode == kModeFm ? n : n - 1) * (size_t)cs.decimation + cs.tapCount;
}

// Channels [c0, c0 + n) of a multi-channel call as one grouped launch's parameters (outStride in outputs).
inline bool chain_group(const ChainSpec& cs, const float* chans, const float* devs, uint32_t c0, uint32_t n,
                        size_t outStride, MultiParams* mp) {
  *mp = MultiParams{};
  mp->count = n;
  mp->out_stride = outStride;
  for (uint32_t c = 0; c < n; ++c) {
    const float dev = cs.mode == kModeFm ? devs[c0 + c] : 1.0f;
    if (!chain_channel(cs, chans[c0 + c], dev, &mp->inc[c], &mp->gain[c])) return false;
  }
  return true;
}

// Bytes of one output: floats for FM and AM, complex elements for IQ.
inline size_t chain_out_bytes(int mode) { return mode == kModeIq ? sizeof(float2) : sizeof(float); }

inline void* chain_out_at(const ChainSpec& cs, void* out, size_t element) {
  return static_cast<char*>(out) + element * chain_out_bytes(cs.mode);
}

// f(std::integral_constant<int, MODE>) for the one of MODES that `mode` names (the last one otherwise: a unit is
// only handed its own modes).
template <int M, int... REST, class F>
inline hipError_t with_mode(int mode, F&& f) {
  if constexpr (sizeof...(REST) > 0) {
    if (mode != M) return with_mode<REST...>(mode, f);
  }
  return f(std::integral_constant<int, M>{});
}

// One channel: gsdrFmDemod / gsdrAmDemod / gsdrxXlatingFir and their int8 forms. `dev` is read for FM only.
template <class InT, int... MODES>
hipError_t chain_entry(const ChainSpec& cs, float chan, float dev, const InT* input, void* output, size_t numOutputs,
                       int32_t device, hipStream_t stream) {
  if (numOutputs == 0) return hipSuccess;
  if (cs.decimation == 0 || output == nullptr || input == nullptr) return hipErrorInvalidValue;
  if (cs.tapCount > 0 && cs.taps == nullptr) return hipErrorInvalidValue;
  FirJob job;
  if (!chain_job(cs, chan, dev, output, numOutputs, &job)) return hipErrorInvalidValue;
  job.in = input;
  job.L = chain_input_len(cs, numOutputs);
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return with_mode<MODES...>(cs.mode, [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
    // no taps: y == 0 everywhere: the generic kernel evaluates the epilogue on zero without touching taps
    if (cs.tapCount == 0) return launch_generic<float, InT, MODE>(job, stream);
    return launch_fir<float, InT, MODE>(job, stream);
  });
}

// `count` channels of one input: gsdrxFmDemodMulti / gsdrxAmDemodMulti / gsdrxXlatingFirMulti. Channel c's outputs
// start at element c * numOutputs. `devs` is read for FM only.
template <class InT, int... MODES>
hipError_t chain_multi_entry(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                             const InT* input, void* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  if (numOutputs == 0 || count == 0) return hipSuccess;
  if (chans == nullptr || (cs.mode == kModeFm && devs == nullptr)) return hipErrorInvalidValue;
  if (cs.decimation == 0 || output == nullptr || input == nullptr) return hipErrorInvalidValue;
  if (cs.tapCount > 0 && cs.taps == nullptr) return hipErrorInvalidValue;
  for (uint32_t c0 = 0; c0 < count; c0 += kMaxMultiChannels) {
    const uint32_t n = count - c0 < (uint32_t)kMaxMultiChannels ? count - c0 : (uint32_t)kMaxMultiChannels;
    MultiParams mp;
    if (!chain_group(cs, chans, devs, c0, n, numOutputs, &mp)) return hipErrorInvalidValue;
    void* out = chain_out_at(cs, output, (size_t)c0 * numOutputs);
    hipError_t e = hipErrorNotSupported;
    bool grouped = cs.tapCount > 0;
    // FM / AM from int8 I/Q at decimation 4: the single-channel default is the matrix-core chain, so each channel
    // runs it (bit-identical to gsdrxFmDemodInt8 / gsdrxAmDemodInt8 with that channel's frequency). IQ has no
    // matrix-core chain and always tries the grouped kernel.
    if (std::is_same<InT, Iq8>::value && cs.mode != kModeIq && cs.decimation == 4 &&
        cs.tapCount <= (size_t)firplan::kI8ChainMaxT) {
      grouped = false;
    }
    if (grouped) {
      FirJob job = chain_job(cs, out, numOutputs);
      job.in = input;
      job.L = chain_input_len(cs, numOutputs);
      DeviceScope scope(device);
      if (scope.status() != hipSuccess) return scope.status();
      e = with_mode<MODES...>(cs.mode, [&](auto mode) {
        return launch_multi_chain<InT, decltype(mode)::value>(job, mp, stream);
      });
    }
    // launch_multi_chain returns hipErrorNotSupported before launching anything (so there is no sticky launch
    // error of ours to clear): one channel at a time through the single-channel path
    if (e == hipErrorNotSupported) {
      e = hipSuccess;
      for (uint32_t c = 0; c < n && e == hipSuccess; ++c) {
        e = chain_entry<InT, MODES...>(cs, chans[c0 + c], cs.mode == kModeFm ? devs[c0 + c] : 1.0f, input,
                                       chain_out_at(cs, out, (size_t)c * numOutputs), numOutputs, device, stream);
      }
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// gsdrx*Multi's sampleFormat as the sample type.
template <int... MODES>
hipError_t chain_multi_format(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                              int sampleFormat, const void* input, void* output, size_t numOutputs, int32_t device,
                              hipStream_t stream) {
  if (sampleFormat == GSDRX_SAMPLES_CS8) {
    return chain_multi_entry<Iq8, MODES...>(cs, chans, devs, count, static_cast<const Iq8*>(input), output,
                                            numOutputs, device, stream);
  }
  if (sampleFormat != GSDRX_SAMPLES_CF32) return hipErrorInvalidValue;
  return chain_multi_entry<float2, MODES...>(cs, chans, devs, count, static_cast<const float2*>(input), output,
                                             numOutputs, device, stream);
}

// The streaming object's one-launch chain step on the tiled kernels (stream_step_tiled), complex float or int8 I/Q
// chunks.
template <int... MODES>
hipError_t chain_step_tiled(const ChainSpec& cs, bool int8, float chan, float dev, const StreamOperands& so,
                            void* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  FirJob job;
  if (!chain_job(cs, chan, dev, output, numOutputs, &job)) return hipErrorInvalidValue;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  return with_mode<MODES...>(cs.mode, [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
    return int8 ? stream_step_tiled<Iq8, MODE>(job, so, stream) : stream_step_tiled<float2, MODE>(job, so, stream);
  });
}

// The multi-channel streaming object's one-launch step (stream.hip, gsdrxStreamCreateMulti) on complex float
// chunks: the grouped kernel of the multi-channel entry (up to kMaxMultiChannels channels a launch) with the
// single-channel stream step's operands -- output 0's window at chunk offset in_off, seam samples read from the
// shared input history, the next history copied by workgroup 0 of the first launch. Channel c's outputs go to
// element c * outStride of `output`. Each workgroup runs the single-channel tile, so channel c is bit-identical to
// its own gsdrxStream (and to one monolithic call). hipErrorNotSupported (nothing launched): the shape has no
// grouped kernel; the stream then runs the channels one by one.
template <int... MODES>
hipError_t chain_multi_step(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                            const StreamOperands& so, void* output, size_t outStride, size_t numOutputs,
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
    FirJob job = chain_job(cs, chain_out_at(cs, output, (size_t)c0 * outStride), numOutputs);
    set_step_tiled<float2>(job, so);
    if (c0 != 0) job.step.hist_out = nullptr;  // every group reads the old history; the first writes the next
    const hipError_t e = with_mode<MODES...>(cs.mode, [&](auto mode) {
      return launch_multi_chain<float2, decltype(mode)::value>(job, mp, stream);
    });
    if (e != hipSuccess) return e;  // hipErrorNotSupported only from the first group (same shape for all)
  }
  return hipSuccess;
}

}  // namespace gsdr
