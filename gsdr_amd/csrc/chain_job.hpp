// gsdr-mi355x: how a chain (NCO + FIR + epilogue: FM, AM or the complex output of the frequency-translating FIR)
// becomes a FirJob. Shared by the files that launch chains (fm_am.hip, xlate.hip), so there is one job builder.
#pragma once

#include <math.h>

#include "fir_dispatch.hpp"

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

}  // namespace gsdr
