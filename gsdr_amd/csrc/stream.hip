// gsdr-mi355x: streaming continuity object (include/gsdr/stream.h).
//
// Host-side bookkeeping around the filter kernels. The reference has no equivalent: its callers
// re-supply the overlap themselves (include/gsdr/fm.h:26, fm.cu:202), one launch per chunk. Per Process
// call, ONE launch (round 4; the int8 matrix-core kernels since round 3):
//   * seam outputs (window starts in the history, ends in the new chunk) read their first samples from
//     the history buffer by offset, every other output straight from the caller's chunk;
//   * workgroup 0 of the same launch copies the samples the next output still needs (< one window) into
//     the spare history buffer (ping-pong).
// The launch runs the kernel one monolithic call would run, with the absolute index of output 0's first
// sample as firstSampleIndex, so the NCO phase and the per-output MAC order are those of that call: the
// outputs are bit-identical. Shapes without a one-launch kernel (runtime-decimation and generic kernels)
// keep the older plan (stream_seam_plan, stream_buffers.hpp): a gather launch (seam = history + chunk head, next
// history), then the seam and the main outputs as two filter calls. Which outputs a call writes and where the kept
// samples go is stream_plan.hpp (L = 1), shared with gsdrxResampler.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "gsdr/am.h"
#include "gsdr/fir.h"
#include "gsdr/fm.h"
#include "gsdr/gsdr_ext.h"
#include "gsdr/stream.h"
#include "stream_buffers.hpp"
#include "stream_step.hpp"

struct gsdrxStream_t {
  int kind = GSDRX_STREAM_FIR;
  int format = GSDRX_SAMPLES_CF32;
  uint32_t D = 1;
  const float* taps = nullptr;
  size_t T = 0;
  size_t W = 0;  // samples one output needs
  float fs = 0.0f, tune = 0.0f;
  uint64_t n0 = 0;  // absolute index of stream sample 0
  int32_t device = 0;
  size_t sb = 8;  // bytes per input sample
  size_t ob = 8;  // bytes per output
  gsdr::StreamState st;  // history: samples [next_out * D, consumed) (empty if next_out * D >= consumed)
  // channels of one RF input (gsdrxStreamCreateMulti; one channel for gsdrxStreamCreate): frequency and
  // deviation per channel, channel c's outputs at output + c * outputCapacity
  std::vector<float> chans, devs;
};

namespace gsdr {
namespace {

bool plan_of(const gsdrxStream_t& s, size_t chunk, StreamPlan* sp) {
  return stream_plan(1, s.D, s.W, 0, s.st.consumed, s.st.next_out, chunk, sp);
}

hipError_t filter(const gsdrxStream_t& s, size_t c, const void* in, uint64_t first, void* out, size_t n,
                  hipStream_t st) {
  const bool i8 = s.format == GSDRX_SAMPLES_CS8;
  const float chan = s.chans[c], dev = s.devs[c];
  switch (s.kind) {
    case GSDRX_STREAM_FIR:
      // the default path of gsdrxFirFCInt8 told the output's absolute index: the decimation-4 matrix-core
      // kernel aligns its summation blocks to it, so chunks reproduce one call (fir_i8_mfma.hpp)
      return i8 ? fir_int8_at((first - s.n0) / s.D, s.D, s.taps, s.T, static_cast<const int8_t*>(in),
                              static_cast<hipFloatComplex*>(out), n, s.device, st)
                : gsdrFirFC(s.D, s.taps, s.T, static_cast<const hipFloatComplex*>(in),
                            static_cast<hipFloatComplex*>(out), n, s.device, st);
    case GSDRX_STREAM_FM:
      return i8 ? gsdrxFmDemodInt8(s.fs, s.tune, chan, dev, s.D, first, s.taps, s.T,
                                   static_cast<const int8_t*>(in), static_cast<float*>(out), n, s.device, st)
                : gsdrFmDemod(s.fs, s.tune, chan, dev, s.D, first, s.taps, s.T,
                              static_cast<const hipFloatComplex*>(in), static_cast<float*>(out), n, s.device, st);
    case GSDRX_STREAM_XLATE:
      return i8 ? gsdrxXlatingFirInt8(s.fs, s.tune, chan, s.D, first, s.taps, s.T, static_cast<const int8_t*>(in),
                                      static_cast<hipFloatComplex*>(out), n, s.device, st)
                : gsdrxXlatingFir(s.fs, s.tune, chan, s.D, first, s.taps, s.T,
                                  static_cast<const hipFloatComplex*>(in), static_cast<hipFloatComplex*>(out), n,
                                  s.device, st);
    default:
      return i8 ? gsdrxAmDemodInt8(s.fs, s.tune, chan, s.D, first, s.taps, s.T,
                                   static_cast<const int8_t*>(in), static_cast<float*>(out), n, s.device, st)
                : gsdrAmDemod(s.fs, s.tune, chan, s.D, first, s.taps, s.T, static_cast<const hipFloatComplex*>(in),
                              static_cast<float*>(out), n, s.device, st);
  }
}

// The small device-to-device moves of one call (seam = history + chunk head, next history = the tail of
// old history + chunk), gathered into ONE launch: as separate hipMemcpyAsync calls each was a runtime blit
// launch of ~4-5 us, four of them per call, which is what a short float call paid (tools/float_stream_time.py).
// Segments never overlap (they write seam / spare and read hist / the chunk). A move list of stream_plan.hpp
// resolved against an object's pointers, in bytes: an int8 I/Q sample is 2 of them.
struct Gather {
  static constexpr int kMax = 4;
  struct Seg {
    char* dst;
    const char* src;
    uint64_t bytes;
  } seg[kMax];
  int n = 0;
  void add(void* dst, const void* src, size_t bytes) {
    if (bytes) seg[n++] = Seg{static_cast<char*>(dst), static_cast<const char*>(src), bytes};
  }
};

__global__ __launch_bounds__(256) void k_stream_gather(Gather g) {
  for (int i = 0; i < g.n; ++i) {
    const Gather::Seg sg = g.seg[i];
    // 4-byte moves when both ends and the length allow (every sample format is 2 or 8 bytes)
    if (((reinterpret_cast<uintptr_t>(sg.dst) | reinterpret_cast<uintptr_t>(sg.src) | sg.bytes) & 3u) == 0) {
      uint32_t* d = reinterpret_cast<uint32_t*>(sg.dst);
      const uint32_t* s = reinterpret_cast<const uint32_t*>(sg.src);
      for (uint64_t k = threadIdx.x + (uint64_t)blockIdx.x * blockDim.x; k < sg.bytes / 4; k += (uint64_t)gridDim.x * blockDim.x)
        d[k] = s[k];
    } else {
      for (uint64_t k = threadIdx.x + (uint64_t)blockIdx.x * blockDim.x; k < sg.bytes; k += (uint64_t)gridDim.x * blockDim.x)
        sg.dst[k] = sg.src[k];
    }
  }
}

// One channel's one-launch step: int8 I/Q at decimation 4 on the matrix cores, every other shape on the tiled
// kernels (the same kernels as one monolithic call, tile for tile). hipErrorNotSupported, with nothing
// launched: the shape has no one-launch step.
hipError_t channel_step(const gsdrxStream_t& s, const ChainSpec& cs, size_t c, const StreamOperands& so, void* out,
                        size_t n, hipStream_t st) {
  const bool i8 = s.format == GSDRX_SAMPLES_CS8;
  hipError_t e = hipErrorNotSupported;
  if (s.kind == GSDRX_STREAM_FIR) {
    hipFloatComplex* o = static_cast<hipFloatComplex*>(out);
    if (i8) e = fir_int8_stream_step(s.st.next_out, s.D, s.taps, s.T, so, o, n, s.device, st);
    if (e != hipErrorNotSupported) return e;
    return i8 ? fir_int8_stream_step_tiled(s.D, s.taps, s.T, so, o, n, s.device, st)
              : fir_fc_stream_step(s.D, s.taps, s.T, so, o, n, s.device, st);
  }
  // (XLATE has no matrix-core form: int8 I/Q takes the tiled kernels at every decimation)
  const bool xlate = s.kind == GSDRX_STREAM_XLATE;
  if (i8 && !xlate) {
    e = chain_int8_stream_step(cs, s.chans[c], s.devs[c], so, static_cast<float*>(out), n, s.device, st);
  }
  if (e != hipErrorNotSupported) return e;
  ChainStepTiled* step = xlate ? xlate_stream_step_tiled : chain_stream_step_tiled;
  return step(cs, i8, s.chans[c], s.devs[c], so, out, n, s.device, st);
}

}  // namespace

hipError_t stream_move(const StreamState& b, const StreamMoves& mv, const void* chunk, size_t sb, hipStream_t st) {
  if (mv.n == 0) return hipSuccess;
  Gather g;
  uint64_t most = 0;
  for (int i = 0; i < mv.n; ++i) {
    const StreamMoves::Seg& m = mv.seg[i];
    g.add(b.at(m.dst, chunk) + m.dst_off * sb, b.at(m.src, chunk) + m.src_off * sb, m.count * sb);
    most = std::max<uint64_t>(most, m.count * sb);
  }
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(64, ceil_div<uint64_t>(most, 256u * 4u));
  k_stream_gather<<<blocks, 256, 0, st>>>(g);
  return launch_status();
}

}  // namespace gsdr

using gsdr::StreamPlan;

GSDR_C_LINKAGE void gsdrxStreamPlan(uint32_t decimation, size_t window, uint64_t consumed, uint64_t nextOutput,
                                    size_t chunk, uint64_t plan[5]) GSDR_NO_EXCEPT {
  if (plan == nullptr) return;
  StreamPlan p;
  (void)gsdr::stream_plan(1, decimation, window, 0, consumed, nextOutput, chunk, &p);
  plan[0] = p.seam;  // (all zero when refused)
  plan[1] = p.head;
  plan[2] = p.outputs - p.seam;
  plan[3] = (uint64_t)p.main_off;
  plan[4] = p.hist_after;
}

namespace gsdr {
namespace {
hipError_t create_stream(gsdrxStream* stream, int kind, int sampleFormat, uint32_t decimation, const float* taps,
                         size_t tapCount, float rfSampleRate, float tuningFrequency, const float* chans,
                         const float* devs, uint32_t count, size_t firstSampleIndex, int32_t cudaDevice) {
  if (stream == nullptr) return hipErrorInvalidValue;
  *stream = nullptr;
  if (decimation == 0 || tapCount == 0 || taps == nullptr || count == 0) return hipErrorInvalidValue;
  if (kind != GSDRX_STREAM_FIR && kind != GSDRX_STREAM_FM && kind != GSDRX_STREAM_AM && kind != GSDRX_STREAM_XLATE) {
    return hipErrorInvalidValue;
  }
  if (sampleFormat != GSDRX_SAMPLES_CF32 && sampleFormat != GSDRX_SAMPLES_CS8) return hipErrorInvalidValue;
  gsdrxStream s = new (std::nothrow) gsdrxStream_t;
  if (s == nullptr) return hipErrorOutOfMemory;
  s->kind = kind;
  s->format = sampleFormat;
  s->D = decimation;
  s->taps = taps;
  s->T = tapCount;
  s->W = kind == GSDRX_STREAM_FM ? tapCount + decimation : tapCount;
  s->fs = rfSampleRate;
  s->tune = tuningFrequency;
  try {
    s->chans.assign(chans, chans + count);
    s->devs.assign(devs, devs + count);
  } catch (...) {
    delete s;
    return hipErrorOutOfMemory;
  }
  s->n0 = firstSampleIndex;
  s->device = cudaDevice;
  s->sb = sampleFormat == GSDRX_SAMPLES_CS8 ? 2 : 8;
  s->ob = (kind == GSDRX_STREAM_FIR || kind == GSDRX_STREAM_XLATE) ? 8 : 4;
  const hipError_t e =
      s->st.alloc(cudaDevice, stream_hist_capacity(1, s->W) * s->sb, stream_seam_capacity(1, s->W) * s->sb);
  if (e != hipSuccess) {
    (void)gsdrxStreamDestroy(s);
    return e;
  }
  *stream = s;
  return hipSuccess;
}
}  // namespace
}  // namespace gsdr

GSDR_C_LINKAGE hipError_t gsdrxStreamCreate(gsdrxStream* stream, int kind, int sampleFormat, uint32_t decimation,
                                            const float* taps, size_t tapCount, float rfSampleRate,
                                            float tuningFrequency, float channelFrequency, float frequencyDeviation,
                                            size_t firstSampleIndex, int32_t cudaDevice) GSDR_NO_EXCEPT {
  return gsdr::create_stream(stream, kind, sampleFormat, decimation, taps, tapCount, rfSampleRate, tuningFrequency,
                             &channelFrequency, &frequencyDeviation, 1, firstSampleIndex, cudaDevice);
}

GSDR_C_LINKAGE hipError_t gsdrxStreamCreateMulti(gsdrxStream* stream, int kind, int sampleFormat, uint32_t decimation,
                                                 const float* taps, size_t tapCount, float rfSampleRate,
                                                 float tuningFrequency, const float* channelFrequencies,
                                                 const float* frequencyDeviations, uint32_t numChannels,
                                                 size_t firstSampleIndex, int32_t cudaDevice) GSDR_NO_EXCEPT {
  if (stream != nullptr) *stream = nullptr;
  if (kind != GSDRX_STREAM_FM && kind != GSDRX_STREAM_AM && kind != GSDRX_STREAM_XLATE) return hipErrorInvalidValue;
  if (numChannels == 0 || channelFrequencies == nullptr) return hipErrorInvalidValue;
  if (kind == GSDRX_STREAM_FM && frequencyDeviations == nullptr) return hipErrorInvalidValue;
  std::vector<float> ones;
  if (frequencyDeviations == nullptr) {  // AM, XLATE: deviations unused
    try {
      ones.assign(numChannels, 1.0f);
    } catch (...) {
      return hipErrorOutOfMemory;
    }
    frequencyDeviations = ones.data();
  }
  return gsdr::create_stream(stream, kind, sampleFormat, decimation, taps, tapCount, rfSampleRate, tuningFrequency,
                             channelFrequencies, frequencyDeviations, numChannels, firstSampleIndex, cudaDevice);
}

GSDR_C_LINKAGE size_t gsdrxStreamOutputsFor(gsdrxStream s, size_t numInputSamples) GSDR_NO_EXCEPT {
  StreamPlan p;
  return s != nullptr && gsdr::plan_of(*s, numInputSamples, &p) ? (size_t)p.outputs : 0;
}

GSDR_C_LINKAGE hipError_t gsdrxStreamProcess(gsdrxStream s, const void* input, size_t numInputSamples, void* output,
                                             size_t outputCapacity, size_t* numOutputsWritten,
                                             hipStream_t cudaStream) GSDR_NO_EXCEPT {
  if (numOutputsWritten) *numOutputsWritten = 0;
  if (s == nullptr) return hipErrorInvalidValue;
  if (numInputSamples == 0) return hipSuccess;
  if (input == nullptr) return hipErrorInvalidValue;
  StreamPlan p;
  if (!gsdr::plan_of(*s, numInputSamples, &p)) return hipErrorInvalidValue;
  const size_t n_out = (size_t)p.outputs;
  if (n_out > outputCapacity || (n_out && output == nullptr)) return hipErrorInvalidValue;
  gsdr::DeviceScope scope(s->device);
  if (scope.status() != hipSuccess) return scope.status();
  const char* chunk = static_cast<const char*>(input);
  char* out = static_cast<char*>(output);
  const size_t C = s->chans.size();
  const size_t ostride = outputCapacity * s->ob;  // bytes between channels' output blocks
  const uint64_t S = s->st.consumed, h0 = p.first;  // = next_out * D
  hipError_t e = hipErrorNotSupported;  // (no one-launch step yet)
  if (n_out > 0) {
    // ONE launch (per channel, or per 16 channels on the grouped kernel) does the seam outputs (their samples
    // before the chunk read from the history buffer), the direct outputs and the next history copy: the int8
    // matrix-core kernels at decimation 4, the tiled kernels otherwise (the same kernels as one monolithic
    // call, tile for tile). Every channel reads the old history; only channel 0's launch writes the next one.
    gsdr::StreamOperands so{};
    so.chunk = chunk;
    so.chunk_len = numInputSamples;
    so.in_off = (int64_t)h0 - (int64_t)S;
    so.hist = s->st.hist;
    so.hist_len = p.hist;
    so.hist_out = s->st.spare;
    so.hist_from = (int64_t)p.first_after - (int64_t)S;
    so.hist_n = p.hist_after;
    // (the chain part is unused by a FIR stream)
    const int mode = s->kind == GSDRX_STREAM_FM      ? gsdr::kModeFm
                     : s->kind == GSDRX_STREAM_XLATE ? gsdr::kModeIq
                                                     : gsdr::kModeAm;
    const gsdr::ChainSpec cs{mode, s->fs, s->tune, s->D, s->n0 + h0, s->taps, s->T};
    if (C > 1 && s->format != GSDRX_SAMPLES_CS8) {
      gsdr::ChainMultiStep* step =
          s->kind == GSDRX_STREAM_XLATE ? gsdr::xlate_multi_stream_step : gsdr::chain_multi_stream_step;
      e = step(cs, s->chans.data(), s->devs.data(), (uint32_t)C, so, out, outputCapacity, n_out, s->device, cudaStream);
    }
    // otherwise one launch per channel; a shape without a one-launch step returns hipErrorNotSupported from
    // channel 0, before anything was launched, and the call takes the seam path below
    for (size_t c = 0; c < C && e == hipErrorNotSupported; ++c) {
      const hipError_t ec = gsdr::channel_step(*s, cs, c, so, out + c * ostride, n_out, cudaStream);
      so.hist_out = nullptr;  // the channels after the first only read the old history
      if (ec == hipErrorNotSupported && c == 0) break;
      // a failure after channel 0 leaves channels 0..c-1 written and the stream unchanged (stream.h: the
      // outputs of a failed call are unspecified)
      if (ec != hipSuccess) {
        e = ec == hipErrorNotSupported ? hipErrorUnknown : ec;  // (one shape for every channel: cannot happen)
        break;
      }
      if (c + 1 == C) e = hipSuccess;
    }
  }
  if (e == hipErrorNotSupported) {
    // not this shape, or only samples to keep: the seam plan through the filter calls
    e = gsdr::stream_seam_plan(s->st, p, chunk, numInputSamples, s->sb, C, cudaStream,
                               [&](size_t c, const char* in, uint64_t k, uint64_t n) {
                                 return gsdr::filter(*s, c, in, s->n0 + h0 + k * s->D, out + c * ostride + k * s->ob, n,
                                                     cudaStream);
                               });
  }
  if (e != hipSuccess) return e;
  s->st.commit(p, numInputSamples);
  if (numOutputsWritten) *numOutputsWritten = n_out;
  return hipSuccess;
}

GSDR_C_LINKAGE hipError_t gsdrxStreamDestroy(gsdrxStream s) GSDR_NO_EXCEPT {
  if (s == nullptr) return hipSuccess;
  const hipError_t e = s->st.release(s->device);
  delete s;
  return e;
}
