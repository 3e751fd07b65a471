// gsdr-mi355x: what crosses translation units between the streaming object (stream.hip) and the files that
// launch the filter kernels (fir.hip, fir_int8.hip, fm_am.hip, xlate.hip). Kept free of the kernel headers, so
// stream.hip stays cheap to compile; the defining files include it too, so a signature that drifts does not compile.
#pragma once

#include <hip/hip_complex.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fir_plan.hpp"

namespace gsdr {

// (enum Mode { kModeFir, kModeFm, kModeAm, kModeIq }: fir_plan.hpp)

// One streaming step's input (FirParams, fir_nco.hpp): output 0's window starts at sample in_off of the
// chunk (negative: in the history `hist` of hist_len samples, chunk offset i < 0 being hist[hist_len + i]);
// workgroup 0 of the launch copies chunk offsets [hist_from, hist_from + hist_n) to hist_out, the next
// history (nullptr: no copy).
struct StreamOperands {
  const void* chunk;
  uint64_t chunk_len;
  int64_t in_off;
  const void* hist;
  uint64_t hist_len;
  void* hist_out;
  int64_t hist_from;
  uint64_t hist_n;
};

// A chain (FM, AM or the frequency-translating FIR) without its channel: firstSampleIndex is the absolute index of
// output 0's first sample.
struct ChainSpec {
  int mode;  // kModeFm, kModeAm or kModeIq
  float fs, tune;
  uint32_t decimation;
  uint64_t firstSampleIndex;
  const float* taps;
  size_t tapCount;
};

// fir_int8.hip: gsdrxFirFCInt8 for outputs whose absolute index (counted from the stream's first output)
// starts at outputIndex. The decimation-4 matrix-core kernel aligns its 16-output blocks to that index, so
// chunked calls reproduce one call bit for bit (fir_i8_mfma.hpp).
hipError_t fir_int8_at(uint64_t outputIndex, size_t decimation, const float* taps, size_t tapCount,
                       const int8_t* input, hipFloatComplex* output, size_t numOutputs, int32_t device,
                       hipStream_t stream);

// The one-launch steps. Each returns hipErrorNotSupported, with nothing launched, for a shape it does not
// take; the stream then tries the next step and at last its seam plan.
// int8 I/Q on the matrix cores at decimation 4: fir_int8.hip, fm_am.hip
hipError_t fir_int8_stream_step(uint64_t outputIndex, size_t decimation, const float* taps, size_t tapCount,
                                const StreamOperands& so, hipFloatComplex* output, size_t numOutputs, int32_t device,
                                hipStream_t stream);
hipError_t chain_int8_stream_step(const ChainSpec& cs, float chan, float dev, const StreamOperands& so, float* output,
                                  size_t numOutputs, int32_t device, hipStream_t stream);
// the tiled kernels (fir_dispatch.hpp stream_step_tiled): fir.hip, fir_int8.hip, fm_am.hip
hipError_t fir_fc_stream_step(size_t decimation, const float* taps, size_t tapCount, const StreamOperands& so,
                              hipFloatComplex* output, size_t numOutputs, int32_t device, hipStream_t stream);
hipError_t fir_int8_stream_step_tiled(size_t decimation, const float* taps, size_t tapCount, const StreamOperands& so,
                                      hipFloatComplex* output, size_t numOutputs, int32_t device, hipStream_t stream);
// The chains' steps (chain_job.hpp) come once per unit that holds chain kernels -- fm_am.hip (cs.mode kModeFm or
// kModeAm, float outputs) and xlate.hip (kModeIq, complex outputs; dev / devs unused) -- with one parameter list.
using ChainStepTiled = hipError_t(const ChainSpec& cs, bool int8, float chan, float dev, const StreamOperands& so,
                                  void* output, size_t numOutputs, int32_t device, hipStream_t stream);
// the grouped multi-channel kernel on complex float chunks, channel c's outputs at element c * outStride of output
using ChainMultiStep = hipError_t(const ChainSpec& cs, const float* chans, const float* devs, uint32_t count,
                                  const StreamOperands& so, void* output, size_t outStride, size_t numOutputs,
                                  int32_t device, hipStream_t stream);
ChainStepTiled chain_stream_step_tiled, xlate_stream_step_tiled;
ChainMultiStep chain_multi_stream_step, xlate_multi_stream_step;

}  // namespace gsdr
