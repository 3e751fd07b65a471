/*
 * gsdr-mi355x extension: a streaming rational resampler, the stream form of gsdrxResampleFF / gsdrxResampleFC
 * (gsdr_ext.h) as gsdrxStream (stream.h) is the stream form of the FIR, FM, AM and frequency-translating chains.
 *
 * The one-shot calls leave a stream's bookkeeping to the caller: keep the last ceil(T / L) samples of every chunk,
 * paste them in front of the next one, track U = phase0 + m0 * M and pass input + U / L and U mod L by hand (as
 * the reference leaves the overlap to its callers, include/gsdr/fm.h:26). A gsdrxResampler object does it on the
 * device: it keeps the samples the next output still needs in a small device buffer, and a call is ONE kernel
 * launch: the tiled kernel of the one-shot call, whose first tiles stage their samples from two places (the kept
 * history, then the caller's chunk), while one more workgroup of the same launch copies the next history. (A call
 * that writes no output but has history to move is one small copy launch. Shapes the one-shot call serves with
 * its generic kernel, and interpolation == 1, which is gsdrFirFF / gsdrFirFC, take three launches: history + chunk
 * head gathered into a seam buffer, then the outputs that start in the history and the remaining outputs as two
 * one-shot calls.)
 *
 * Contract: with L = interpolation, M = decimation, T = numTaps and phase0 = phase, feeding a stream x[0..S) in
 * chunks of any sizes (including 0, 1 and chunks shorter than a window) produces, concatenated over the calls,
 * exactly the outputs of ONE gsdrxResampleFF / FC(L, M, phase0, taps, T, x, N) call -- bit for bit -- where N is
 * the largest count with gsdrxResampleInputsFor(L, M, phase0, T, N) <= S. (The stream runs the kernel the one-shot
 * call runs: it is chosen from (L, M, T, sample type) alone, and every output is one ascending fmaf chain from +0
 * whatever the tile or the call it falls into.) Output m is written by the first call after which
 * floor((phase0 + m * M + T - 1) / L) + 1 samples have arrived, the InputsFor rule applied per output; an output
 * whose window holds no tap (T < L) follows the same rule and is +0.
 *
 * State between calls: the 64-bit counts of samples consumed and outputs written, and the samples the next
 * output m still needs, x[ceil(s / L) .. consumed) with s = phase0 + m * M: at most ceil(T / L) - 1 of them. When
 * M / L is large that first sample may lie beyond `consumed`: the history is then empty and the samples up to it
 * are skipped in the coming chunks.
 *
 * Threading and streams: as stream.h. The history lives in two device buffers used alternately (a call reads the
 * previous call's and writes the other one); nothing is allocated after creation and there is no event or host
 * synchronisation between calls, so the calls on one object are ordered only by the HIP stream they share: every
 * gsdrxResamplerProcess call on one object must be given the SAME hipStream_t (synchronise the old one before
 * moving an object to another). Do not call one object from two host threads concurrently. The taps buffer is the
 * caller's and must stay valid while the object is used.
 */
#ifndef GSDR_RESAMPLER_H_
#define GSDR_RESAMPLER_H_

#include <gsdr/gsdr_export.h>
#include <gsdr/util.h>
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#define GSDRX_RESAMPLER_F32 0  /* float samples:           the stream form of gsdrxResampleFF */
#define GSDRX_RESAMPLER_CF32 1 /* hipFloatComplex samples: the stream form of gsdrxResampleFC */

typedef struct gsdrxResampler_t* gsdrxResampler;

/**
 * Create a resampler on `cudaDevice`: two history buffers of ceil(numTaps / interpolation) samples and a seam
 * buffer of twice that; nothing is allocated later. `phase` in [0, interpolation) is output 0's offset in the
 * zero-stuffed stream, as in gsdrxResampleFF. Returns hipErrorInvalidValue, before any device call, for a null
 * handle pointer, an unknown sampleType, interpolation == 0, decimation == 0, phase >= interpolation, null taps or
 * numTaps == 0.
 */
GSDR_C_LINKAGE GSDR_PUBLIC hipError_t gsdrxResamplerCreate(
    gsdrxResampler* resampler,
    int sampleType,
    uint32_t interpolation,
    uint32_t decimation,
    uint32_t phase,
    const float* taps,
    size_t numTaps,
    int32_t cudaDevice) GSDR_NO_EXCEPT;

/** Number of outputs the next gsdrxResamplerProcess call with `numInputSamples` samples will write (0 for null). */
GSDR_C_LINKAGE GSDR_PUBLIC size_t gsdrxResamplerOutputsFor(gsdrxResampler resampler, size_t numInputSamples)
    GSDR_NO_EXCEPT;

/**
 * Append `numInputSamples` samples (device memory, float or hipFloatComplex by the sample type, at any 4- or
 * 8-byte alignment) and write every output that became computable to `output`, in order. Nothing outside
 * [input, input + numInputSamples) and the object's own buffers is read. `*numOutputsWritten` (may be null)
 * receives the count: host-known, no synchronisation. Asynchronous on `cudaStream`; the chunk may be reused once
 * the stream's work has completed.
 * Returns hipErrorInvalidValue, with the object unchanged, for a null object, a null input with
 * numInputSamples > 0, a null output when outputs are due, outputCapacity below the outputs due, and when the
 * zero-stuffed index phase0 + m * M + numTaps of an output of this call or of the next one would leave 63 bits. On
 * a launch error the state is also unchanged and the same chunk can be passed again (the contents of `output`
 * are then unspecified).
 */
GSDR_C_LINKAGE GSDR_PUBLIC hipError_t gsdrxResamplerProcess(
    gsdrxResampler resampler,
    const void* input,
    size_t numInputSamples,
    void* output,
    size_t outputCapacity,
    size_t* numOutputsWritten,
    hipStream_t cudaStream) GSDR_NO_EXCEPT;

/** Free the object's device buffers (synchronises the device, as hipFree does). Null is a no-op: hipSuccess. */
GSDR_C_LINKAGE GSDR_PUBLIC hipError_t gsdrxResamplerDestroy(gsdrxResampler resampler) GSDR_NO_EXCEPT;

/**
 * The host-side plan of one Process call, exposed so that it can be tested without a GPU: a pure function of
 * L = interpolation, M = decimation, T = numTaps, phase0, the samples consumed so far, the index of the next
 * output and the chunk length.
 *   plan[0] = outputs of this call;
 *   plan[1] = how many of them (the first ones) start in the history: the seam outputs;
 *   plan[2] = history samples in use before the call;
 *   plan[3] = samples at the head of the chunk skipped before the first one any output reads (the whole chunk
 *             when that sample lies beyond it);
 *   plan[4] = history length after the call;
 *   plan[5] = samples of later chunks still to skip after the call.
 * The next history is the tail of the chunk, or the tail of the old history plus the whole chunk when the chunk
 * is shorter than what is kept, or empty. All six are 0 for arguments the object rejects (L, M or T == 0,
 * phase0 >= L, an index that leaves 63 bits) and for a null `plan` nothing is written.
 */
GSDR_C_LINKAGE GSDR_PUBLIC void gsdrxResamplerPlan(
    uint32_t interpolation,
    uint32_t decimation,
    uint64_t numTaps,
    uint32_t phase,
    uint64_t consumed,
    uint64_t nextOutput,
    uint64_t chunk,
    uint64_t plan[6]) GSDR_NO_EXCEPT;

#endif /* GSDR_RESAMPLER_H_ */
