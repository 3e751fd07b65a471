// gsdr-mi355x: the device side both streaming objects share (gsdrxStream in stream.hip, gsdrxResampler in
// resample.hip): the position and the three buffers a stream keeps between calls, the one launch that carries out a
// move list of stream_plan.hpp, and the seam plan for shapes without a one-launch kernel.
#pragma once

#include <initializer_list>
#include <utility>

#include "launch.hpp"
#include "stream_plan.hpp"

namespace gsdr {

struct StreamState {
  uint64_t consumed = 0;  // samples that have arrived
  uint64_t next_out = 0;  // outputs written
  char* hist = nullptr;   // x[first(next_out) .. consumed) (empty when that lies beyond)
  char* spare = nullptr;  // the other history buffer (ping-pong)
  char* seam = nullptr;   // seam plan: history + chunk head for the outputs that start in the history

  hipError_t alloc(int32_t device, size_t hist_bytes, size_t seam_bytes) {
    DeviceScope scope(device);
    hipError_t e = scope.status();
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&hist), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&spare), hist_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&seam), seam_bytes);
    return e;
  }
  // the first hipFree error, every buffer tried
  hipError_t release(int32_t device) {
    DeviceScope scope(device);
    hipError_t e = scope.status();
    if (e != hipSuccess) return e;
    for (char* b : {hist, spare, seam}) {
      const hipError_t f = b ? hipFree(b) : hipSuccess;
      if (e == hipSuccess) e = f;
    }
    return e;
  }
  void swap() { std::swap(hist, spare); }
  // after every launch of the call has succeeded: the spare buffer holds the next history
  void commit(const StreamPlan& sp, uint64_t chunk) {
    if (sp.hist_after) swap();
    consumed += chunk;
    next_out += sp.outputs;
  }
  char* at(StreamBuffer b, const void* chunk) const {
    return b == kHist ? hist : b == kSpare ? spare : b == kSeam ? seam : static_cast<char*>(const_cast<void*>(chunk));
  }
};

// p + n samples of sb bytes, n possibly negative: the origin of a virtual input, formed without stepping a pointer
// outside its buffer (only addresses inside the chunk are ever read through it)
inline const char* offset_by(const char* p, int64_t n, size_t sb) {
  return reinterpret_cast<const char*>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)n * sb);
}

// One launch for a move list, samples of sb bytes (stream.hip); nothing launched for an empty list.
hipError_t stream_move(const StreamState& b, const StreamMoves& mv, const void* chunk, size_t sb, hipStream_t st);

// The seam plan: history + chunk head gathered into the seam buffer (with the next history, one launch), then, a
// channel, the outputs that start in the history and the remaining ones as two one-shot calls.
// one_shot(c, in, k, n): outputs [k, k + n) of the call for channel c, `in` placed at x[origin] of output k.
template <class OneShot>
hipError_t stream_seam_plan(const StreamState& b, const StreamPlan& sp, const char* chunk, uint64_t len, size_t sb,
                            size_t channels, hipStream_t st, OneShot one_shot) {
  StreamMoves mv;
  stream_seam(sp, &mv);
  stream_next_history(sp, len, &mv);
  hipError_t e = stream_move(b, mv, chunk, sb, st);
  for (size_t c = 0; c < channels && e == hipSuccess; ++c) {
    if (sp.seam) e = one_shot(c, b.seam, 0, sp.seam);
    if (e == hipSuccess && sp.outputs > sp.seam) {
      e = one_shot(c, offset_by(chunk, sp.main_off, sb), sp.seam, sp.outputs - sp.seam);
    }
  }
  return e;
}

}  // namespace gsdr
