// gsdr-mi355x: polyphase rational (L / M) resampling FIR -- gsdrxResampleFF / FC / InputsFor
// (include/gsdr/gsdr_ext.h). With s(m) = phase + m M the start of output m's window in the zero-stuffed stream,
//     i0 = (L - s mod L) mod L,  n0 = (s + i0) / L,  output[m] = sum_{p, i0 + p L < T} taps[i0 + p L] input[n0 + p]:
// only the taps that meet a real sample are multiplied. Every output component is one ascending-p fmaf chain from
// +0 in both kernels, so the bits depend on neither the route, the tile size nor where a stream is cut into calls.
// The launch plan is resample_plan.hpp.
//
// gsdrxResampler (include/gsdr/resampler.h) is the stream form: the host bookkeeping of every stream
// (stream_plan.hpp, stream_buffers.hpp) around the same kernels. On the tile route a call is one launch of k_resample_tile<S, true>, which stages a tile from
// the kept history and then from the caller's chunk, with one appended workgroup that copies the next history.
#include <hip/hip_runtime.h>

#include <new>
#include <type_traits>

#include "gsdr/fir.h"
#include "gsdr/gsdr_ext.h"
#include "gsdr/resampler.h"
#include "launch.hpp"
#include "resample_plan.hpp"
#include "stream_buffers.hpp"

namespace gsdr {
namespace resample {

struct Params {
  const void* in;
  const float* taps;
  void* out;
  uint64_t N;      // outputs
  uint64_t need;   // input samples the call reads (gsdrxResampleInputsFor)
  uint64_t phase;  // q < L
  uint64_t T;
  uint32_t L, M;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// A sample in registers: float, or the two floats of a complex sample as one vector (float2's layout)
template <class S>
struct Value {
  using type = float;
};
template <>
struct Value<float2> {
  using type = f32x2;
};

// acc += t * x, one rounding a component; complex samples take one v_pk_fma_f32 with the tap in both halves
__device__ __forceinline__ void mac(float& acc, float t, float x) { acc = fmaf(t, x, acc); }
__device__ __forceinline__ void mac(f32x2& acc, float t, f32x2 x) {
  acc = __builtin_elementwise_fma(f32x2{t, t}, x, acc);
}

#define GSDR_LDS __attribute__((address_space(3)))

// Copies src[0, count) to dst[off, off + count) of LDS, off = src's element offset inside its 16-byte granule of
// global memory (dst is 16-byte aligned): granules wholly inside the range move with one 16-byte load, the ragged
// head and tail element by element. Nothing outside src[0, count) is read.
template <bool NT, class E>
__device__ __forceinline__ void stage(E* dst, const E* __restrict__ src, uint32_t off, uint32_t count, uint32_t tid,
                                      uint32_t wg) {
  constexpr uint32_t G = 16 / sizeof(E);
  const uint32_t end = off + count;
  const f32x4* src16 = reinterpret_cast<const f32x4*>(reinterpret_cast<uintptr_t>(src) - off * sizeof(E));
  for (uint32_t g = tid; g * G < end; g += wg) {
    const uint32_t lo = g * G;
    if (lo >= off && lo + G <= end) {
      reinterpret_cast<f32x4*>(dst)[g] = NT ? __builtin_nontemporal_load(src16 + g) : src16[g];
    } else {
      for (uint32_t e = lo < off ? off : lo; e < lo + G && e < end; ++e) dst[e] = src[e - off];
    }
  }
}

template <class E>
__device__ __forceinline__ uint32_t granule_offset(const E* p) {
  return (uint32_t)(reinterpret_cast<uintptr_t>(p) / sizeof(E)) % (uint32_t)(16 / sizeof(E));
}

// What the tiled kernel would otherwise divide for: quotients by L of values the host knows (L >= 2 here).
struct TileArgs {
  uint32_t span;      // the plan's span (LDS samples before the taps)
  uint32_t magic;     // floor(2^32 / L): div_l
  uint32_t full;      // T / L: steps every output takes
  uint32_t most;      // ceil(T / L): samples an output reads at most
  uint32_t tile_q, tile_r;  // (KT M) / L and (KT M) mod L: the zero-stuffed distance between tiles
  uint32_t step_q, step_r;  // (WG M) / L and (WG M) mod L: between a thread's outputs
};

// u / L and u mod L for u < 2^32, L in [2, 2^31): e = mulhi(u, floor(2^32 / L)) is the quotient or one less
// (u / L - 1 < u floor(2^32 / L) / 2^32 <= u / L), so one correction step.
__device__ __forceinline__ uint32_t div_l(uint32_t u, uint32_t L, uint32_t magic, uint32_t* rem) {
  uint32_t e = __umulhi(u, magic), r = u - e * L;
  if (r >= L) {
    r -= L;
    e += 1;
  }
  *rem = r;
  return e;
}

// The next-history moves of one streaming call (stream_next_history, stream_plan.hpp) as the tiled kernel's appended
// workgroup takes them: in 4-byte words, a sample is one or two of them.
struct Moves {
  static constexpr int kMax = 4;
  struct Seg {
    float* dst;
    const float* src;
    uint64_t words;
  } seg[kMax];
  int n = 0;
  void add(void* dst, const void* src, uint64_t words) {
    if (words) seg[n++] = Seg{static_cast<float*>(dst), static_cast<const float*>(src), words};
  }
};

__device__ __forceinline__ void move_words(const Moves& mv, uint64_t first, uint64_t stride) {
  for (int i = 0; i < mv.n; ++i) {
    for (uint64_t k = first; k < mv.seg[i].words; k += stride) mv.seg[i].dst[k] = mv.seg[i].src[k];
  }
}

// What a streaming launch of the tiled kernel adds. The call's input is the virtual array history ++ chunk: Params::in
// is placed so that in[n] is the chunk's sample for n >= split, and in[n] for hist_first <= n < split is
// hist[n - hist_first] (hist_first = 0 or 1: index 0 is never read when the call's phase is not 0).
struct StreamArgs {
  const void* hist;
  uint64_t split;
  uint32_t hist_first;
  uint32_t tiles;  // workgroups that compute; workgroup `tiles` copies the next history
  Moves next;
};
struct NoStream {};

// One workgroup a tile of KT = kR * blockDim.x consecutive outputs: the tile's input span and all T taps are staged
// into LDS, then thread `tid` computes outputs tid, tid + WG, ... of the tile (coalesced stores). Lane j's tap
// reads taps[i0(j) + p L]: the taps' natural order is the [p][phase] layout. The first T / L steps meet a tap for
// every output; step T / L only for outputs with i0 + (T / L) L < T, and no product past tap T - 1 is formed.
// STREAM (gsdrxResamplerProcess): the part of a tile's span in front of the chunk, fewer than ceil(T / L) samples and
// met only by the first tiles, comes from the history element by element, placed so that the chunk part keeps the
// granule staging; the LDS image holds the values of the one-shot call, so the outputs' bits are that call's.
template <class S, bool STREAM>
__global__ __launch_bounds__(kMaxWG) void k_resample_tile(const Params p, const TileArgs a,
                                                          const std::conditional_t<STREAM, StreamArgs, NoStream> sa) {
  extern __shared__ f32x4 lds16[];
  const uint32_t tid = threadIdx.x, wg = blockDim.x, KT = kR * wg;
  if constexpr (STREAM) {
    if (blockIdx.x == sa.tiles) {
      move_words(sa.next, tid, wg);
      return;
    }
  }
  const uint32_t L = p.L, M = p.M, T = (uint32_t)p.T;
  const uint64_t m0 = (uint64_t)blockIdx.x * KT;
  const uint32_t kt = p.N - m0 < KT ? (uint32_t)(p.N - m0) : KT;  // outputs of this tile (>= 1)

  // the tile's base, once per workgroup in 64 bits: s(m0) = phase + b (KT M) = d0 L + r0, first sample n_first =
  // ceil(s(m0) / L). With KT M = tile_q L + tile_r only phase + b tile_r is left to divide, in 32 bits when it fits.
  const uint64_t v = p.phase + (uint64_t)blockIdx.x * a.tile_r;
  uint64_t d0 = (uint64_t)blockIdx.x * a.tile_q;
  uint32_t r0;
  if ((v >> 32) == 0) {
    d0 += div_l((uint32_t)v, L, a.magic, &r0);
  } else {
    const uint64_t dq = v / L;
    d0 += dq;
    r0 = (uint32_t)(v - dq * L);
  }
  const uint32_t up0 = r0 != 0 ? 1u : 0u;
  const uint64_t n_first = d0 + up0;

  // samples the tile reads: through the last output's ceil(T / L), within the call's input
  const uint32_t u_last = r0 + (kt - 1) * M;  // < L + KT M < 2^32 (tile_fits)
  uint32_t rm_last;
  const uint32_t qd_last = div_l(u_last, L, a.magic, &rm_last);
  uint32_t count = qd_last + (rm_last != 0 ? 1u : 0u) - up0 + a.most;
  const uint64_t left = p.need > n_first ? p.need - n_first : 0;
  if (count > left) count = (uint32_t)left;

  constexpr uint32_t G = 16 / sizeof(S);
  S* xs = reinterpret_cast<S*>(lds16);
  float* ts = reinterpret_cast<float*>(lds16 + ((size_t)(a.span + G - 1) * sizeof(S) + 15) / 16);
  const uint32_t toff = granule_offset(p.taps);
  uint32_t xoff;
  // the samples stream through once (non-temporal); every workgroup reads the taps again (cached)
  if constexpr (STREAM) {
    const uint64_t ahead = sa.split > n_first ? sa.split - n_first : 0;  // samples in front of the chunk
    const uint32_t hc = count < ahead ? count : (uint32_t)ahead;
    const S* src = static_cast<const S*>(p.in) + (n_first + hc);
    const uint32_t coff = granule_offset(src);
    xoff = (coff - hc) % G;  // the chunk part lands at its own granule offset, coff = (xoff + hc) mod G
    // a thread's (first) history sample is loaded ahead of its chunk granules and stored behind them, so that the
    // first tile pays one trip to memory for both and not one after the other
    const S* hs = static_cast<const S*>(sa.hist) + (n_first - sa.hist_first);
    S mine = S();
    if (tid < hc) mine = hs[tid];
    if (count > hc) stage<true>(xs + (xoff + hc - coff), src, coff, count - hc, tid, wg);
    if (tid < hc) xs[xoff + tid] = mine;
    for (uint32_t e = tid + wg; e < hc; e += wg) xs[xoff + e] = hs[e];
  } else {
    const S* src = static_cast<const S*>(p.in) + n_first;
    xoff = granule_offset(src);
    if (count > 0) stage<true>(xs, src, xoff, count, tid, wg);
  }
  stage<false>(ts, p.taps, toff, T, tid, wg);
  __syncthreads();

  // output k = tid + r wg of the tile: u = r0 + k M = qd L + rm, i0 = (L - rm) mod L, sample n_first + qd + (rm != 0)
  // - up0. One division per thread; the step from r to r + 1 is (wg M) / L and (wg M) mod L with a carry.
  uint32_t rm;
  uint32_t qd = div_l(r0 + tid * M, L, a.magic, &rm);
  using V = typename Value<S>::type;
  const GSDR_LDS float* tp[kR];  // the output's next tap and next sample, as 32-bit LDS addresses
  const GSDR_LDS V* xp[kR];
  bool last[kR];
  const uint32_t full = a.full;
#pragma unroll
  for (uint32_t r = 0; r < kR; ++r) {
    if (tid + r * wg >= kt) {  // past a ragged tile: repeat its last output (staged indices), store nothing
      qd = qd_last;
      rm = rm_last;
    }
    const uint32_t i0 = rm != 0 ? L - rm : 0u;
    tp[r] = (const GSDR_LDS float*)ts + (toff + i0);
    xp[r] = (const GSDR_LDS V*)xs + (xoff + qd + (rm != 0 ? 1u : 0u) - up0);
    last[r] = i0 + full * L < T;  // full L <= T < 2^15, i0 < L < 2^31
    qd += a.step_q;
    rm += a.step_r;
    if (rm >= L) {
      rm -= L;
      qd += 1;
    }
  }

  V acc[kR];
#pragma unroll
  for (uint32_t r = 0; r < kR; ++r) acc[r] = V(0.0f);
  // a step: the 2 kR LDS reads of all chains first (their addresses are ready), then the kR MACs and the pointers'
  // steps: the reads' latency is paid once a step, not once a MAC
  for (uint32_t pp = 0; pp < full; ++pp) {
    float t[kR];
    V x[kR];
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r) {
      t[r] = *tp[r];
      x[r] = *xp[r];
    }
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r) {
      mac(acc[r], t[r], x[r]);
      tp[r] += L;
      xp[r] += 1;
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * kR, 0);  // DS reads
    __builtin_amdgcn_sched_group_barrier(0x002, 3 * kR, 0);  // VALU
  }
#pragma unroll
  for (uint32_t r = 0; r < kR; ++r) {
    if (last[r]) mac(acc[r], *tp[r], *xp[r]);
  }

  V* out = static_cast<V*>(p.out) + m0;
#pragma unroll
  for (uint32_t r = 0; r < kR; ++r) {
    const uint32_t k = tid + r * wg;
    if (k < kt) out[k] = acc[r];
  }
}

// One output per thread straight from global memory, every index in 64 bits: shapes whose taps or tile span do
// not fit in LDS.
template <class S>
__global__ __launch_bounds__(kGenericWG) void k_resample_generic(const Params p) {
  const uint64_t m = (uint64_t)blockIdx.x * kGenericWG + threadIdx.x;
  if (m >= p.N) return;
  const uint64_t s = p.phase + m * p.M;
  const uint64_t d = s / p.L, rm = s - d * p.L;
  using V = typename Value<S>::type;
  const V* __restrict__ x = static_cast<const V*>(p.in) + d + (rm != 0 ? 1 : 0);
  const float* __restrict__ t = p.taps;
  V acc = V(0.0f);
  for (uint64_t i = rm != 0 ? p.L - rm : 0; i < p.T; i += p.L) mac(acc, t[i], *x++);
  static_cast<V*>(p.out)[m] = acc;
}

// sa: the streaming operands of a tile-route launch (one more workgroup), null for a one-shot call
template <class S>
static hipError_t launch(const Params& p, const Plan& pl, hipStream_t stream, const StreamArgs* sa = nullptr) {
  if (pl.route == kRouteTile) {
    TileArgs a;
    a.span = pl.span;
    a.magic = (uint32_t)((1ull << 32) / p.L);
    a.full = (uint32_t)(p.T / p.L);
    a.most = (uint32_t)ceil_div64(p.T, p.L);
    const uint32_t tile = pl.kt * p.M, step = pl.wg * p.M;  // < 2^31 (tile_fits)
    a.tile_q = tile / p.L;
    a.tile_r = tile % p.L;
    a.step_q = step / p.L;
    a.step_r = step % p.L;
    if (sa != nullptr) {
      StreamArgs st = *sa;
      st.tiles = (uint32_t)pl.blocks;
      k_resample_tile<S, true><<<dim3((uint32_t)pl.blocks + 1), dim3(pl.wg), pl.lds_bytes, stream>>>(p, a, st);
    } else {
      k_resample_tile<S, false><<<dim3((uint32_t)pl.blocks), dim3(pl.wg), pl.lds_bytes, stream>>>(p, a, NoStream{});
    }
  } else {
    k_resample_generic<S><<<dim3((uint32_t)pl.blocks), dim3(pl.wg), 0, stream>>>(p);
  }
  return launch_status();
}

static size_t inputs_for(uint64_t L, uint64_t extent) { return extent == 0 ? 0 : (size_t)((extent - 1) / L + 1); }

template <class S>
static hipError_t entry(uint32_t L, uint32_t M, uint32_t phase, const float* taps, size_t T, const S* input, S* output,
                        size_t N, int32_t device, hipStream_t stream) {
  if (N == 0) return hipSuccess;
  if (L == 0 || M == 0 || phase >= L) return hipErrorInvalidValue;
  if (input == nullptr || output == nullptr || (T > 0 && taps == nullptr)) return hipErrorInvalidValue;
  uint64_t extent = 0;
  if (!stuffed_extent(phase, M, T, N, &extent)) return hipErrorInvalidValue;
  if (L == 1) {
    // plain decimation: the FIR engine's kernels, bit for bit (fir_entry<float, S>)
    if constexpr (sizeof(S) == sizeof(float)) {
      return gsdrFirFF(M, taps, T, input, output, N, device, stream);
    } else {
      return gsdrFirFC(M, taps, T, reinterpret_cast<const hipFloatComplex*>(input),
                       reinterpret_cast<hipFloatComplex*>(output), N, device, stream);
    }
  }
  Plan pl{};
  if (T > 0 && !plan(L, M, T, sizeof(S), N, &pl)) return hipErrorInvalidValue;  // more outputs than one launch takes
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  if (T == 0) {  // no tap: every output is zero, as fir_entry
    const hipError_t st = hipMemsetAsync(output, 0, N * sizeof(S), stream);
    return st != hipSuccess ? st : launch_status();
  }
  Params p{};
  p.in = input;
  p.taps = taps;
  p.out = output;
  p.N = N;
  p.need = inputs_for(L, extent);
  p.phase = phase;
  p.T = T;
  p.L = L;
  p.M = M;
  return launch<S>(p, pl, stream);
}

}  // namespace resample
}  // namespace gsdr

struct gsdrxResampler_t {
  uint32_t L = 1, M = 1, phase0 = 0;
  const float* taps = nullptr;
  size_t T = 0;
  int32_t device = 0;
  size_t sb = 4;       // bytes per sample
  bool tiled = false;  // one launch a call (k_resample_tile<S, true>); else the seam plan through the one-shot calls
  gsdr::StreamState st;  // history: x[ceil(s / L) .. consumed), s = phase0 + next_out M
};

namespace gsdr {
namespace resample {

template <class S>
static hipError_t process(gsdrxResampler_t& r, const StreamPlan& sp, const char* chunk, uint64_t len, S* out,
                          hipStream_t stream) {
  const uint64_t s = r.phase0 + r.st.next_out * r.M;  // (the plan checked it)
  if (sp.outputs == 0 || !r.tiled) {
    // the seam plan through the one-shot calls (only samples to keep: its move launch alone)
    const auto one_shot = [&](size_t, const char* in, uint64_t k, uint64_t n) {
      return entry<S>(r.L, r.M, (uint32_t)((s + k * r.M) % r.L), r.taps, r.T, reinterpret_cast<const S*>(in), out + k, n,
                      r.device, stream);
    };
    return stream_seam_plan(r.st, sp, chunk, len, sizeof(S), 1, stream, one_shot);
  }
  // ONE launch: the one-shot call at output next_out (origin x[s / L], phase s mod L) over history ++ chunk
  const uint64_t Sx = r.st.consumed, origin = s / r.L;
  uint64_t extent = 0;
  Plan pl{};
  if (!stuffed_extent(s % r.L, r.M, r.T, sp.outputs, &extent) || !plan(r.L, r.M, r.T, sizeof(S), sp.outputs, &pl)) {
    return hipErrorInvalidValue;
  }
  Params p{};
  p.in = offset_by(chunk, (int64_t)(origin - Sx), sizeof(S));
  p.taps = r.taps;
  p.out = out;
  p.N = sp.outputs;
  p.need = inputs_for(r.L, extent);
  p.phase = s % r.L;
  p.T = r.T;
  p.L = r.L;
  p.M = r.M;
  StreamArgs sa{};
  sa.hist = r.st.hist;
  sa.split = Sx > origin ? Sx - origin : 0;
  sa.hist_first = (uint32_t)sp.lead;  // 0 or 1
  StreamMoves next;
  stream_next_history(sp, len, &next);
  for (int i = 0; i < next.n; ++i) {
    const StreamMoves::Seg& m = next.seg[i];
    sa.next.add(r.st.at(m.dst, chunk) + m.dst_off * sizeof(S), r.st.at(m.src, chunk) + m.src_off * sizeof(S),
                m.count * (sizeof(S) / 4));
  }
  return launch<S>(p, pl, stream, &sa);
}

}  // namespace resample
}  // namespace gsdr

GSDR_C_LINKAGE hipError_t gsdrxResamplerCreate(gsdrxResampler* resampler, int sampleType, uint32_t interpolation,
                                               uint32_t decimation, uint32_t phase, const float* taps, size_t numTaps,
                                               int32_t cudaDevice) GSDR_NO_EXCEPT {
  if (resampler == nullptr) return hipErrorInvalidValue;
  *resampler = nullptr;
  if (sampleType != GSDRX_RESAMPLER_F32 && sampleType != GSDRX_RESAMPLER_CF32) return hipErrorInvalidValue;
  if (interpolation == 0 || decimation == 0 || phase >= interpolation) return hipErrorInvalidValue;
  if (taps == nullptr || numTaps == 0) return hipErrorInvalidValue;
  gsdrxResampler r = new (std::nothrow) gsdrxResampler_t;
  if (r == nullptr) return hipErrorOutOfMemory;
  r->L = interpolation;
  r->M = decimation;
  r->phase0 = phase;
  r->taps = taps;
  r->T = numTaps;
  r->device = cudaDevice;
  r->sb = sampleType == GSDRX_RESAMPLER_CF32 ? 8 : 4;
  if (interpolation > 1) {  // (interpolation == 1 is gsdrFirFF / FC: the seam plan)
    gsdr::resample::Plan pl{};
    gsdr::resample::route_of(interpolation, decimation, numTaps, r->sb, &pl);
    r->tiled = pl.route == gsdr::resample::kRouteTile;
  }
  const hipError_t e = r->st.alloc(cudaDevice, gsdr::stream_hist_capacity(interpolation, numTaps) * r->sb,
                                   gsdr::stream_seam_capacity(interpolation, numTaps) * r->sb);
  if (e != hipSuccess) {
    (void)gsdrxResamplerDestroy(r);
    return e;
  }
  *resampler = r;
  return hipSuccess;
}

GSDR_C_LINKAGE size_t gsdrxResamplerOutputsFor(gsdrxResampler r, size_t numInputSamples) GSDR_NO_EXCEPT {
  gsdr::StreamPlan sp;
  if (r == nullptr) return 0;
  if (!gsdr::stream_plan(r->L, r->M, r->T, r->phase0, r->st.consumed, r->st.next_out, numInputSamples, &sp)) return 0;
  return (size_t)sp.outputs;
}

GSDR_C_LINKAGE hipError_t gsdrxResamplerProcess(gsdrxResampler r, const void* input, size_t numInputSamples,
                                                void* output, size_t outputCapacity, size_t* numOutputsWritten,
                                                hipStream_t cudaStream) GSDR_NO_EXCEPT {
  if (numOutputsWritten) *numOutputsWritten = 0;
  if (r == nullptr) return hipErrorInvalidValue;
  if (numInputSamples == 0) return hipSuccess;
  if (input == nullptr) return hipErrorInvalidValue;
  gsdr::StreamPlan sp;
  if (!gsdr::stream_plan(r->L, r->M, r->T, r->phase0, r->st.consumed, r->st.next_out, numInputSamples, &sp)) {
    return hipErrorInvalidValue;
  }
  if (sp.outputs > outputCapacity || (sp.outputs && output == nullptr)) return hipErrorInvalidValue;
  gsdr::DeviceScope scope(r->device);
  if (scope.status() != hipSuccess) return scope.status();
  const char* chunk = static_cast<const char*>(input);
  const hipError_t e =
      r->sb == 8 ? gsdr::resample::process<float2>(*r, sp, chunk, numInputSamples, static_cast<float2*>(output), cudaStream)
                 : gsdr::resample::process<float>(*r, sp, chunk, numInputSamples, static_cast<float*>(output), cudaStream);
  if (e != hipSuccess) return e;
  r->st.commit(sp, numInputSamples);
  if (numOutputsWritten) *numOutputsWritten = (size_t)sp.outputs;
  return hipSuccess;
}

GSDR_C_LINKAGE hipError_t gsdrxResamplerDestroy(gsdrxResampler r) GSDR_NO_EXCEPT {
  if (r == nullptr) return hipSuccess;
  const hipError_t e = r->st.release(r->device);
  delete r;
  return e;
}

GSDR_C_LINKAGE void gsdrxResamplerPlan(uint32_t interpolation, uint32_t decimation, uint64_t numTaps, uint32_t phase,
                                       uint64_t consumed, uint64_t nextOutput, uint64_t chunk,
                                       uint64_t plan[6]) GSDR_NO_EXCEPT {
  if (plan == nullptr) return;
  gsdr::StreamPlan sp;
  (void)gsdr::stream_plan(interpolation, decimation, numTaps, phase, consumed, nextOutput, chunk, &sp);
  plan[0] = sp.outputs;  // (all zero when refused)
  plan[1] = sp.seam;
  plan[2] = sp.hist;
  plan[3] = sp.skip;
  plan[4] = sp.hist_after;
  plan[5] = sp.skip_after;
}

GSDR_C_LINKAGE hipError_t gsdrxResampleFF(uint32_t interpolation, uint32_t decimation, uint32_t phase,
                                          const float* taps, size_t numTaps, const float* input, float* output,
                                          size_t numOutputs, int32_t cudaDevice,
                                          hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::resample::entry<float>(interpolation, decimation, phase, taps, numTaps, input, output, numOutputs,
                                      cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrxResampleFC(uint32_t interpolation, uint32_t decimation, uint32_t phase,
                                          const float* taps, size_t numTaps, const hipFloatComplex* input,
                                          hipFloatComplex* output, size_t numOutputs, int32_t cudaDevice,
                                          hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::resample::entry<float2>(interpolation, decimation, phase, taps, numTaps,
                                       reinterpret_cast<const float2*>(input), reinterpret_cast<float2*>(output),
                                       numOutputs, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE size_t gsdrxResampleInputsFor(uint32_t interpolation, uint32_t decimation, uint32_t phase,
                                             size_t numTaps, size_t numOutputs) GSDR_NO_EXCEPT {
  uint64_t extent = 0;
  if (numOutputs == 0 || interpolation == 0 || decimation == 0 || phase >= interpolation) return 0;
  if (!gsdr::resample::stuffed_extent(phase, decimation, numTaps, numOutputs, &extent)) return 0;
  return gsdr::resample::inputs_for(interpolation, extent);
}
