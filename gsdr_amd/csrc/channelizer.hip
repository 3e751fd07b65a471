// gsdr-mi355x: polyphase filter bank, M uniformly spaced channels of one input in one pass -- gsdrxChannelizer
// (include/gsdr/gsdr_ext.h). For output time m, with r0 = (firstSampleIndex + m D) mod M:
//     v[p]      = sum_k taps[p + k M] input[m D + p + k M],  p in [0, M)   (one ascending-k fmaf chain a component)
//     X[c]      = sum_p v[p] exp(-j 2 pi c p / M)                           (radix-2 DFT in registers)
//     output[c] = X[c] exp(-j 2 pi c r0 / M)                                (skipped when r0 == 0)
// Both kernels run the same three steps on the same registers, so the bits of an output depend on its window, the
// taps and r0 alone: not on the tile, nor on where a stream is cut into calls. The launch plan is
// channelizer_plan.hpp.
#include <hip/hip_runtime.h>

#include "channelizer_plan.hpp"
#include "fir_samples.hpp"
#include "gsdr/gsdr_ext.h"
#include "launch.hpp"

namespace gsdr {
namespace channelizer {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Params {
  const void* in;
  const float* taps;
  f32x2* out;    // channel c's row at out + c N
  uint64_t N;    // output times
  uint64_t T;
  uint64_t D;
  uint32_t r0;   // firstSampleIndex mod M
};

// exp(-j 2 pi k / 64), k in [0, 64): each component correctly rounded from its exact value, the first octant
// computed and the rest by symmetry, so entry k + 32 is minus entry k and the axes are exact. A bank of M channels
// uses every (64 / M)-th entry.
__device__ const f32x2 kTwiddle[64] = {
    {1.0f, 0.0f}, {0.99518472f, -0.0980171412f}, {0.980785251f, -0.195090324f}, {0.956940353f, -0.290284663f},
    {0.923879504f, -0.382683426f}, {0.881921291f, -0.471396744f}, {0.831469595f, -0.555570245f}, {0.773010433f, -0.634393275f},
    {0.707106769f, -0.707106769f}, {0.634393275f, -0.773010433f}, {0.555570245f, -0.831469595f}, {0.471396744f, -0.881921291f},
    {0.382683426f, -0.923879504f}, {0.290284663f, -0.956940353f}, {0.195090324f, -0.980785251f}, {0.0980171412f, -0.99518472f},
    {0.0f, -1.0f}, {-0.0980171412f, -0.99518472f}, {-0.195090324f, -0.980785251f}, {-0.290284663f, -0.956940353f},
    {-0.382683426f, -0.923879504f}, {-0.471396744f, -0.881921291f}, {-0.555570245f, -0.831469595f}, {-0.634393275f, -0.773010433f},
    {-0.707106769f, -0.707106769f}, {-0.773010433f, -0.634393275f}, {-0.831469595f, -0.555570245f}, {-0.881921291f, -0.471396744f},
    {-0.923879504f, -0.382683426f}, {-0.956940353f, -0.290284663f}, {-0.980785251f, -0.195090324f}, {-0.99518472f, -0.0980171412f},
    {-1.0f, 0.0f}, {-0.99518472f, 0.0980171412f}, {-0.980785251f, 0.195090324f}, {-0.956940353f, 0.290284663f},
    {-0.923879504f, 0.382683426f}, {-0.881921291f, 0.471396744f}, {-0.831469595f, 0.555570245f}, {-0.773010433f, 0.634393275f},
    {-0.707106769f, 0.707106769f}, {-0.634393275f, 0.773010433f}, {-0.555570245f, 0.831469595f}, {-0.471396744f, 0.881921291f},
    {-0.382683426f, 0.923879504f}, {-0.290284663f, 0.956940353f}, {-0.195090324f, 0.980785251f}, {-0.0980171412f, 0.99518472f},
    {0.0f, 1.0f}, {0.0980171412f, 0.99518472f}, {0.195090324f, 0.980785251f}, {0.290284663f, 0.956940353f},
    {0.382683426f, 0.923879504f}, {0.471396744f, 0.881921291f}, {0.555570245f, 0.831469595f}, {0.634393275f, 0.773010433f},
    {0.707106769f, 0.707106769f}, {0.773010433f, 0.634393275f}, {0.831469595f, 0.555570245f}, {0.881921291f, 0.471396744f},
    {0.923879504f, 0.382683426f}, {0.956940353f, 0.290284663f}, {0.980785251f, 0.195090324f}, {0.99518472f, 0.0980171412f},
};

// acc += t * x: one v_pk_fma_f32 with the tap in both halves, one rounding a component
__device__ __forceinline__ void mac(f32x2& acc, float t, f32x2 x) {
  acc = __builtin_elementwise_fma(f32x2{t, t}, x, acc);
}

// a * w, w a unit phasor: two roundings a component
__device__ __forceinline__ f32x2 cmul(f32x2 a, f32x2 w) {
  return f32x2{fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.x, w.y, a.y * w.x)};
}

__device__ __forceinline__ f32x2 sample_of(float2 s) { return f32x2{s.x, s.y}; }
__device__ __forceinline__ f32x2 sample_of(Iq8 s) { return f32x2{norm_i8(s.x), norm_i8(s.y)}; }

constexpr uint32_t bit_reverse(uint32_t i, uint32_t M) {
  uint32_t r = 0;
  for (uint32_t b = 1; b < M; b <<= 1, i >>= 1) r = (r << 1) | (i & 1);
  return r;
}

// Forward M-point DFT in place, decimation in frequency: X[c] is left in v[bit_reverse(c)]. Every index and every
// twiddle is a compile-time constant once the loops are unrolled, so v stays in registers; multiplications by 1
// and by -j are a copy and a swap.
template <uint32_t M>
__device__ __forceinline__ void dft(f32x2 (&v)[M]) {
#pragma unroll
  for (uint32_t half = M / 2; half >= 1; half /= 2) {
#pragma unroll
    for (uint32_t base = 0; base < M; base += 2 * half) {
#pragma unroll
      for (uint32_t j = 0; j < half; ++j) {
        const f32x2 a = v[base + j], b = v[base + j + half];
        const f32x2 d = a - b;
        v[base + j] = a + b;
        const uint32_t w = j * (32 / half);  // exp(-j 2 pi j / (2 half)) as an index into kTwiddle
        if (w == 0) {
          v[base + j + half] = d;
        } else if (w == 16) {
          v[base + j + half] = f32x2{d.y, -d.x};
        } else {
          v[base + j + half] = cmul(d, kTwiddle[w]);
        }
      }
    }
  }
}

// X[c] exp(-j 2 pi c r0 / M) to out[c N + m] for every c; the identity for r0 == 0.
template <uint32_t M>
__device__ __forceinline__ void rotate_and_store(f32x2 (&v)[M], uint32_t r0, f32x2* __restrict__ out, uint64_t N,
                                                 uint64_t m, bool store) {
  if (r0 != 0) {
#pragma unroll
    for (uint32_t c = 1; c < M; ++c) {
      const uint32_t at = bit_reverse(c, M);
      v[at] = cmul(v[at], kTwiddle[((c * r0) & (M - 1)) * (64 / M)]);
    }
  }
  if (store) {
#pragma unroll
    for (uint32_t c = 0; c < M; ++c) out[c * N + m] = v[bit_reverse(c, M)];
  }
}

// The 16 / sizeof(S) samples of one 16-byte granule of global memory to tile samples j, j + 1, ... of the padded LDS
// image (tile sample j at padded(j, D)), converted to float2.
template <uint32_t D, class S>
__device__ __forceinline__ void put_granule(f32x2* xs, uint32_t j, u32x4 q) {
  if constexpr (sizeof(S) == 8) {
    xs[padded(j, D)] = f32x2{__uint_as_float(q.x), __uint_as_float(q.y)};
    xs[padded(j + 1, D)] = f32x2{__uint_as_float(q.z), __uint_as_float(q.w)};
  } else {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      const float4 two = iq8x2_granule(w[e]);
      xs[padded(j + 2 * e, D)] = f32x2{two.x, two.y};
      xs[padded(j + 2 * e + 1, D)] = f32x2{two.z, two.w};
    }
  }
}

// 16-byte loads a thread has in flight while it stages: 8 of complex samples, 4 of int8 I/Q (four times the samples a
// load, and their conversion's registers)
template <class S>
constexpr uint32_t kStageDepth = sizeof(S) == 8 ? 8 : 4;

// src[0, count) to the padded LDS image xs: granules of 16 bytes of global memory wholly inside the range move with
// one load each, kStageDepth<S> of them issued before the first is written (a workgroup of one wave would otherwise
// pay the memory latency once a granule); the ragged head and tail go sample by sample. Nothing outside
// src[0, count) is read. The samples stream through once (non-temporal).
template <uint32_t D, class S>
__device__ __forceinline__ void stage(f32x2* xs, const S* __restrict__ src, uint32_t count, uint32_t tid,
                                      uint32_t wg) {
  constexpr uint32_t G = 16 / sizeof(S);
  const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(src) / sizeof(S)) % G;
  const uint32_t end = off + count;
  const u32x4* src16 = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(src) - off * sizeof(S));
  constexpr uint32_t kDepth = kStageDepth<S>;
  // whole granules [g0, g1); g0 G - off < G samples in front of them and fewer than G behind
  const uint32_t g0 = off != 0 ? 1u : 0u, g1 = end / G;
  for (uint32_t g = g0 + tid; g < g1; g += kDepth * wg) {
    u32x4 q[kDepth];
#pragma unroll
    for (uint32_t u = 0; u < kDepth; ++u) {
      if (g + u * wg < g1) q[u] = __builtin_nontemporal_load(src16 + g + u * wg);
    }
#pragma unroll
    for (uint32_t u = 0; u < kDepth; ++u) {
      if (g + u * wg < g1) put_granule<D, S>(xs, (g + u * wg) * G - off, q[u]);
    }
  }
  const uint32_t head = g0 * G < end ? g0 * G - off : count;       // samples before the first whole granule
  const uint32_t tail = g1 > g0 ? g1 * G - off : head;             // first sample behind the last whole granule
  if (tid < head) xs[padded(tid, D)] = sample_of(src[tid]);
  if (tail + tid < count) xs[padded(tail + tid, D)] = sample_of(src[tail + tid]);
}

// One workgroup a tile of KT = blockDim.x consecutive output times, D in {M, M / 2}: the tile's (kt - 1) D + T
// samples are staged into LDS, then thread `tid` owns output time tid of the tile. Lanes are consecutive m: the
// tap of a step is uniform across the wave (scalar loads), the samples are D apart in LDS, and each channel's row
// gets a contiguous 512-byte store a wave.
template <uint32_t M, uint32_t D, class S>
__global__ __launch_bounds__(kMaxWG) void k_channelizer_tile(const Params p) {
  extern __shared__ float4 lds16[];
  constexpr uint32_t kPitch = D + row_pad(D);  // LDS samples a row of D
  const uint32_t tid = threadIdx.x, KT = blockDim.x, T = (uint32_t)p.T;
  const uint64_t m0 = (uint64_t)blockIdx.x * KT;
  const uint32_t kt = p.N - m0 < KT ? (uint32_t)(p.N - m0) : KT;  // output times of this tile (>= 1)

  f32x2* xs = reinterpret_cast<f32x2*>(lds16);
  stage<D>(xs, static_cast<const S*>(p.in) + m0 * D, (kt - 1) * D + T, tid, KT);
  __syncthreads();

  // past a ragged tile: repeat its last output time (staged samples), store nothing
  const uint32_t ml = tid < kt ? tid : kt - 1;
  const f32x2* xp = xs + ml * kPitch;
  const float* __restrict__ tp = p.taps;
  f32x2 v[M];
#pragma unroll
  for (uint32_t q = 0; q < M; ++q) v[q] = f32x2{0.0f, 0.0f};
  // sample m D + k M + q is (M / D) k rows on, at q + (q / D) pad of its row: a compile-time offset
  for (uint32_t k = 0; k < T / M; ++k) {
#pragma unroll
    for (uint32_t q = 0; q < M; ++q) mac(v[q], tp[q], xp[padded(q, D)]);
    tp += M;
    xp += (M / D) * kPitch;
  }
  const uint32_t tail = T % M;
#pragma unroll
  for (uint32_t q = 0; q < M - 1; ++q) {
    if (q < tail) mac(v[q], tp[q], xp[padded(q, D)]);
  }

  dft<M>(v);
  const uint64_t m = m0 + ml;
  const uint32_t r0 = (uint32_t)((p.r0 + m * D) & (M - 1));
  rotate_and_store<M>(v, r0, p.out, p.N, m, tid < kt);
}

// One output time per thread straight from global memory, every index in 64 bits: every other decimation, and
// taps too long for a tile.
template <uint32_t M, class S>
__global__ __launch_bounds__(kGenericWG) void k_channelizer_generic(const Params p) {
  const uint64_t m = (uint64_t)blockIdx.x * kGenericWG + threadIdx.x;
  if (m >= p.N) return;
  const S* __restrict__ x = static_cast<const S*>(p.in) + m * p.D;
  const float* __restrict__ t = p.taps;
  f32x2 v[M];
#pragma unroll
  for (uint32_t q = 0; q < M; ++q) v[q] = f32x2{0.0f, 0.0f};
  const uint64_t full = p.T / M * M;
  for (uint64_t i = 0; i < full; i += M) {
#pragma unroll
    for (uint32_t q = 0; q < M; ++q) mac(v[q], t[i + q], sample_of(x[i + q]));
  }
  const uint32_t tail = (uint32_t)(p.T - full);
#pragma unroll
  for (uint32_t q = 0; q < M - 1; ++q) {
    if (q < tail) mac(v[q], t[full + q], sample_of(x[full + q]));
  }
  dft<M>(v);
  const uint32_t r0 = (uint32_t)((p.r0 + m * p.D) & (M - 1));
  rotate_and_store<M>(v, r0, p.out, p.N, m, true);
}

template <uint32_t M, class S>
static void launch(const Params& p, const Plan& pl, hipStream_t stream) {
  const dim3 grid((uint32_t)pl.blocks), block(pl.wg);
  if (pl.route == kRouteTile) {
    if (p.D == M) {
      k_channelizer_tile<M, M, S><<<grid, block, pl.lds_bytes, stream>>>(p);
    } else {
      k_channelizer_tile<M, M / 2, S><<<grid, block, pl.lds_bytes, stream>>>(p);
    }
  } else {
    k_channelizer_generic<M, S><<<grid, block, 0, stream>>>(p);
  }
}

template <class S>
static hipError_t launch_bank(uint32_t M, const Params& p, const Plan& pl, hipStream_t stream) {
  switch (M) {
    case 2: launch<2, S>(p, pl, stream); break;
    case 4: launch<4, S>(p, pl, stream); break;
    case 8: launch<8, S>(p, pl, stream); break;
    case 16: launch<16, S>(p, pl, stream); break;
    case 32: launch<32, S>(p, pl, stream); break;
    case 64: launch<64, S>(p, pl, stream); break;
    default: return hipErrorInvalidValue;
  }
  return launch_status();
}

}  // namespace channelizer
}  // namespace gsdr

GSDR_C_LINKAGE hipError_t gsdrxChannelizer(uint32_t numChannels, uint32_t decimation, size_t firstSampleIndex,
                                           const float* taps, size_t numTaps, int sampleFormat, const void* input,
                                           hipFloatComplex* output, size_t numOutputs, int32_t cudaDevice,
                                           hipStream_t cudaStream) GSDR_NO_EXCEPT {
  using namespace gsdr::channelizer;
  if (numOutputs == 0) return hipSuccess;
  if (!valid_channels(numChannels) || decimation == 0) return hipErrorInvalidValue;
  if (input == nullptr || output == nullptr || (numTaps > 0 && taps == nullptr)) return hipErrorInvalidValue;
  if (sampleFormat != GSDRX_SAMPLES_CF32 && sampleFormat != GSDRX_SAMPLES_CS8) return hipErrorInvalidValue;
  uint64_t need = 0;
  if (!extents(numChannels, decimation, numTaps, numOutputs, &need)) return hipErrorInvalidValue;
  Plan pl{};
  if (!plan(numChannels, decimation, numTaps, numOutputs, &pl)) return hipErrorInvalidValue;
  gsdr::DeviceScope scope(cudaDevice);
  if (scope.status() != hipSuccess) return scope.status();
  if (numTaps == 0) {  // no tap: every output is zero, as fir_entry
    const hipError_t st = hipMemsetAsync(output, 0, (size_t)numChannels * numOutputs * sizeof(hipFloatComplex), cudaStream);
    return st != hipSuccess ? st : gsdr::launch_status();
  }
  Params p{};
  p.in = input;
  p.taps = taps;
  p.out = reinterpret_cast<f32x2*>(output);
  p.N = numOutputs;
  p.T = numTaps;
  p.D = decimation;
  p.r0 = (uint32_t)((uint64_t)firstSampleIndex & (numChannels - 1));
  if (sampleFormat == GSDRX_SAMPLES_CS8) return launch_bank<gsdr::Iq8>(numChannels, p, pl, cudaStream);
  return launch_bank<float2>(numChannels, p, pl, cudaStream);
}
