// gsdr-mi355x: gsdrFirFC (reference src/fir.cu:73-171, include/gsdr/fir.h:30-68), its tuning variants
// and probes. FF / CC / CF and the int8 front end live in fir_ff.hip, fir_cc.hip, fir_cf.hip and
// fir_int8.hip (one sample-type pair per translation unit, built in parallel).
#include <hip/hip_runtime.h>

#include "fir_dispatch.hpp"
#include "fir_entry.hpp"
#include "gsdr/fir.h"
#include "gsdr/gsdr_ext.h"
#include "launch.hpp"

namespace gsdr {

#ifdef GSDR_TUNING_PROBES
// Tuning probes are not part of the product library: they are compiled only into
// build/probes/libgsdr_probes.so (`make probes`), which the tools/ scripts load through GSDR_LIB.

// Streaming ceiling probe for this traffic mix: reads the 8*N_in input bytes with fully coalesced
// 16-byte loads and writes 8*N_out bytes (outputs are a sum of loaded samples, not a FIR).
template <bool NT>
__global__ __launch_bounds__(256) void k_stream_probe(const float4* __restrict__ in, float4* __restrict__ out,
                                                      uint64_t n_in16, uint64_t n_out16) {
  // each thread: 4 input granules (one per 1 KiB wave-slab) -> 1 output granule
  const uint64_t wave = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t o = wave * 64u + lane;
  if (o >= n_out16) return;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t i = (wave * 4u + k) * 64u + lane;
    if (i < n_in16) {
      const float4 v = NT ? load16_nt(in + i) : in[i];
      a.x += v.x;
      a.y += v.y;
      a.z += v.z;
      a.w += v.w;
    }
  }
  out[o] = a;
}

hipError_t launch_stream_probe(const FirJob& j, hipStream_t s, bool nt) {
  const uint64_t n_in16 = j.L * 8 / 16, n_out16 = j.N * 8 / 16;
  const uint32_t blocks = (uint32_t)ceil_div<uint64_t>(n_out16, 256);
  const auto k = nt ? k_stream_probe<true> : k_stream_probe<false>;
  k<<<blocks, 256, 0, s>>>(reinterpret_cast<const float4*>(j.in), reinterpret_cast<float4*>(j.out), n_in16, n_out16);
  return launch_status();
}

// The headline shape (GSDR_FIR_ROWS row C4; real taps against complex samples) and the probes' launch of a tile on it.
using Headline = TileShape<4, 4, 16, 256>;
struct StreamedDma : TileStreamed {  // variant 14's options
  static constexpr bool DMA = true;
};
struct StreamedXcdOrder : TileStreamed {  // variant 9's options
  static constexpr bool XM = true;
};
template <int MODE, class Opts, class Shape = Headline>
hipError_t launch_probe(const FirJob& j, hipStream_t s) {
  return launch_poly_shape<float, float2, Shape, MODE, Opts>(j, s);
}

// Ablation probes (gsdrxFirFCVariant >= 100) used for the energy split in DESIGN.md section 3.1:
// the default shape with only one half of its work.
hipError_t launch_fc_probe(const FirJob& j, hipStream_t s) {
  // the FM chain (config 3's shape) on the same buffers, for the probes from 120 on
  FirJob c = j;
  c.mode = kModeFm;
  c.N = j.N - 1;  // an FM output needs one more FIR output than the input holds for N FIR outputs
  c.nco_inc = 429496730u;  // 0.1 fs
  c.fm_gain = 7.957747f;   // fs / (2 pi 0.02 fs)
  switch (j.variant) {
    case 104:  // compute only (no staging; the tile holds whatever LDS held)
      return launch_probe<kModeFir, Probed<TileStreamed, kProbeComputeOnly>>(j, s);
    case 105:  // staging only, plain loads
      return launch_probe<kModeFir, Probed<TileOpts<>, kProbeStageOnly>>(j, s);
    case 107:  // staging only, non-temporal loads
      return launch_probe<kModeFir, Probed<TileStreamed, kProbeStageOnly>>(j, s);
    case 113:  // matrix-core kernel with register taps, compute only
      return launch_mfma_bc_shape<kProbeComputeOnly>(j, s);
    case 117:  // staging only by LDS-DMA, non-temporal
      return launch_probe<kModeFir, Probed<StreamedDma, kProbeStageOnly>>(j, s);
    // FM chain split: 120 full FM kernel, 121 no NCO mix, 122 no discriminator (plain float store), 123 neither,
    // 124 staging + NCO + discriminator without the FIR, 125 staging only
    case 120: return launch_probe<kModeFm, TileStreamed>(c, s);
    case 121: return launch_probe<kModeFm, Probed<TileStreamed, kProbeNoMix>>(c, s);
    case 122: return launch_probe<kModeFm, Probed<TileStreamed, kProbeNoDisc>>(c, s);
    case 123: return launch_probe<kModeFm, Probed<TileStreamed, kProbeNoMix | kProbeNoDisc>>(c, s);
    case 124: return launch_probe<kModeFm, Probed<TileStreamed, kProbeStageOnly>>(c, s);
    case 125: return launch_probe<kModeFm, Probed<TileStreamed, kProbeStageOnly | kProbeNoMix | kProbeNoDisc>>(c, s);
    // FM chain tile-shape sweep: 130 default (R 4, JC 16, WG 256), 131 R 8 WG 128, 132 JC 8, 133 R 2, 134 WG 128,
    // 135 R 8 JC 8 WG 128, 136 default with the XCD-aware tile order
    case 130: return launch_probe<kModeFm, TileStreamed>(c, s);
    case 131: return launch_probe<kModeFm, TileStreamed, TileShape<4, 8, 16, 128>>(c, s);
    case 132: return launch_probe<kModeFm, TileStreamed, TileShape<4, 4, 8, 256>>(c, s);
    case 133: return launch_probe<kModeFm, TileStreamed, TileShape<4, 2, 16, 256>>(c, s);
    case 134: return launch_probe<kModeFm, TileStreamed, TileShape<4, 4, 16, 128>>(c, s);
    case 135: return launch_probe<kModeFm, TileStreamed, TileShape<4, 8, 8, 128>>(c, s);
    case 136: return launch_probe<kModeFm, StreamedXcdOrder>(c, s);
    case 110:
    case 111:
      return launch_stream_probe(j, s, j.variant == 111);
    default:
      return hipErrorInvalidValue;
  }
}
#else
hipError_t launch_fc_probe(const FirJob&, hipStream_t) { return hipErrorInvalidValue; }
#endif  // GSDR_TUNING_PROBES

// The streaming object's one-launch FIR step on complex float samples (stream.hip; stream_step_tiled).
hipError_t fir_fc_stream_step(size_t decimation, const float* taps, size_t tapCount, const StreamOperands& so,
                              hipFloatComplex* output, size_t numOutputs, int32_t device, hipStream_t stream) {
  return fir_stream_step_tiled<float2>(decimation, taps, tapCount, so, output, numOutputs, device, stream);
}

}  // namespace gsdr

using gsdr::fir_entry;

GSDR_C_LINKAGE hipError_t gsdrFirFC(size_t decimation, const float* taps, size_t tapCount,
                                    const hipFloatComplex* input, hipFloatComplex* output, size_t numOutputs,
                                    int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return fir_entry<float, float2>(decimation, taps, tapCount, input, output, numOutputs, cudaDevice, cudaStream, -1);
}

GSDR_C_LINKAGE hipError_t gsdrxFirFCVariant(int variant, size_t decimation, const float* taps, size_t tapCount,
                                            const hipFloatComplex* input, hipFloatComplex* output,
                                            size_t numOutputs, int32_t cudaDevice,
                                            hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return fir_entry<float, float2>(decimation, taps, tapCount, input, output, numOutputs, cudaDevice, cudaStream,
                                  variant);
}
