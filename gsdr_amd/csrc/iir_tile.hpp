// gsdr-mi355x: the pieces of an IIR chunk pass: the padded tile in LDS, its staging and its coalesced store, the
// inputs before a chunk, the recursion over one chunk and the transition over one chunk. Included by iir.hip inside
// namespace gsdr::iir, after its Acc / fma_s / coeff / x_at helpers. The single-pass k_iir_resident
// (iir_resident.hpp) is built from all of them. The multi-pass scan's k_iir_chunks (iir.hip) shares the layout,
// load_pre and chunk_transition_column and keeps its staging, recursion and store in its own body: reached through
// these functions the same operations were scheduled differently in all 48 instantiations, and gsdrIirCC at order 8
// and both order-16 calls measured 0.15 - 1 % slower. A change to the layout, the operation
// order of the recursion or the staging must be made in both places; tools/iir_bits.py compares both against an
// earlier build bit for bit. Arrays and plain values are passed, never a struct by reference.
#pragma once

// A workgroup of WG threads = WG / NC consecutive chunks = one tile of samples, staged through LDS so HBM sees
// coalesced loads / stores; lane t runs the recursion of component t % NC of chunk t / NC from the tile (chunk stride
// kChunk + 1 elements: consecutive lanes land on different banks). The scan's tiles have 128 threads (33 KB of LDS,
// real or complex), the single pass's 256.
template <class S, int WG_>
struct TileLayout {
  static constexpr int WG = WG_;
  static constexpr int NC = sizeof(S) / sizeof(float);  // components per sample: one lane each
  static constexpr int CPT = WG / NC;                     // chunks per tile
  static constexpr int TS = CPT * kChunk;                 // samples per tile
  static constexpr int STRIDE = kChunk + 1;               // LDS row stride (in S units; floats of one component)
  static constexpr size_t kBytes = sizeof(float) * WG * STRIDE;
  static constexpr int SPV = 16 / sizeof(S);   // samples per 16-byte load
  static constexpr int NV = TS / SPV / WG;     // 16-byte loads per thread for a whole tile
  __device__ static int at(int idx) { return idx + idx / kChunk; }  // sample idx -> padded slot (in S units)
};

// A whole tile's 16-byte loads into registers. Staging them (stage_tile) is a separate call: the callers issue their
// other loads in between, and all of them are in flight together.
template <class L, class S>
__device__ __forceinline__ void load_tile(const S* __restrict__ x, uint64_t base, int t, float4 (&r)[L::NV]) {
  const float4* __restrict__ src = reinterpret_cast<const float4*>(x + base);
#pragma unroll
  for (int k = 0; k < L::NV; ++k) r[k] = src[k * L::WG + t];
}

// The tile into its padded rows: the registers of load_tile (whole), or tlen samples one at a time (a ragged tile,
// or buffers that allow no 16-byte access); ZFILL zero-fills the rows past tlen (the single pass scans every chunk).
template <class L, bool ZFILL, class S>
__device__ __forceinline__ void stage_tile(S* tile, bool whole, const float4 (&v)[L::NV], const S* __restrict__ x,
                                           uint64_t base, uint32_t tlen, int t) {
  if (whole) {
#pragma unroll
    for (int k = 0; k < L::NV; ++k) {
      const int idx = (k * L::WG + t) * L::SPV;  // SPV consecutive samples, all in one chunk row
      float* d = reinterpret_cast<float*>(tile + L::at(idx));
      d[0] = v[k].x;
      d[1] = v[k].y;
      d[2] = v[k].z;
      d[3] = v[k].w;
    }
  } else {
    for (int idx = t; idx < (ZFILL ? L::TS : (int)tlen); idx += L::WG)
      tile[L::at(idx)] = (!ZFILL || idx < (int)tlen) ? x[base + idx] : zero_s(S{});
  }
}

// The tile out of its rows, coalesced: 16-byte stores for a whole tile, else tlen samples one at a time.
template <class L, class S>
__device__ __forceinline__ void store_tile(const S* tile, bool whole, S* y, uint64_t base, uint32_t tlen, int t) {
  if (whole) {
    float4* __restrict__ dst = reinterpret_cast<float4*>(y + base);
#pragma unroll
    for (int k = 0; k < L::NV; ++k) {
      const int idx = (k * L::WG + t) * L::SPV;
      const float* d = reinterpret_cast<const float*>(tile + L::at(idx));
      dst[k * L::WG + t] = make_float4(d[0], d[1], d[2], d[3]);
    }
  } else {
    for (int idx = t; idx < (int)tlen; idx += L::WG) y[base + idx] = tile[L::at(idx)];
  }
}

// Thread t < P: x[base - 1 - t], one of the P samples before the tile (the input history for the first tile), loaded
// beside the tile and stored to pre[t] with it.
template <int P, class S>
__device__ __forceinline__ S load_pre(const S* __restrict__ x, const S* __restrict__ xh, int K, uint64_t base, int t) {
  S pv = zero_s(S{});
  if (t < P) pv = x_at(x, xh, K, (int64_t)base - 1 - t);
  return pv;
}

// xd[i] = component comp of x[n0 - 1 - i] for chunk lc of the tile, from the tile or from pre: read for every chunk
// before any row is overwritten with y
template <class L, int P, class S>
__device__ __forceinline__ void prev_inputs(const S* tile, const S* pre, int lc, int comp, double (&xd)[P]) {
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int m = lc * kChunk - 1 - i;  // tile index of x[n0-1-i]; < 0: before the tile
    xd[i] = (double)reinterpret_cast<const float*>(m >= 0 ? tile + L::at(m) : pre + (-1 - m))[comp];
  }
}

// The recursion over one chunk of len samples in `row` (one component, NC floats apart) from the previous inputs xd
// and outputs ys, newest first; both end as the state after the chunk. WRITE: y replaces x in the row, rounded to
// float. Inputs are held as doubles (converted once per sample, exact); a whole chunk is fully unrolled so the state
// shifts are register renames. The feedback terms are added oldest first, so only the last FMA (a[1] y[n-1]) waits
// for the previous step's output: one FMA latency per sample on the recursion's critical path instead of P (the
// chunk passes are latency-bound). `row` is not __restrict__: other lanes and the coalesced
// store read the rows through the tile, and restrict would let the compiler move those accesses across the stores.
template <int P, int NC, bool WRITE>
__device__ __forceinline__ void run_chunk(float* row, uint32_t len, const double (&b)[P + 1], const double (&am)[P + 1],
                                          double (&xd)[P], double (&ys)[P]) {
  auto step = [&](uint32_t k) {
    const double xv = (double)row[k * NC];
    double acc = b[0] * xv;
#pragma unroll
    for (int i = 1; i <= P; ++i) acc = fma(b[i], xd[i - 1], acc);
#pragma unroll
    for (int i = P; i >= 1; --i) acc = fma(am[i], ys[i - 1], acc);
#pragma unroll
    for (int i = P - 1; i > 0; --i) {
      xd[i] = xd[i - 1];
      ys[i] = ys[i - 1];
    }
    xd[0] = xv;
    ys[0] = acc;
    if constexpr (WRITE) row[k * NC] = (float)acc;
  };
  if (len == (uint32_t)kChunk) {
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kChunk; ++k) step(k);
  } else {
    for (int k = 0; k < (int)len; ++k) step(k);
  }
}

// Column t of M_0, the transition over one chunk: the state after kChunk steps of the homogeneous recursion
// y[n] = -sum a[i] y[n-i] from e_t; with STEPS, output k of those steps goes to gk[k * P + t]. The scan's setup tables
// (iir_setup), the fused tails pass's powers (build_pow) and the single pass's tables (k_res_setup) all grow from this
// one function, so they hold the same doubles.
template <int P, bool STEPS = false>
__device__ __forceinline__ void chunk_transition_column(const Coeffs& cf, int t, double (&m)[P], double* gk = nullptr) {
  double am[P + 1];
#pragma unroll
  for (int i = 0; i <= P; ++i) am[i] = -coeff(cf.a, cf.K, i);
#pragma unroll
  for (int i = 0; i < P; ++i) m[i] = i == t ? 1.0 : 0.0;
  for (int k = 0; k < kChunk; ++k) {
    double acc = 0.0;
#pragma unroll
    for (int i = 1; i <= P; ++i) acc = fma(am[i], m[i - 1], acc);
#pragma unroll
    for (int i = P - 1; i > 0; --i) m[i] = m[i - 1];
    m[0] = acc;
    if constexpr (STEPS) gk[k * P + t] = acc;
  }
}
