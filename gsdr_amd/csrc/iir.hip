// gsdr-mi355x: IIR filter as a true recursive filter (include/gsdr/iir.h; SURVEY.md section 8(f)
// row 4). Replaces reference src/iir.cu, whose kernel restarts every thread's 8-sample chunk from
// zero state (iir.cu:121-127) and ignores the history arguments (iir.cu:213-214).
//
//   y[n] = sum_{i<=P} b[i] x[n-i] - sum_{1<=i<=P} a[i] y[n-i],   P = K - 1
//
// Parallel scan over the linear recursion (state s = (y[n-1], ..., y[n-P])):
//   1. k_iir_chunks<kTails>: the signal is cut into 32-sample chunks (a workgroup stages WG chunks
//      through LDS for coalesced HBM access); each thread filters its chunk from zero output state
//      (the FIR part sees the true previous inputs) and stores the chunk's zero-state tail T_c.
//   2. The true state entering chunk c obeys S_{c+1} = M S_c + T_c, M = the P x P transition over a
//      chunk of the homogeneous recursion (k_iir_setup, with its powers M^(G^k)). That affine
//      recurrence is scanned hierarchically in groups of 64 elements, one wave per group and one
//      element per lane: up-sweep = Hillis-Steele scan within the wave (6 steps with M^(2^s)),
//      whose last lane is the group aggregate for the next level; down-sweep = every element's start
//      state M^r S_group + prefix_(r-1) at once (table of M^r, r < 64, per level).
//   3. k_iir_chunks<kFinal>: each chunk re-runs from its true start state and writes y.
//   4. The last chunk of that pass writes the last P inputs / outputs into the caller's history buffers.
// For P <= 8 level 0's up-sweep runs inside the tails pass and its down-sweep in the final pass; up to
// 2^25 samples the levels above 1 and level 1's down-sweep take one launch (k_iir_scan_upper), so 2^24
// samples run as tails, level-1 up-sweep, upper scan, final: 4 launches.
// State, scan and matrices are double (see Acc below); complex samples with real coefficients are
// two independent recursions sharing M. State dimensions are padded to a compiled P (zero
// coefficients beyond K-1 leave the recursion unchanged).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "gsdr/iir.h"
#include "iir_plan.hpp"
#include "launch.hpp"

namespace gsdr {
namespace iir {

// The recursion state, the scan and the transition matrices are kept in double: the direct form
// amplifies an inconsistent perturbation of its P-sample state by 10^2..10^3 (tests/test_gpu_iir.py),
// and rounding a scanned state to float32 at every chunk boundary is exactly such a perturbation.
// Samples stay float32 in HBM and LDS; only the outputs are rounded.
template <class S>
struct Acc;
template <>
struct Acc<float> {
  using type = double;
};
template <>
struct Acc<float2> {
  using type = double2;
};
template <class S>
using AccT = typename Acc<S>::type;

__device__ __forceinline__ float zero_s(float) { return 0.0f; }
__device__ __forceinline__ float2 zero_s(float2) { return make_float2(0.0f, 0.0f); }
__device__ __forceinline__ double zero_s(double) { return 0.0; }
__device__ __forceinline__ double2 zero_s(double2) { return make_double2(0.0, 0.0); }
__device__ __forceinline__ double fma_s(double c, double x, double acc) { return fma(c, x, acc); }
__device__ __forceinline__ double2 fma_s(double c, double2 x, double2 acc) {
  return make_double2(fma(c, x.x, acc.x), fma(c, x.y, acc.y));
}
__device__ __forceinline__ double fma_s(double c, float x, double acc) { return fma(c, (double)x, acc); }
__device__ __forceinline__ double2 fma_s(double c, float2 x, double2 acc) {
  return make_double2(fma(c, (double)x.x, acc.x), fma(c, (double)x.y, acc.y));
}
__device__ __forceinline__ double to_acc(float v) { return (double)v; }
__device__ __forceinline__ double2 to_acc(float2 v) { return make_double2(v.x, v.y); }
__device__ __forceinline__ double add_s(double a, double b) { return a + b; }
__device__ __forceinline__ double shfl_up_s(double v, int d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ double2 shfl_up_s(double2 v, int d) {
  return make_double2(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64));
}
__device__ __forceinline__ double2 add_s(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double shfl_xor_s(double v, int d) { return __shfl_xor(v, d, 64); }
__device__ __forceinline__ double2 shfl_xor_s(double2 v, int d) {
  return make_double2(__shfl_xor(v.x, d, 64), __shfl_xor(v.y, d, 64));
}

struct Coeffs {
  const float* b;
  const float* a;
  int K;
};

// coefficient i of a zero-padded array (uniform: the compiler turns these into scalar loads)
// every load unconditional (clamped index, K >= 1), so the coefficient loads issue together instead of one
// round trip each behind a branch
__device__ __forceinline__ double coeff(const float* c, int K, int i) {
  const float v = c[i < K ? i : K - 1];
  return i < K ? (double)v : 0.0;
}

// x[n] for n >= -P: the input, or the caller's input history (K-1 entries) for n < 0, else zero
template <class S>
__device__ __forceinline__ S x_at(const S* __restrict__ x, const S* __restrict__ xh, int K, int64_t n) {
  if (n >= 0) return x[n];
  return (xh && -1 - n < K - 1) ? xh[-1 - n] : zero_s(S{});
}

// workgroup barrier for LDS-only phases: waits for this wave's LDS accesses, not its global loads
// (__syncthreads would also drain the tile loads in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// matrix product C = A * B (P x P, row-major) by a workgroup: each thread computes entries
template <int P>
__device__ __forceinline__ void mat_mul(const double* __restrict__ A, const double* __restrict__ B,
                                        double* __restrict__ C, int t, int nt) {
  for (int e = t; e < P * P; e += nt) {
    const int i = e / P, j = e % P;
    double acc = 0.0;
#pragma unroll
    for (int l = 0; l < P; ++l) acc = fma(A[i * P + l], B[l * P + j], acc);
    C[e] = acc;
  }
}

// acc += M x (M: P x P, row-major; double, or double2 = two recursions sharing M): per row i from acc[i], then
// l = 0 .. P-1. Every scan step and every start state below is this one order of operations. mat_row_acc is one
// row of it, for down_group, which stores each row as it is formed.
template <class V, int P>
__device__ __forceinline__ V mat_row_acc(const double* __restrict__ Mi, const V (&x)[P], V a) {
#pragma unroll
  for (int l = 0; l < P; ++l) a = fma_s(Mi[l], x[l], a);
  return a;
}
template <class V, int P>
__device__ __forceinline__ void mat_vec_acc(const double* __restrict__ M, const V (&x)[P], V (&acc)[P]) {
#pragma unroll
  for (int i = 0; i < P; ++i) acc[i] = mat_row_acc<V, P>(M + i * P, x, acc[i]);
}

// Hillis-Steele scan of one group over the affine composition from zero state, one element per lane:
// v_r <- v_r + M^(2^s) v_(r-2^s), s < 6, ending with the zero-state prefix through element r. M^(2^s) is pw[2^s] of
// a level's table T[r] = M^r (kTablePow) or pw[s] of powers stored one after another (kPackedPow). The steps run on
// a copy of the caller's array: in place through the reference, k_iir_up<double, 16> took 134 VGPRs, not 70.
constexpr bool kTablePow = false, kPackedPow = true;
template <class V, int P, bool PACKED>
__device__ __forceinline__ void wave_scan(V (&io)[P], int r, const double* __restrict__ pw) {
  V v[P];
#pragma unroll
  for (int i = 0; i < P; ++i) v[i] = io[i];
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int d = 1 << s;
    V w[P];
#pragma unroll
    for (int i = 0; i < P; ++i) w[i] = shfl_up_s(v[i], d);
    if (r >= d) mat_vec_acc<V, P>(pw + (size_t)(PACKED ? s : d) * P * P, w, v);
  }
#pragma unroll
  for (int i = 0; i < P; ++i) io[i] = v[i];
}

#include "iir_tile.hpp"  // the chunk pass's pieces, shared with the single-pass kernel (iir_resident.hpp)

// One workgroup prepares the scan's constants:
//   s0        = entry state (double) from the caller's output history, zero-padded to P;
//   T[k][r]   = M_k^r for r in [0, 64), with M_0 the transition over one chunk (column j = state after
//               kChunk steps of y[n] = -sum a[i] y[n-i] from e_j) and M_{k+1} = M_k^64,
// for every level k = 0..levels. Each level's table is built by doubling in `work` (LDS when it fits,
// else the global table itself): T[h] = T[h/2]^2, then T[h + q] = T[h] T[q].
// barrier for the setup workgroup; the device-scope fence is needed only when the table lives in
// global memory (it costs ~1 us, and the doubling rounds need ~50 barriers)
template <bool INLDS>
__device__ __forceinline__ void sync_table() {
  if constexpr (!INLDS) __threadfence();
  __syncthreads();
}

// INLDS (compile time): `work` is the caller's LDS table. Inlined with a compile-time choice, the table
// accesses compile to ds_read / ds_write; a runtime select between LDS and global made every one of
// them a flat access.
template <class S, int P, int NT, bool INLDS>
__device__ __forceinline__ void iir_setup(const Coeffs& cf, const S* __restrict__ yh,
                                          typename Acc<S>::type* __restrict__ s0, double* __restrict__ T, int levels,
                                          double* __restrict__ work) {
  const int t = threadIdx.x;
  const int Pk = cf.K - 1;
  constexpr int PP = P * P;
  if (t < P) s0[t] = (yh && t < Pk) ? to_acc(yh[t]) : zero_s(typename Acc<S>::type{});
  for (int lv = 0; lv <= levels; ++lv) {
    double* __restrict__ W = INLDS ? work : T + (size_t)lv * kGroup * PP;
    if (lv == 0) {
      if (t < P) {
        double m[P];
        chunk_transition_column<P>(cf, t, m);
#pragma unroll
        for (int i = 0; i < P; ++i) W[PP + i * P + t] = m[i];
      }
    } else {  // M_lv = M_{lv-1}^64 = (M_{lv-1}^32)^2, from the previous level's table
      const double* Tp = INLDS ? work : T + (size_t)(lv - 1) * kGroup * PP;
      double m2[(PP + NT - 1) / NT];
      int c = 0;
      for (int e = t; e < PP; e += NT, ++c) {
        const int i = e / P, j = e % P;
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < P; ++l) acc = fma(Tp[32 * PP + i * P + l], Tp[32 * PP + l * P + j], acc);
        m2[c] = acc;
      }
      sync_table<INLDS>();
      c = 0;
      for (int e = t; e < PP; e += NT, ++c) W[PP + e] = m2[c];
    }
    for (int e = t; e < PP; e += NT) W[e] = (e / P == e % P) ? 1.0 : 0.0;
    sync_table<INLDS>();
    for (int h = 2; h < kGroup; h *= 2) {
      mat_mul<P>(W + (h / 2) * PP, W + (h / 2) * PP, W + h * PP, t, NT);
      sync_table<INLDS>();
      for (int w = t; w < (h - 1) * PP; w += NT) {
        const int q = 1 + w / PP, e = w % PP;
        if (h + q < kGroup) {
          const int i = e / P, j = e % P;
          double acc = 0.0;
#pragma unroll
          for (int l = 0; l < P; ++l) acc = fma(W[h * PP + i * P + l], W[q * PP + l * P + j], acc);
          W[(h + q) * PP + e] = acc;
        }
      }
      sync_table<INLDS>();
    }
    if constexpr (INLDS) {  // publish the level's table
      double* Tl = T + (size_t)lv * kGroup * PP;
      for (int e = t; e < kGroup * PP; e += NT) Tl[e] = W[e];
      __syncthreads();
    }
  }
}

// the scan's chunk-pass tile (iir_tile.hpp): 128 threads
template <class S>
using ScanTile = TileLayout<S, 128>;
static_assert(ScanTile<float>::TS * sizeof(float) == kTileSampleBytes, "the plan counts these tiles");
static_assert(ScanTile<float2>::TS * sizeof(float2) == kTileSampleBytes, "the plan counts these tiles");

enum ChunkPass : int { kTails = 0, kFinal = 1 };

// What each pass of k_iir_chunks reads besides the input, by pass and by whether level 0 of the scan is fused
// into the chunk passes. Scan states are AccT<S>, P per element.
template <class S, int PASS, bool FUSED>
struct PassArgs;
template <class S>
struct SetupArgs {  // the setup workgroup of the tails pass (iir_setup)
  const S* yh;
  AccT<S>* s0;
  double* T;
  int levels;
  const S* xh;  // the caller's input history, copied to xh_copy for the final pass
  S* xh_copy;
};
template <class S>
struct PassArgs<S, kTails, false> {
  SetupArgs<S> setup;
  AccT<S>* tails;  // every chunk's zero-state tail (the level-0 elements)
};
template <class S>
struct PassArgs<S, kTails, true> {
  SetupArgs<S> setup;
  AccT<S>* incl;  // level-0 inclusive zero-state prefixes, written by the pass's own up-sweep
  AccT<S>* aggs;  // level-1 elements (group aggregates), or null when level 0 is the top
};
// final pass: its last chunk writes the caller's history buffers (Pk = K - 1 entries); the pass reads the input
// history from the tails pass's copy, so no tile reads what the last one overwrites
template <class S>
struct PassArgs<S, kFinal, false> {
  S* y;
  const AccT<S>* starts;  // every chunk's start state
  float *xh_out, *yh_out;
  int Pk;
};
template <class S>
struct PassArgs<S, kFinal, true> {
  S* y;
  const AccT<S>* incl;    // level-0 inclusive prefixes (from the tails pass)
  const double* T0;       // M_0^r, r < 64
  const AccT<S>* gstart;  // level-1 start states, or null: s0 is the group start
  const AccT<S>* s0;
  float *xh_out, *yh_out;
  int Pk;
};

template <int P>
constexpr bool kTableInLds = kGroup * P * P * sizeof(double) <= 32 * 1024;

// Level-0 scan fused into the chunk passes (P <= kFusedMaxP): the tails pass runs the up-sweep of its
// own groups from LDS (no tails round trip through HBM, no separate launch) and the final pass
// derives each chunk's start state itself (the level-0 down-sweep). P > kFusedMaxP (K > 9) runs the unfused
// passes: level 0 as launches of its own (k_iir_up / k_iir_down, or k_iir_scan_rest), tails and start states
// through HBM.
constexpr int kFusedMaxP = 8;

// Up-sweep of group g of one level (one wave, lane r = element j = g*64 + r, read from mine[0 .. P): the level's
// elements in global memory, or the workgroup's tails in LDS for the fused level 0). Lane r's result, the zero-state
// prefix through element r, is kept in `incl` for the down-sweep; the last lane's is the next level's element g.
template <class A, int P, bool PACKED>
__device__ __forceinline__ void up_group(const A* __restrict__ mine, uint64_t E, const double* __restrict__ pw,
                                         A* __restrict__ incl, A* __restrict__ aggs, uint64_t g, int r) {
  const uint64_t j = g * kGroup + r;
  const uint64_t last = (E - 1 < g * kGroup + kGroup - 1) ? E - 1 - g * kGroup : kGroup - 1;
  A v[P];
#pragma unroll
  for (int i = 0; i < P; ++i) v[i] = j < E ? mine[i] : zero_s(A{});
  wave_scan<A, P, PACKED>(v, r, pw);
  if (j < E) {
#pragma unroll
    for (int i = 0; i < P; ++i) incl[j * P + i] = v[i];
  }
  if (aggs && (uint64_t)r == last) {
#pragma unroll
    for (int i = 0; i < P; ++i) aggs[g * P + i] = v[i];
  }
}

// One chunk pass of the scan. Its staging, previous inputs, recursion and store are the operations of iir_tile.hpp's
// stage_tile / prev_inputs / run_chunk / store_tile, written out here: through those functions the compiler scheduled
// every instantiation differently and three of eight timed calls got slower (iir_tile.hpp).
template <class S, int P, int PASS, bool VEC, bool FUSED = false>
__global__ __launch_bounds__(ScanTile<S>::WG) void k_iir_chunks(Coeffs cf, const S* __restrict__ x,
                                                                 const S* __restrict__ xh, uint64_t n,
                                                                 PassArgs<S, PASS, FUSED> pa) {
  using TSh = ScanTile<S>;
  using A = typename Acc<S>::type;
  constexpr size_t kTileBytes = TSh::kBytes;
  constexpr size_t kTableBytes = kTableInLds<P> ? kGroup * P * P * sizeof(double) : 0;
  __shared__ __attribute__((aligned(16))) char smem[kTileBytes > kTableBytes ? kTileBytes : kTableBytes];
  // fused tails pass: M_0^(2^s), s < 6, and the workgroup's chunk tails
  constexpr int kPow = (FUSED && PASS == kTails) ? 6 * P * P : 1;
  static_assert(!FUSED || TSh::CPT * P * sizeof(A) <= kTileBytes, "tails alias the tile");
  __shared__ double mpow[kPow];
  __shared__ S pre[P];  // x[base - 1 - i], i < P
  S* tile = reinterpret_cast<S*>(smem);
  A* tl = reinterpret_cast<A*>(smem);  // fused tails pass: the chunk tails, once the tile is consumed
  const int t = threadIdx.x;
  // 1. Setup workgroup
  if constexpr (PASS == kTails) {
    // the extra FIRST workgroup builds the scan constants while the others compute the tails (as the
    // last one it was dispatched after most tiles and finished after them: ~7 us at the kernel's end)
    if (blockIdx.x == 0) {
      const SetupArgs<S>& su = pa.setup;
      if (su.xh != nullptr && t < cf.K - 1) su.xh_copy[t] = su.xh[t];
      iir_setup<S, P, TSh::WG, kTableInLds<P>>(cf, su.yh, su.s0, su.T, su.levels, reinterpret_cast<double*>(smem));
      return;
    }
  }
  // Workgroup b filters tile b (a register prefetch of the next tile in a persistent grid measured no
  // faster). Barriers wait for LDS only (lds_barrier), so global loads issued before them stay in flight.
  const uint64_t ntiles = (n + TSh::TS - 1) / TSh::TS;
  constexpr int SPV = 16 / sizeof(S);          // samples per 16-byte load
  constexpr int NV = TSh::TS / SPV / TSh::WG;   // 16-byte loads per thread for a whole tile
  constexpr int NC = TSh::NC;
  const int comp = t % NC;
  auto is_whole = [&](uint64_t i) { return VEC && (i + 1) * (uint64_t)TSh::TS <= n; };
  auto load_tile = [&](uint64_t i, float4 (&r)[NV]) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(x + i * TSh::TS);
#pragma unroll
    for (int k = 0; k < NV; ++k) r[k] = src[k * TSh::WG + t];
  };
  uint64_t ti = PASS == kTails ? blockIdx.x - 1 : blockIdx.x;
  const uint64_t first_ti = ti;
  auto build_pow = [&]() {
    // M_0 (chunk_transition_column, as iir_setup's T[1]), then squared five times: the same products as
    // iir_setup's T[2], T[4], ..., T[32], so the same doubles
    if (t < P) {
      double m[P];
      chunk_transition_column<P>(cf, t, m);
#pragma unroll
      for (int i = 0; i < P; ++i) mpow[i * P + t] = m[i];
    }
    lds_barrier();
    for (int q = 1; q < 6; ++q) {
      mat_mul<P>(mpow + (q - 1) * P * P, mpow + (q - 1) * P * P, mpow + q * P * P, t, TSh::WG);
      lds_barrier();
    }
  };
  double b[P + 1], am[P + 1];
#pragma unroll
  for (int i = 0; i <= P; ++i) {
    b[i] = coeff(cf.b, cf.K, i);
    am[i] = -coeff(cf.a, cf.K, i);
  }
  // One tile per workgroup (the launcher starts ntiles workgroups): written as a loop that ends after its
  // first pass, so nothing is live across iterations. With `ti += nwg` the compiler kept the coefficients
  // and the fused scan's state live around the loop: 148 VGPRs, 3 waves per SIMD, instead of 66 / 112.
  for (; ti < ntiles; ti = ntiles) {
    const uint64_t base = ti * TSh::TS;
    const uint32_t tlen = n - base < (uint64_t)TSh::TS ? (uint32_t)(n - base) : (uint32_t)TSh::TS;
    const bool whole = is_whole(ti);
    const uint64_t c = ti * TSh::CPT + t / NC;
    const uint64_t n0 = c * kChunk;
    double ys[P];  // component of y[n-1-i]: the chunk's start state
#pragma unroll
    for (int i = 0; i < P; ++i) ys[i] = 0.0;
    // 2. Start-state operands
    // Final pass: the operands of the chunk's start state are loaded BEFORE the tile. Vector loads retire
    // in order, so operands loaded after the tile could only be used once the whole tile had arrived: the
    // start state's FMAs would then sit on the critical path instead of under the tile's load latency.
    constexpr bool kPro = FUSED && PASS == kFinal;
    constexpr int PP = P * P;
    double mr[kPro ? PP : 1], inc[kPro ? P : 1], sgc[kPro ? P : 1];
    const uint64_t g = c / kGroup;
    const int r = (int)(c % kGroup);
    if constexpr (kPro) {
      // level-0 down-sweep for this chunk: start = M_0^r S_g + prefix_(r-1) (as down_group)
      if (n0 < n) {
        const double* __restrict__ Mr = pa.T0 + (size_t)r * PP;
#pragma unroll
        for (int e = 0; e < PP; ++e) mr[e] = Mr[e];
        const double* __restrict__ incl_d = reinterpret_cast<const double*>(pa.incl);
#pragma unroll
        for (int i = 0; i < P; ++i) inc[i] = r > 0 ? incl_d[((c - 1) * P + i) * NC + comp] : 0.0;
        const double* __restrict__ sg = reinterpret_cast<const double*>(pa.gstart ? pa.gstart + g * P : pa.s0);
#pragma unroll
        for (int l = 0; l < P; ++l) sgc[l] = sg[l * NC + comp];
      }
    }
    // 3. Tile loads
    float4 v[NV];
    if (whole) load_tile(ti, v);  // in flight while the final pass computes the chunk start state

    // the P samples before the tile (the input history for the first tile), loaded beside it
    const S pv = load_pre<P>(x, xh, cf.K, base, t);
    // 4. Start state
    if constexpr (kPro) {
      if (n0 < n) {
#pragma unroll
        for (int i = 0; i < P; ++i) ys[i] = inc[i];
        mat_vec_acc<double, P>(mr, sgc, ys);
      }
    } else if constexpr (PASS == kFinal && !FUSED) {
      if (n0 < n) {
        const double* __restrict__ starts_d = reinterpret_cast<const double*>(pa.starts);
#pragma unroll
        for (int i = 0; i < P; ++i) ys[i] = starts_d[(c * P + i) * NC + comp];
      }
    }
    // 5. Stage
    if (whole) {
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int idx = (k * TSh::WG + t) * SPV;  // SPV consecutive samples, all in one chunk row
        float* d = reinterpret_cast<float*>(tile + TSh::at(idx));
        d[0] = v[k].x;
        d[1] = v[k].y;
        d[2] = v[k].z;
        d[3] = v[k].w;
      }
    } else {
      for (int idx = t; idx < (int)tlen; idx += TSh::WG) tile[TSh::at(idx)] = x[base + idx];
    }
    if (t < P) pre[t] = pv;
    lds_barrier();
    // 6. Previous inputs
    // component of x[n-1-i] for every chunk, read before any row is overwritten with y
    double xd[P];
    {
      const int lc = t / NC;  // chunk within the tile
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int m = lc * kChunk - 1 - i;  // tile index of x[n0-1-i]; < 0: before the tile
        xd[i] = (double)reinterpret_cast<const float*>(m >= 0 ? tile + TSh::at(m) : pre + (-1 - m))[comp];
      }
    }
    if constexpr (PASS == kFinal) lds_barrier();
    // 7. Recursion
    // lane t runs the recursion of component t % NC of chunk t / NC (complex samples with real
    // coefficients are two independent real recursions): scalar double state, twice the lanes
    if (n0 < n) {
      const uint32_t len = n - n0 < (uint64_t)kChunk ? (uint32_t)(n - n0) : (uint32_t)kChunk;
      float* __restrict__ row = reinterpret_cast<float*>(tile + (t / NC) * TSh::STRIDE) + comp;
      // inputs held as doubles (converted once per sample, exact); a whole chunk is fully unrolled
      // so the state shifts are register renames
      // The feedback terms are added oldest first, so only the last FMA (a[1] y[n-1]) waits for the
      // previous step's output: one FMA latency per sample on the recursion's critical path instead of
      // P (the chunk passes are latency-bound).
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
        if constexpr (PASS == kFinal) row[k * NC] = (float)acc;  // y replaces x in this chunk's row
      };
      if (len == (uint32_t)kChunk) {
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kChunk; ++k) step(k);
      } else {
        for (uint32_t k = 0; k < len; ++k) step(k);
      }
      // 8. Tails (unfused: to HBM), or the history after the final pass's last chunk
      if constexpr (PASS == kTails && !FUSED) {
        double* __restrict__ tails_d = reinterpret_cast<double*>(pa.tails);
#pragma unroll
        for (int i = 0; i < P; ++i) tails_d[(c * P + i) * NC + comp] = ys[i];
      } else if constexpr (PASS == kFinal) {
        if (n0 + len == n) {
          // the last chunk's state after the call (outputs, then inputs, newest first) into the caller's
          // history buffers (component comp of entry i)
#pragma unroll
          for (int i = 0; i < P; ++i) {
            if (i < pa.Pk) {
              if (pa.yh_out) pa.yh_out[i * NC + comp] = (float)ys[i];
              if (pa.xh_out) pa.xh_out[i * NC + comp] = (float)xd[i];
            }
          }
        }
      }
    }
    // 8, fused: the tails into LDS and the up-sweep of the workgroup's own level-0 groups
    if constexpr (PASS == kTails && FUSED) {
      if (ti == first_ti) build_pow();
      lds_barrier();  // every lane is done reading the tile
      if (n0 < n) {
#pragma unroll
        for (int i = 0; i < P; ++i) reinterpret_cast<double*>(&tl[(t / NC) * P + i])[comp] = ys[i];
      }
      lds_barrier();
      const int w = t / kGroup;
      if (w < TSh::CPT / kGroup) {
        const uint64_t C = (n + kChunk - 1) / kChunk;
        const uint64_t g = ti * (TSh::CPT / kGroup) + w;
        const int lane = t % kGroup;
        up_group<A, P, kPackedPow>(tl + (w * kGroup + lane) * P, C, mpow, pa.incl, pa.aggs, g, lane);
      }
    }
    // 9. Store
    if constexpr (PASS == kFinal) {
      lds_barrier();
      S* __restrict__ y = pa.y;
      if (whole) {
        float4* __restrict__ dst = reinterpret_cast<float4*>(y + base);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int idx = (k * TSh::WG + t) * SPV;
          const float* d = reinterpret_cast<const float*>(tile + TSh::at(idx));
          dst[k * TSh::WG + t] = make_float4(d[0], d[1], d[2], d[3]);
        }
      } else {
        for (int idx = t; idx < (int)tlen; idx += TSh::WG) y[base + idx] = tile[TSh::at(idx)];
      }
    }
    lds_barrier();  // the tile's LDS is free for the next one
  }
}

// Down-sweep of group g: element j = g*64 + r starts in state M^r S_g + prefix_(r-1), with S_g the
// group's start state (group_starts[g], or s0 at the top level) and prefix the up-sweep's inclusive
// zero-state prefix of the previous lane. Overwrites incl with the start states.
template <class A, int P>
__device__ __forceinline__ void down_group(uint64_t E, const double* __restrict__ T, const A* __restrict__ group_starts,
                                           const A* __restrict__ s0, A* __restrict__ incl_starts, uint64_t g, int r) {
  constexpr int PP = P * P;
  const uint64_t j = g * kGroup + r;
  A pre[P], sg[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const A mine = j < E ? incl_starts[j * P + i] : zero_s(A{});
    pre[i] = shfl_up_s(mine, 1);
    sg[i] = group_starts ? group_starts[g * P + i] : s0[i];
  }
  if (j < E) {
    const double* __restrict__ Mr = T + (size_t)r * PP;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      incl_starts[j * P + i] = mat_row_acc<A, P>(Mr + i * P, sg, r > 0 ? pre[i] : zero_s(A{}));
    }
  }
}

// level 0 (many groups): one wave per group
template <class A, int P>
__global__ __launch_bounds__(64) void k_iir_up(const A* __restrict__ elems, uint64_t E, const double* __restrict__ T,
                                               A* __restrict__ incl, A* __restrict__ aggs) {
  up_group<A, P, kTablePow>(elems + ((uint64_t)blockIdx.x * kGroup + threadIdx.x) * P, E, T, incl, aggs, blockIdx.x,
                           threadIdx.x);
}

template <class A, int P>
__global__ __launch_bounds__(64) void k_iir_down(uint64_t E, const double* __restrict__ T,
                                                 const A* __restrict__ group_starts, A* __restrict__ incl_starts) {
  down_group<A, P>(E, T, group_starts, nullptr, incl_starts, blockIdx.x, threadIdx.x);
}

// The upper levels with at most kRestGroups groups run in ONE single-workgroup launch, up-sweeps then
// down-sweeps (one wave per group, a barrier between levels, workgroup-scope visibility); larger levels
// get one launch each. A single workgroup is latency-bound walking many groups: 128 groups per level
// took 5x longer than a launch per level, and even with each wave scanning 4-8 groups at once (their
// loads issued together) the whole of levels 1..3 for 2^24 samples took 72 us on one CU against ~19 us
// for the per-level launches. Up and down in one launch: 8.9 us instead of 6.2 + 4.9 us.
constexpr int kRestWaves = 16;
// a call's planned workspace, typed: level k's elements, their start states and its table T[r] = M_k^r
template <class A>
struct Workspace {
  char* ws;
  ScanPlan pl;
  __host__ __device__ A* elems(int k) const { return reinterpret_cast<A*>(ws + pl.elems[k]); }
  __host__ __device__ A* starts(int k) const { return reinterpret_cast<A*>(ws + pl.starts[k]); }
  __host__ __device__ double* table(int k) const {
    return reinterpret_cast<double*>(ws + pl.tables + k * pl.table_bytes);
  }
};

template <class A, int P>
__global__ __launch_bounds__(64 * kRestWaves) void k_iir_scan_rest(Workspace<A> W, const A* __restrict__ s0, int from) {
  const int w = threadIdx.x / 64, r = threadIdx.x % 64;
  for (int k = from; k <= W.pl.levels; ++k) {
    const uint64_t groups = ceil_div<uint64_t>(W.pl.E[k], kGroup);
    for (uint64_t g = w; g < groups; g += kRestWaves) {
      up_group<A, P, kTablePow>(W.elems(k) + (g * kGroup + r) * P, W.pl.E[k], W.table(k), W.starts(k),
                                k < W.pl.levels ? W.elems(k + 1) : nullptr, g, r);
    }
    __syncthreads();
  }
  for (int k = W.pl.levels; k >= from; --k) {
    const uint64_t groups = ceil_div<uint64_t>(W.pl.E[k], kGroup);
    for (uint64_t g = w; g < groups; g += kRestWaves) {
      down_group<A, P>(W.pl.E[k], W.table(k), k < W.pl.levels ? W.starts(k + 1) : nullptr, s0, W.starts(k), g, r);
    }
    __syncthreads();
  }
}

// Levels >= 2 up and down plus level 1's down-sweep in ONE launch (E2 <= kUpperE2 level-2 elements:
// 2^25 samples), after level 1's up-sweep (k_iir_up). Every workgroup scans all of level 2 itself (at most 4
// groups of 64, one wave each, in registers and LDS: a few KB from L2) and derives the level-2 start states
// its own level-1 groups need; then wave j down-sweeps level-1 group 4 b + j of its workgroup b. The
// redundant upper scan costs nothing next to what it replaces: the single-workgroup upper-level kernel
// walked levels 2..3 through global memory (one dependent round trip per phase, 8.3 us at 2^24 samples) and
// a separate level-1 down-sweep (or its fold into the final pass's prologue).
constexpr int kUpperWaves = 4;
static_assert(kUpperE2 == kUpperWaves * kGroup, "one wave per level-2 group");

// T[k] = M_k^r, r < 64 (setup tables); elems1 = level-1 elements (their inclusive prefixes in starts1 from
// k_iir_up, overwritten with start states), elems2 = level-2 elements (group aggregates of level 1)
template <int P>
__global__ __launch_bounds__(64 * kUpperWaves) void k_iir_scan_upper(uint64_t E1, uint64_t E2, int NC,
                                                                     const double* __restrict__ T1,
                                                                     const double* __restrict__ T2,
                                                                     const double* __restrict__ T3,
                                                                     const double* __restrict__ elems2,
                                                                     const double* __restrict__ s0,
                                                                     double* __restrict__ starts1) {
  constexpr int PP = P * P;
  __shared__ double incl2[kUpperE2][P];      // level-2 zero-state inclusive prefixes within their group
  __shared__ double gstart[kUpperWaves][P];  // level-2 group start states
  const int comp = blockIdx.y;
  const int t = threadIdx.x, r = t % 64, w = t / 64;
  // this wave's level-1 group (= level-2 element) and its own operands, loaded first
  const uint64_t e2 = (uint64_t)blockIdx.x * kUpperWaves + w;
  const uint64_t e1 = e2 * kGroup + r;
  const bool live = e2 < E2 && e1 < E1;
  double mine[P], m1r[PP];
#pragma unroll
  for (int i = 0; i < P; ++i) mine[i] = live ? starts1[(e1 * P + i) * NC + comp] : 0.0;
#pragma unroll
  for (int q = 0; q < PP; ++q) m1r[q] = T1[(size_t)r * PP + q];
  // 1. level 2: every workgroup scans all E2 elements, wave j the group j (one element a lane)
  double v[P];
  const uint64_t j2 = (uint64_t)t;
#pragma unroll
  for (int i = 0; i < P; ++i) v[i] = j2 < E2 ? elems2[(j2 * P + i) * NC + comp] : 0.0;
  wave_scan<double, P, kTablePow>(v, r, T2);
#pragma unroll
  for (int i = 0; i < P; ++i) incl2[t][i] = v[i];
  __syncthreads();
  // 2. the level-2 groups' start states: at most 4, composed in order from s0 (M_3 = M_2^64)
  if (t < P) {
    double sg[P];
#pragma unroll
    for (int i = 0; i < P; ++i) sg[i] = s0[i * NC + comp];
    const int ng = (int)((E2 + kGroup - 1) / kGroup);
    for (int q = 0; q < kUpperWaves; ++q) {
      gstart[q][t] = sg[t];
      if (q + 1 < ng) {
        double nv[P];
#pragma unroll
        for (int i = 0; i < P; ++i) nv[i] = incl2[q * kGroup + kGroup - 1][i];
        mat_vec_acc<double, P>(T3 + PP, sg, nv);
#pragma unroll
        for (int i = 0; i < P; ++i) sg[i] = nv[i];
      }
    }
  }
  __syncthreads();
  if (!(e2 < E2)) return;
  // 3. this wave's level-2 element start: M_2^r2 S_group + incl2[e2 - 1] (uniform across the wave)
  const int r2 = (int)(e2 % kGroup);
  const int q2 = (int)(e2 / kGroup);
  double s2[P], sg[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    s2[i] = r2 > 0 ? incl2[e2 - 1][i] : 0.0;
    sg[i] = gstart[q2][i];
  }
  mat_vec_acc<double, P>(T2 + (size_t)r2 * PP, sg, s2);
  // 4. level-1 down-sweep of group e2: element e1 starts in M_1^r S2 + incl1[e1 - 1]
  double st[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const double prev = __shfl_up(mine[i], 1, 64);
    st[i] = r > 0 ? prev : 0.0;
  }
  mat_vec_acc<double, P>(m1r, s2, st);
  if (live) {
#pragma unroll
    for (int i = 0; i < P; ++i) starts1[(e1 * P + i) * NC + comp] = st[i];
  }
}

// one chunk pass: 16-byte tile loads / stores when the caller's buffers allow them (vec)
template <class S, int P, int PASS, bool FUSED>
static void launch_chunks(uint32_t blocks, hipStream_t st, bool vec, const Coeffs& cf, const S* x, const S* xh,
                          uint64_t n, const PassArgs<S, PASS, FUSED>& pa) {
  const auto kernel = vec ? k_iir_chunks<S, P, PASS, true, FUSED> : k_iir_chunks<S, P, PASS, false, FUSED>;
  kernel<<<blocks, ScanTile<S>::WG, 0, st>>>(cf, x, xh, n, pa);
}

// the multi-pass scan of one call, state size P
template <class S, int P>
static hipError_t run(const Coeffs& cf, S* xh, S* yh, const S* x, S* y, uint64_t n, hipStream_t st) {
  using A = typename Acc<S>::type;
  constexpr bool F = P <= kFusedMaxP;
  Workspace<A> W{};
  const ScanPlan& pl = W.pl;
  if (!scan_plan(n, P, sizeof(A), sizeof(S), F, &W.pl)) return hipErrorInvalidValue;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&W.ws), pl.bytes, st);
  if (e != hipSuccess) return e;
  auto groups = [&](int k) { return (uint32_t)ceil_div<uint64_t>(pl.E[k], kGroup); };
  A* s0 = reinterpret_cast<A*>(W.ws + pl.s0);
  S* xh_copy = reinterpret_cast<S*>(W.ws + pl.xh_copy);
  const uint32_t blocks = (uint32_t)pl.ntiles;  // one workgroup per tile (k_iir_chunks)
  const bool vec = aligned16(x) && aligned16(y);
  // tails pass (plus the setup workgroup); fused, it leaves level 0's inclusive prefixes and group aggregates
  PassArgs<S, kTails, F> ta{};
  ta.setup.yh = yh;
  ta.setup.s0 = s0;
  ta.setup.T = W.table(0);
  ta.setup.levels = pl.levels;
  ta.setup.xh = xh;
  ta.setup.xh_copy = xh_copy;
  if constexpr (F) {
    ta.incl = W.starts(0);
    ta.aggs = pl.levels > 0 ? W.elems(1) : nullptr;
  } else {
    ta.tails = W.elems(0);
  }
  launch_chunks<S, P, kTails, F>(blocks + 1, st, vec, cf, x, xh, n, ta);
  // up-sweeps of the large levels, then k_iir_scan_upper, or k_iir_scan_rest and the large levels' down-sweeps
  for (int k = pl.lowest; k < (pl.upper ? 2 : pl.rest); ++k)
    k_iir_up<A, P><<<groups(k), 64, 0, st>>>(W.elems(k), pl.E[k], W.table(k), W.starts(k), W.elems(k + 1));
  if constexpr (F) {
    if (pl.upper) {
      const dim3 grid((uint32_t)ceil_div<uint64_t>(pl.E[2], kUpperWaves), ScanTile<S>::NC);
      k_iir_scan_upper<P><<<grid, 64 * kUpperWaves, 0, st>>>(
          pl.E[1], pl.E[2], ScanTile<S>::NC, W.table(1), W.table(2), pl.levels >= 3 ? W.table(3) : nullptr,
          reinterpret_cast<const double*>(W.elems(2)), reinterpret_cast<const double*>(s0),
          reinterpret_cast<double*>(W.starts(1)));
    }
  }
  if (!pl.upper) {
    if (pl.rest <= pl.levels) k_iir_scan_rest<A, P><<<1, 64 * kRestWaves, 0, st>>>(W, s0, pl.rest);
    for (int k = pl.rest - 1; k >= pl.lowest; --k)
      k_iir_down<A, P><<<groups(k), 64, 0, st>>>(pl.E[k], W.table(k), W.starts(k + 1), W.starts(k));
  }
  // final pass; fused, it finishes level 0 itself. Its last chunk writes the caller's history (no launch for that)
  PassArgs<S, kFinal, F> fa{};
  fa.y = y;
  if constexpr (F) {
    fa.incl = W.starts(0);
    fa.T0 = W.table(0);
    fa.gstart = pl.levels > 0 ? W.starts(1) : nullptr;
    fa.s0 = s0;
  } else {
    fa.starts = W.starts(0);
  }
  fa.xh_out = reinterpret_cast<float*>(xh);
  fa.yh_out = reinterpret_cast<float*>(yh);
  fa.Pk = cf.K - 1;  // live state components (<= P); the rest stay zero
  launch_chunks<S, P, kFinal, F>(blocks, st, vec, cf, x, xh ? xh_copy : nullptr, n, fa);
  e = launch_status();
  const hipError_t f = hipFreeAsync(W.ws, st);
  return e != hipSuccess ? e : f;
}

// f(std::integral_constant<int, P>) for the compiled state size P that holds the filter's K - 1
template <class F>
static hipError_t dispatch_state_size(size_t Pk, F&& f) {
  if (Pk <= 1) return f(std::integral_constant<int, 1>{});
  if (Pk <= 2) return f(std::integral_constant<int, 2>{});
  if (Pk <= 4) return f(std::integral_constant<int, 4>{});
  if (Pk <= 8) return f(std::integral_constant<int, 8>{});
  if (Pk <= 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 31>{});
}

template <class S>
static hipError_t entry(const float* b, const float* a, size_t K, S* xh, S* yh, const S* x, S* y, size_t n,
                        int32_t device, hipStream_t st) {
  if (K < 2 || K > 32) return hipErrorInvalidValue;  // reference limits (iir.cu:229-235)
  if (n == 0) return hipSuccess;
  if (b == nullptr || a == nullptr || x == nullptr || y == nullptr) return hipErrorInvalidValue;
  static_assert(kChunk >= 31, "a chunk must hold the largest state");
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  const Coeffs cf{b, a, (int)K};
  return dispatch_state_size(K - 1, [&](auto p) { return run<S, decltype(p)::value>(cf, xh, yh, x, y, n, st); });
}

}  // namespace iir
}  // namespace gsdr

GSDR_C_LINKAGE hipError_t gsdrIirFF(const float* bCoeffs, const float* aCoeffs, size_t coeffCount, float* inputHistory,
                                    float* outputHistory, const float* input, float* output, size_t numElements,
                                    int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::iir::entry<float>(bCoeffs, aCoeffs, coeffCount, inputHistory, outputHistory, input, output,
                                 numElements, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrIirCC(const float* bCoeffs, const float* aCoeffs, size_t coeffCount,
                                    hipFloatComplex* inputHistory, hipFloatComplex* outputHistory,
                                    const hipFloatComplex* input, hipFloatComplex* output, size_t numElements,
                                    int32_t cudaDevice, hipStream_t cudaStream) GSDR_NO_EXCEPT {
  return gsdr::iir::entry<float2>(bCoeffs, aCoeffs, coeffCount, reinterpret_cast<float2*>(inputHistory),
                                  reinterpret_cast<float2*>(outputHistory), reinterpret_cast<const float2*>(input),
                                  reinterpret_cast<float2*>(output), numElements, cudaDevice, cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrIirFFCustom(const float* bCoeffs, const float* aCoeffs, size_t coeffCount,
                                          float* inputHistory, float* outputHistory, const float* input, float* output,
                                          size_t numElements, size_t samplesPerThread, int32_t cudaDevice,
                                          hipStream_t cudaStream) GSDR_NO_EXCEPT {
  if (samplesPerThread == 0 || samplesPerThread > 32) return hipErrorInvalidValue;  // iir.cu (Custom) limits
  return gsdrIirFF(bCoeffs, aCoeffs, coeffCount, inputHistory, outputHistory, input, output, numElements, cudaDevice,
                   cudaStream);
}

GSDR_C_LINKAGE hipError_t gsdrIirCCCustom(const float* bCoeffs, const float* aCoeffs, size_t coeffCount,
                                          hipFloatComplex* inputHistory, hipFloatComplex* outputHistory,
                                          const hipFloatComplex* input, hipFloatComplex* output, size_t numElements,
                                          size_t samplesPerThread, int32_t cudaDevice,
                                          hipStream_t cudaStream) GSDR_NO_EXCEPT {
  if (samplesPerThread == 0 || samplesPerThread > 32) return hipErrorInvalidValue;
  return gsdrIirCC(bCoeffs, aCoeffs, coeffCount, inputHistory, outputHistory, input, output, numElements, cudaDevice,
                   cudaStream);
}

#ifdef GSDR_TUNING_PROBES
// Tuning-probe build only (libgsdr_probes.so; tools/ and tests/test_gpu_iir.py bind them by name): the single-pass
// kernel of iir_resident.hpp beside the scan above, which stays the product's only path.
namespace gsdr {
namespace iir {
#include "iir_resident.hpp"

// bit 0: a single-pass tile gave up waiting since the last gsdrxIirSinglePassStatus (per device)
__device__ uint32_t g_res_status;

template <class S, int P>
static hipError_t run_resident(const Coeffs& cf, S* xh, S* yh, const S* x, S* y, uint64_t n, hipStream_t st,
                               uint32_t max_polls) {
  constexpr int NC = res::Tile<S>::NC;
  const uint64_t ntiles = ceil_div<uint64_t>(n, res::Tile<S>::TS);
  const uint64_t nsb = ceil_div<uint64_t>(ntiles, res::kResSB);
  // one block: the tile aggregates, the superblock aggregates (both filled with kResEmpty by the setup
  // kernel), the tables and coefficients
  const uint64_t nagg = (ntiles + nsb) * P * NC;
  const size_t off_tabs = nagg * sizeof(double);
  const size_t off_ticket = off_tabs + (res::res_tab_doubles<P>() + res::res_coef_doubles<P>()) * sizeof(double);
  const size_t bytes = off_ticket + 16;
  void* status = nullptr;
  hipError_t se = hipGetSymbolAddress(&status, HIP_SYMBOL(g_res_status));
  if (se != hipSuccess) return se;
  char* ws = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&ws), bytes, st);
  if (e != hipSuccess) return e;
  res::ResArgs ra{};
  ra.loc = reinterpret_cast<double*>(ws);
  ra.sbagg = ra.loc + ntiles * P * NC;
  double* tabs = reinterpret_cast<double*>(ws + off_tabs);
  ra.tabs = tabs;
  ra.xh_out = reinterpret_cast<float*>(xh);
  ra.yh_out = reinterpret_cast<float*>(yh);
  ra.Pk = cf.K - 1;
  ra.ticket = reinterpret_cast<uint32_t*>(ws + off_ticket);
  ra.status = static_cast<uint32_t*>(status);
  ra.max_polls = max_polls;
  const uint32_t nclear = (uint32_t)std::min<uint64_t>(512, ceil_div<uint64_t>(nagg, 8 * res::kResWG));
  res::k_res_setup<S, P><<<1 + nclear, res::kResWG, 0, st>>>(cf, tabs, reinterpret_cast<uint64_t*>(ws), nagg, ra.ticket);
  const auto k = aligned16(x) && aligned16(y) ? res::k_iir_resident<S, P, true> : res::k_iir_resident<S, P, false>;
  k<<<(uint32_t)ntiles, res::kResWG, 0, st>>>(cf, x, xh, yh, n, y, ra);
  e = launch_status();
  const hipError_t f = hipFreeAsync(ws, st);
  return e != hipSuccess ? e : f;
}

// entry()'s checks in entry()'s order, then the single-pass kernel: K <= 9 and up to 2^16 tiles (2^29 real / 2^28
// complex samples); anything else is refused, not rerouted
template <class S>
static hipError_t entry_single_pass(const float* b, const float* a, size_t K, S* xh, S* yh, const S* x, S* y, size_t n,
                                    uint32_t max_polls, int32_t device, hipStream_t st) {
  if (K < 2 || K > 32) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (b == nullptr || a == nullptr || x == nullptr || y == nullptr) return hipErrorInvalidValue;
  DeviceScope scope(device);
  if (scope.status() != hipSuccess) return scope.status();
  const Coeffs cf{b, a, (int)K};
  return dispatch_state_size(K - 1, [&](auto p) {
    constexpr int P = decltype(p)::value;
    if constexpr (P <= res::kResMaxP) {
      if (ceil_div<uint64_t>(n, res::Tile<S>::TS) <= res::kResMaxTiles)
        return run_resident<S, P>(cf, xh, yh, x, y, n, st, max_polls);
    }
    return hipErrorNotSupported;
  });
}

}  // namespace iir
}  // namespace gsdr

// gsdrIirFF / gsdrIirCC on the single-pass kernel, chosen per call. maxPolls bounds every wait in polling rounds
// (2^22 is the measured setting; 0 makes every tile that has to wait give up at once, which is how the status
// path is tested); hipErrorNotSupported for K > 9 or more than 2^16 tiles. A give-up is reported by
// gsdrxIirSinglePassStatus, which synchronises the stream and returns hipErrorLaunchFailure (clearing the word)
// when any tile gave up since the last query.
#define GSDR_PROBE_API extern "C" __attribute__((visibility("default")))
GSDR_PROBE_API hipError_t gsdrxIirFFSinglePass(const float* bCoeffs, const float* aCoeffs, size_t coeffCount,
                                               float* inputHistory, float* outputHistory, const float* input,
                                               float* output, size_t numElements, uint32_t maxPolls,
                                               int32_t cudaDevice, hipStream_t cudaStream) noexcept {
  return gsdr::iir::entry_single_pass<float>(bCoeffs, aCoeffs, coeffCount, inputHistory, outputHistory, input, output,
                                             numElements, maxPolls, cudaDevice, cudaStream);
}

GSDR_PROBE_API hipError_t gsdrxIirCCSinglePass(const float* bCoeffs, const float* aCoeffs, size_t coeffCount,
                                               hipFloatComplex* inputHistory, hipFloatComplex* outputHistory,
                                               const hipFloatComplex* input, hipFloatComplex* output,
                                               size_t numElements, uint32_t maxPolls, int32_t cudaDevice,
                                               hipStream_t cudaStream) noexcept {
  return gsdr::iir::entry_single_pass<float2>(
      bCoeffs, aCoeffs, coeffCount, reinterpret_cast<float2*>(inputHistory), reinterpret_cast<float2*>(outputHistory),
      reinterpret_cast<const float2*>(input), reinterpret_cast<float2*>(output), numElements, maxPolls, cudaDevice,
      cudaStream);
}

// hipSuccess when no single-pass tile gave up since the last query, else hipErrorLaunchFailure
GSDR_PROBE_API hipError_t gsdrxIirSinglePassStatus(int32_t cudaDevice, hipStream_t cudaStream) noexcept {
  gsdr::DeviceScope scope(cudaDevice);
  if (scope.status() != hipSuccess) return scope.status();
  uint32_t v = 0;
  hipError_t e = hipMemcpyFromSymbolAsync(&v, HIP_SYMBOL(gsdr::iir::g_res_status), sizeof(v), 0,
                                          hipMemcpyDeviceToHost, cudaStream);
  if (e == hipSuccess) e = hipStreamSynchronize(cudaStream);
  if (e != hipSuccess) return e;
  if (v == 0) return hipSuccess;
  const uint32_t z = 0;
  e = hipMemcpyToSymbolAsync(HIP_SYMBOL(gsdr::iir::g_res_status), &z, sizeof(z), 0, hipMemcpyHostToDevice,
                             cudaStream);
  if (e == hipSuccess) e = hipStreamSynchronize(cudaStream);
  return e != hipSuccess ? e : hipErrorLaunchFailure;
}
#endif  // GSDR_TUNING_PROBES
