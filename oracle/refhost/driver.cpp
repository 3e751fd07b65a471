/*
 * Reference-run driver -- TEST INFRASTRUCTURE ONLY (oracle/README.md, "Reference-run libraries").
 *
 * Compiles the reference's own kernel text, cut at build time into oracle/_ref/extract/*.inc by build_ref.py, as
 * host functions (shim.h) and exports one plain C function per kernel. Each runs the kernel the way the
 * reference's wrappers launch it: ceil(n / 32) blocks of 32 threads (its SIMPLE_CUDA_FNC_START), thread after
 * thread. Built twice, with -ffp-contract=fast -mfma (nvcc contracts a * b + c by default) and with
 * -ffp-contract=off; libm stands in for NVIDIA's device math library.
 *
 * Complex arrays are interleaved float pairs. This file holds no reference text: it names the kernels and
 * restates only what the wrappers do on the host (the D == 1 dispatch of fir.cu, the phase step of trig.cu,
 * the table copy of qpsk256.cu).
 */
#include "shim.h"

#include <string.h>

#include <vector>

#include "cuComplexOperatorOverloads.cuh" /* the reference's operators, from its src/ on the include path */

/* the constellation tables k_Qpsk256Modulate* read (__constant__ arrays in the reference, filled by its init wrapper) */
static cuComplex c_qpsk256_rectangular[256];
static cuComplex c_qpsk256_circular[256];

#include "extract/add_const.inc"
#include "extract/conversion.inc"
#include "extract/fir.inc"
#include "extract/magnitude.inc"
#include "extract/multiply.inc"
#include "extract/qpsk.inc"
#include "extract/qpsk256.inc"
#include "extract/quad_demod.inc"
#include "extract/trig.inc"

#define LAUNCH(n, call)                                          \
  do {                                                           \
    blockDim = dim3(32);                                         \
    const size_t blocks_ = ((size_t)(n) + 31) / 32;              \
    for (size_t b_ = 0; b_ < blocks_; ++b_) {                    \
      blockIdx.x = (unsigned)b_;                                 \
      for (unsigned t_ = 0; t_ < 32; ++t_) {                     \
        threadIdx.x = t_;                                        \
        call;                                                    \
      }                                                          \
    }                                                            \
  } while (0)

/* Several element-wise kernels test `x > n`, so thread n reads in[n] and writes out[n] whenever n is no multiple
 * of 32: run them on zero-extended copies of n + 1 elements and keep the first n outputs. */
template <class T>
static std::vector<T> extended(const T* p, size_t n) {
  std::vector<T> v(n + 1);
  if (n) memcpy(v.data(), p, n * sizeof(T));
  return v;
}

template <class T>
static void keep(T* dst, const std::vector<T>& v, size_t n) {
  if (n) memcpy(dst, v.data(), n * sizeof(T));
}

typedef cuComplex C;

extern "C" {

/* tt: 0 FF, 1 FC, 2 CC, 3 CF (taps, input). decimation 1 runs k_Fir, anything else k_FirDecimate (fir.cu wrappers). */
void ref_fir(int tt, uint32_t D, const void* taps, uint32_t T, const void* x, void* y, uint32_t N) {
#define FIR(IN_T, OUT_T, TAP_T)                                                                              \
  if (D == 1)                                                                                                \
    LAUNCH(N, (k_Fir<IN_T, OUT_T, TAP_T>((const IN_T*)x, (const TAP_T*)taps, T, (OUT_T*)y, N)));             \
  else                                                                                                       \
    LAUNCH(N, (k_FirDecimate<IN_T, OUT_T, TAP_T>((const IN_T*)x, (const TAP_T*)taps, T, D, (OUT_T*)y, N)))
  switch (tt) {
    case 0: FIR(float, float, float); break;
    case 1: FIR(C, C, float); break;
    case 2: FIR(C, C, C); break;
    case 3: FIR(float, C, C); break;
  }
#undef FIR
}

void ref_quad_fm(const C* x, float* out, float gain, uint32_t n) { LAUNCH(n, k_quadFmDemod(x, out, gain, n)); }
void ref_quad_am(const C* x, float* out, uint32_t n) { LAUNCH(n, k_quadAmDemod(x, out, n)); }

void ref_magnitude(const C* x, float* out, size_t n) {
  std::vector<C> a = extended(x, n);
  std::vector<float> b(n + 1);
  LAUNCH(n, k_Magnitude(a.data(), b.data(), n));
  keep(out, b, n);
}

void ref_abs(const float* x, float* out, size_t n) {
  std::vector<float> a = extended(x, n), b(n + 1);
  LAUNCH(n, k_Abs(a.data(), b.data(), n));
  keep(out, b, n);
}

/* variant: 0 FF, 1 CC, 2 CF (complex input, real constant), 3 FC (real input, complex constant) */
void ref_add_const(int variant, const void* x, float cr, float ci, void* out, size_t n) {
  const C cc = make_cuComplex(cr, ci);
  if (variant == 0) {
    std::vector<float> a = extended((const float*)x, n), b(n + 1);
    LAUNCH(n, (k_AddConst<float, float, float>(a.data(), cr, b.data(), n)));
    keep((float*)out, b, n);
  } else if (variant == 3) {
    std::vector<float> a = extended((const float*)x, n);
    std::vector<C> b(n + 1);
    LAUNCH(n, (k_AddConst<float, C, C>(a.data(), cc, b.data(), n)));
    keep((C*)out, b, n);
  } else {
    std::vector<C> a = extended((const C*)x, n), b(n + 1);
    if (variant == 1)
      LAUNCH(n, (k_AddConst<C, C, C>(a.data(), cc, b.data(), n)));
    else
      LAUNCH(n, (k_AddConst<C, float, C>(a.data(), cr, b.data(), n)));
    keep((C*)out, b, n);
  }
}

void ref_add_to_magnitude(const C* x, float c, C* out, size_t n) {
  std::vector<C> a = extended(x, n), b(n + 1);
  LAUNCH(n, k_AddToMagnitude(a.data(), c, b.data(), n));
  keep(out, b, n);
}

/* variant: 0 CC, 1 FF, 2 CF (complex in1, real in2) */
void ref_multiply(int variant, const void* p, const void* q, void* out, size_t n) {
  if (variant == 1) {
    std::vector<float> a = extended((const float*)p, n), b = extended((const float*)q, n), c(n + 1);
    LAUNCH(n, (k_Multiply<float, float, float>(a.data(), b.data(), c.data(), n)));
    keep((float*)out, c, n);
  } else if (variant == 0) {
    std::vector<C> a = extended((const C*)p, n), b = extended((const C*)q, n), c(n + 1);
    LAUNCH(n, (k_Multiply<C, C, C>(a.data(), b.data(), c.data(), n)));
    keep((C*)out, c, n);
  } else {
    std::vector<C> a = extended((const C*)p, n), c(n + 1);
    std::vector<float> b = extended((const float*)q, n);
    LAUNCH(n, (k_Multiply<C, float, C>(a.data(), b.data(), c.data(), n)));
    keep((C*)out, c, n);
  }
}

/* The wrappers of trig.cu form the per-index step on the host: the float difference of the two phases divided
 * in double by the element count, rounded to float. */
void ref_cosine(int complex_out, float phi_begin, float phi_end, void* out, size_t n) {
  const float span = phi_end - phi_begin;
  const float step = (float)((double)span / (double)n);
  if (complex_out) {
    std::vector<C> b(n + 1);
    LAUNCH(n, k_ComplexCosine(step, phi_begin, b.data(), n));
    keep((C*)out, b, n);
  } else {
    std::vector<float> b(n + 1);
    LAUNCH(n, k_RealCosine(step, phi_begin, b.data(), n));
    keep((float*)out, b, n);
  }
}

void ref_int8_to_float(const int8_t* x, float* out, size_t n) {
  std::vector<int8_t> a = extended(x, n);
  std::vector<float> b(n + 1);
  LAUNCH(n, k_int8ToFloat(a.data(), b.data(), n));
  keep(out, b, n);
}

void ref_qpsk_mod(const uint8_t* bits, C* out, uint32_t n, float a) { LAUNCH(n, k_QpskModulate(bits, out, n, a)); }

void ref_qpsk_mod_4x(const uint8_t* b0, const uint8_t* b1, const uint8_t* b2, const uint8_t* b3, C* o0, C* o1, C* o2,
                     C* o3, uint32_t n, float a) {
  LAUNCH(n, k_QpskModulate4x(b0, b1, b2, b3, o0, o1, o2, o3, n, a));
}

/* streams in {1, 2, 4, 8}: the instantiations the reference makes; returns 0 for any other count */
int ref_qpsk_mod_templated(int streams, const uint8_t* bits, C* out, uint32_t n, float a) {
  switch (streams) {
    case 1: LAUNCH(n, k_QpskModulateTemplated<1>(bits, out, n, a)); return 1;
    case 2: LAUNCH(n, k_QpskModulateTemplated<2>(bits, out, n, a)); return 1;
    case 4: LAUNCH(n, k_QpskModulateTemplated<4>(bits, out, n, a)); return 1;
    case 8: LAUNCH(n, k_QpskModulateTemplated<8>(bits, out, n, a)); return 1;
  }
  return 0;
}

/* one thread of one block, as gsdrQpsk256InitConstellation launches the init kernels */
void ref_qpsk256_table(uint32_t type, float amplitude, C* table) {
  blockDim = dim3(1);
  blockIdx.x = threadIdx.x = 0;
  if (type == 0)
    k_InitQpsk256Rectangular(table, amplitude);
  else
    k_InitQpsk256Circular(table, amplitude);
}

static void load_table(uint32_t type, float amplitude) {
  ref_qpsk256_table(type, amplitude, type == 0 ? c_qpsk256_rectangular : c_qpsk256_circular);
}

void ref_qpsk256_mod(uint32_t type, float amplitude, const uint8_t* in, C* out, uint32_t n) {
  load_table(type, amplitude);
  LAUNCH(n, k_Qpsk256Modulate(in, out, n, amplitude, type));
}

void ref_qpsk256_mod_4x(uint32_t type, float amplitude, const uint8_t* i0, const uint8_t* i1, const uint8_t* i2,
                        const uint8_t* i3, C* o0, C* o1, C* o2, C* o3, uint32_t n) {
  load_table(type, amplitude);
  LAUNCH(n, k_Qpsk256Modulate4x(i0, i1, i2, i3, o0, o1, o2, o3, n, amplitude, type));
}

} /* extern "C" */
