// gsdr-mi355x, FIR engine: sample types in memory and in LDS, the multiply-accumulate forms, 16-byte streaming accesses.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fir_plan.hpp"

namespace gsdr {

// ------------------------------------------------------------------------------------------------
// Sample and product types
// ------------------------------------------------------------------------------------------------
// Interleaved int8 I/Q (2 bytes per sample, the SDR front-end format): converted to float while
// staging with gsdrInt8ToNormFloat's semantics (reference src/conversion.cu:26), so the float
// samples exist only in LDS.
struct Iq8 {
  int8_t x, y;
};

// The sample kind of a type (fir_plan.hpp: samples per 16-byte LDS granule, bytes one staging load moves per granule).
template <class T>
struct SampleKind;
template <>
struct SampleKind<float> : std::integral_constant<int, firplan::kSampleReal> {};
template <>
struct SampleKind<float2> : std::integral_constant<int, firplan::kSampleComplex> {};
template <>
struct SampleKind<Iq8> : std::integral_constant<int, firplan::kSampleIq8> {};
template <class T>
struct SampleT {
  static constexpr int kPerGranule = firplan::per_granule(SampleKind<T>::value);
  static constexpr int kSrcAlign = firplan::src_align(SampleKind<T>::value);
};

// sample type as held in LDS (what the compute core reads)
template <class T>
struct LdsSample {
  using type = T;
};
template <>
struct LdsSample<Iq8> {
  using type = float2;
};

// max(-1, v / 127.0f) with IEEE division, from one multiply and an fma correction: equal to the
// correctly rounded quotient for every int8 value (checked exhaustively, tests/test_gpu_int8.py);
// clamping to -127 first gives the reference's max(-1, .) for -128.
__device__ __forceinline__ float norm_i8(int v) {
  const float x = (float)max(v, -127);
  constexpr float r = 1.0f / 127.0f;
  const float q = x * r;
  return fmaf(fmaf(-q, 127.0f, x), r, q);
}
__device__ __forceinline__ float2 to_lds_sample(Iq8 v) { return make_float2(norm_i8(v.x), norm_i8(v.y)); }
__device__ __forceinline__ float2 to_lds_sample(float2 v) { return v; }
__device__ __forceinline__ float to_lds_sample(float v) { return v; }

// two Iq8 samples packed in a dword -> one LDS granule
__device__ __forceinline__ float4 iq8x2_granule(uint32_t w) {
  const int b0 = (int)(w << 24) >> 24, b1 = (int)(w << 16) >> 24, b2 = (int)(w << 8) >> 24, b3 = (int)w >> 24;
  return make_float4(norm_i8(b0), norm_i8(b1), norm_i8(b2), norm_i8(b3));
}

template <class TapT, class InT>
struct Product {
  using type = float2;
};
template <>
struct Product<float, float> {
  using type = float;
};

__device__ __forceinline__ void set_zero(float& a) { a = 0.0f; }
__device__ __forceinline__ void set_zero(float2& a) { a = make_float2(0.0f, 0.0f); }
__device__ __forceinline__ void set_zero(Iq8& a) {
  a.x = 0;
  a.y = 0;
}

// Element e (compile-time after unrolling) of a 16-byte granule.
template <class InT>
__device__ __forceinline__ InT granule_sample(const float4& g, int e);
template <>
__device__ __forceinline__ float granule_sample<float>(const float4& g, int e) {
  return e == 0 ? g.x : (e == 1 ? g.y : (e == 2 ? g.z : g.w));
}
template <>
__device__ __forceinline__ float2 granule_sample<float2>(const float4& g, int e) {
  return e == 0 ? make_float2(g.x, g.y) : make_float2(g.z, g.w);
}

// acc += x * t, with the component products of the reference's cuComplex operator overloads
// (reference src/cuComplexOperatorOverloads.cuh:25-33: c*r, r*c, cuCmulf).
__device__ __forceinline__ void mac(float& acc, float x, float t) { acc = fmaf(x, t, acc); }
__device__ __forceinline__ void mac(float2& acc, float2 x, float t) {
  acc.x = fmaf(x.x, t, acc.x);
  acc.y = fmaf(x.y, t, acc.y);
}
__device__ __forceinline__ void mac(float2& acc, float x, float2 t) {
  acc.x = fmaf(t.x, x, acc.x);
  acc.y = fmaf(t.y, x, acc.y);
}
__device__ __forceinline__ void mac(float2& acc, float2 x, float2 t) {
  acc.x = fmaf(x.x, t.x, acc.x);
  acc.x = fmaf(-x.y, t.y, acc.x);
  acc.y = fmaf(x.x, t.y, acc.y);
  acc.y = fmaf(x.y, t.x, acc.y);
}

// Non-temporal (streaming) 16-byte load: global_load_dwordx4 ... nt.
typedef float gsdr_f32x4 __attribute__((ext_vector_type(4)));
typedef float gsdr_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 load16_nt(const float4* p) {
  const gsdr_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const gsdr_f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void store16_nt(float4* p, float4 v) {
  __builtin_nontemporal_store(gsdr_f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<gsdr_f32x4*>(p));
}

}  // namespace gsdr
