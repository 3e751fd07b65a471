/*
 * Host shim for the reference-run libraries (oracle/_ref/) -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference's kernels are one-thread-per-element CUDA functions with no shuffles, shared memory or atomics
 * (the ones driven here; oracle/README.md lists what is left out). With the CUDA headers for the types
 * (cuComplex, uint3, dim3) and the function-space keywords defined away, g++ compiles their text as ordinary
 * inline functions that read the launch coordinates from three globals, which driver.cpp sets in a loop over
 * blocks and threads. Nothing here is taken from the reference: these are the CUDA built-ins its kernels use,
 * restated for the host.
 */
#ifndef GSDR_REFHOST_SHIM_H_
#define GSDR_REFHOST_SHIM_H_

#include <cuComplex.h>
#include <cuda_runtime.h>

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#undef __global__
#undef __device__
#undef __host__
#undef __forceinline__
#define __global__ inline
#define __device__
#define __host__
#define __forceinline__ inline

/* the launch coordinates of the thread being emulated */
static uint3 threadIdx, blockIdx;
static dim3 blockDim;

#ifndef M_PIf
#define M_PIf 3.14159265358979323846f
#endif

/* CUDA __saturatef: clamp to [0, 1], NaN -> +0 */
static inline float __saturatef(float x) { return x != x ? 0.0f : (x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x)); }
/* CUDA __uint2float_rn: round to nearest even, the host's default conversion */
static inline float __uint2float_rn(unsigned int x) { return (float)x; }
/* CUDA's device overloads of max / min used by the driven kernels */
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline int min(int a, int b) { return a < b ? a : b; }

#endif /* GSDR_REFHOST_SHIM_H_ */
