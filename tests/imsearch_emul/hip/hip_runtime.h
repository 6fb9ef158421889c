// A stand-in for <hip/hip_runtime.h> that lets csrc/imsearch_kernels.h compile as host C++ (tests/test_imsearch_emul_cpu.py): a
// work-group is a set of host threads, __syncthreads a pthread barrier of those, the static LDS a global pointer.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
struct alignas(8) float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
static inline float2 make_float2(float x, float y) { return {x, y}; }
static inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
struct dim3e { int x = 0, y = 0, z = 0; };
extern thread_local dim3e threadIdx, blockIdx;
extern pthread_barrier_t g_bar;
extern uint8_t* g_lds;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
