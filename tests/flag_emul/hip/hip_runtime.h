// A stand-in for <hip/hip_runtime.h> that lets csrc/flag_kernels.h compile as host C++ (tests/test_flag_emul_cpu.py): a work-group is
// as many host threads as it has threads, __syncthreads a pthread barrier of those, and `__shared__` a function-local static -- the
// driver runs one work-group at a time, so its threads share the one instance, which keeps what the work-group before left in it,
// as LDS does.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
struct alignas(8) float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static inline float2 make_float2(float x, float y) { return {x, y}; }
struct dim3e { int x = 0, y = 0, z = 0; };
extern thread_local dim3e threadIdx, blockIdx;
extern pthread_barrier_t g_bar;
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
