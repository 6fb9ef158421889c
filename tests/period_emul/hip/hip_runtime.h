// A stand-in for <hip/hip_runtime.h> that lets csrc/period_kernels.h compile as host C++ (tests/test_period_emul_cpu.py): a work-group is
// 256 host threads, __syncthreads a pthread barrier, __shfl_xor an exchange through a shared array between two barriers (every call
// site in the kernel is reached by all threads of the work-group), `__shared__` a static, and the dynamic LDS a global pointer.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
static inline float2 make_float2(float x, float y) { return {x, y}; }
struct dim3e { int x = 0, y = 0, z = 0; };
extern thread_local dim3e threadIdx, blockIdx;
extern pthread_barrier_t g_bar;
extern float2* g_lds;
extern uint32_t g_slot[256];
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline uint32_t __brev(uint32_t x) { uint32_t r = 0; for (int i = 0; i < 32; i++) r |= ((x >> i) & 1u) << (31 - i); return r; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
template <class T> static inline T __shfl_xor(T v, int o) {
    uint32_t u; memcpy(&u, &v, 4);
    g_slot[threadIdx.x] = u;
    pthread_barrier_wait(&g_bar);
    uint32_t r = g_slot[threadIdx.x ^ o];
    pthread_barrier_wait(&g_bar);
    T out; memcpy(&out, &r, 4); return out;
}
