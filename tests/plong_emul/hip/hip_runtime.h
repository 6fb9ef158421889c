// A stand-in for <hip/hip_runtime.h> that lets csrc/plong_kernels.h compile as host C++ (tests/test_plong_emul_cpu.py): a work-group
// is 256 host threads, __syncthreads a pthread barrier, __shfl_xor an exchange through a shared array between two barriers of the
// wave's own 64 threads (every call site in the kernels is reached by all threads of the wave), `__shared__` a static, and the
// dynamic LDS a global pointer.  The scheme of tests/ffa_emul/, with the complex types and bit functions these kernels use.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
struct dim3e { int x = 0, y = 0, z = 0; };
extern thread_local dim3e threadIdx, blockIdx;
extern pthread_barrier_t g_bar, g_wbar[4];
extern float* g_lds;
extern uint32_t g_slot[256];
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
static inline uint32_t __float_as_uint(float f) { uint32_t i; memcpy(&i, &f, 4); return i; }
static inline uint32_t __brev(uint32_t v) {
    uint32_t r = 0;
    for (int b = 0; b < 32; b++) r |= ((v >> b) & 1u) << (31 - b);
    return r;
}
template <class T> static inline T __shfl_xor(T v, int o) {
    uint32_t u; memcpy(&u, &v, 4);
    g_slot[threadIdx.x] = u;
    pthread_barrier_wait(&g_wbar[threadIdx.x >> 6]);
    uint32_t r = g_slot[threadIdx.x ^ o];
    pthread_barrier_wait(&g_wbar[threadIdx.x >> 6]);
    T out; memcpy(&out, &r, 4); return out;
}
