// A stand-in for <hip/hip_runtime.h> that lets csrc/clean_kernels.h compile as host C++ (tests/test_clean_emul_cpu.py): a work-group
// is 256 host threads, __syncthreads a pthread barrier of those, sincospif in double precision, the dynamic LDS a global pointer, the
// grid's size a global the driver sets before each launch.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
struct dim3e { int x = 0, y = 0, z = 0; };
extern thread_local dim3e threadIdx, blockIdx;
extern dim3e gridDim;
extern pthread_barrier_t g_bar;
extern uint8_t* g_lds;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline void sincospif(float x, float* s, float* c) { *s = (float)sin(M_PI * (double)x); *c = (float)cos(M_PI * (double)x); }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
