// A stand-in for <hip/hip_runtime.h> that lets csrc/predict_kernels.h compile as host C++ (tests/test_predict_emul_cpu.py): a
// work-group of predict_kernel is one wave of 64 host threads, __syncthreads a pthread barrier of those, the 32x32x2 f32 MFMA an
// exchange of the wave's operands between two such barriers followed by the k-ordered fmaf chain of the lane's 16 elements
// (A[row][k] from lane row + 32 k, B[k][col] from lane col + 32 k, C/D register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h,
// column r), sincospif in double precision and the static LDS a global pointer.
#pragma once
#include <pthread.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <cstddef>
struct float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
static inline float2 make_float2(float x, float y) { return {x, y}; }
static inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
struct dim3e { int x = 0, y = 0, z = 0; };
extern thread_local dim3e threadIdx, blockIdx;
extern pthread_barrier_t g_bar;
extern uint8_t* g_lds;
extern float g_a[64], g_b[64];
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline void sincospif(float x, float* s, float* c) { *s = (float)sin(M_PI * (double)x); *c = (float)cos(M_PI * (double)x); }
struct f16v { float e[16] = {}; float& operator[](int i) { return e[i]; } const float& operator[](int i) const { return e[i]; } };
static inline f16v emul_mfma(float a, float b, f16v c) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    g_a[lane] = a; g_b[lane] = b;
    pthread_barrier_wait(&g_bar);
    for (int v = 0; v < 16; v++) {
        const int row = (v & 3) + 8 * (v >> 2) + 4 * h;
        for (int k = 0; k < 2; k++) c.e[v] = fmaf(g_a[row + 32 * k], g_b[r + 32 * k], c.e[v]);
    }
    pthread_barrier_wait(&g_bar);
    return c;
}
#define __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, x, y, z) emul_mfma(a, b, c)
