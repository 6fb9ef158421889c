// A stand-in for <hip/hip_runtime.h> that lets csrc/peel_kernels.h compile as host C++ (tests/test_peel_emul_cpu.py): a work-group
// of peel_solve_kernel is 256 host threads, one of peel_subtract_kernel 64; __syncthreads is a pthread barrier the driver sizes to the
// kernel it runs, __shfl_xor an exchange through a shared array between two barriers of the wave's 64 threads (every call site is
// reached by whole waves), an MFMA an exchange of the wave's operands between two such barriers followed by the k-ordered fmaf chain
// of the lane's elements --
//   16x16x4 f32: A[row][k] from lane row + 16 k, B[k][col] from lane col + 16 k, C/D register v of lane l = row 4 (l >> 4) + v, column l & 15
//   32x32x2 f32: A[row][k] from lane row + 32 k, B[k][col] from lane col + 32 k, C/D register v of lane (r, h) = row (v & 3) + 8 (v >> 2) + 4 h, column r
// -- sincospif in double precision, and the LDS a global pointer.  peel_steer_kernel has no barrier: the driver calls it thread after
// thread.
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
extern pthread_barrier_t g_bar, g_wbar[4];
extern uint8_t* g_lds;
extern float g_slot[256], g_a[256], g_b[256];
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline void sincospif(float x, float* s, float* c) { *s = (float)sin(M_PI * (double)x); *c = (float)cos(M_PI * (double)x); }
static inline float __shfl_xor(float v, int o) {
    const int tid = threadIdx.x, wave = tid >> 6;
    g_slot[tid] = v;
    pthread_barrier_wait(&g_wbar[wave]);
    float r = g_slot[wave * 64 + ((tid & 63) ^ o)];
    pthread_barrier_wait(&g_wbar[wave]);
    return r;
}
struct f4v { float e[4] = {}; float& operator[](int i) { return e[i]; } const float& operator[](int i) const { return e[i]; } };
struct f16v { float e[16] = {}; float& operator[](int i) { return e[i]; } const float& operator[](int i) const { return e[i]; } };
static inline f4v emul_mfma16(float a, float b, f4v c) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    g_a[tid] = a; g_b[tid] = b;
    pthread_barrier_wait(&g_wbar[wave]);
    for (int v = 0; v < 4; v++) {
        const int row = 4 * (lane >> 4) + v;
        for (int k = 0; k < 4; k++) c.e[v] = fmaf(g_a[wave * 64 + row + 16 * k], g_b[wave * 64 + (lane & 15) + 16 * k], c.e[v]);
    }
    pthread_barrier_wait(&g_wbar[wave]);
    return c;
}
static inline f16v emul_mfma32(float a, float b, f16v c) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    g_a[tid] = a; g_b[tid] = b;
    pthread_barrier_wait(&g_wbar[wave]);
    for (int v = 0; v < 16; v++) {
        const int row = (v & 3) + 8 * (v >> 2) + 4 * h;
        for (int k = 0; k < 2; k++) c.e[v] = fmaf(g_a[wave * 64 + row + 32 * k], g_b[wave * 64 + r + 32 * k], c.e[v]);
    }
    pthread_barrier_wait(&g_wbar[wave]);
    return c;
}
#define __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, x, y, z) emul_mfma16(a, b, c)
#define __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, x, y, z) emul_mfma32(a, b, c)
