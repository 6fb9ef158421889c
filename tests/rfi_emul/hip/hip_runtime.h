// A stand-in for <hip/hip_runtime.h> that lets csrc/rfi_kernels.h compile as host C++ (tests/test_rfi_emul_cpu.py): the stand-in of
// tests/plong_emul/ with the grid size and the vector types these kernels use (the driver is compiled with -ffp-contract=off: a
// plain float operation is one IEEE operation, and division and square root are correctly rounded on the host).
#pragma once
#include "../../plong_emul/hip/hip_runtime.h"
extern thread_local dim3e gridDim;
#define __host__
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
