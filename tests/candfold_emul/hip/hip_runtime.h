// A stand-in for <hip/hip_runtime.h> that lets csrc/candfold_kernels.h compile as host C++ (tests/test_candfold_emul_cpu.py): the
// stand-in of tests/plong_emul/ with the grid size, the bit casts and the correctly rounded operations these kernels use (the
// driver is compiled with -ffp-contract=off: a plain float operation is one IEEE operation).
#pragma once
#include "../../plong_emul/hip/hip_runtime.h"
extern thread_local dim3e gridDim;
#define __host__
static inline float __uint_as_float(uint32_t i) { float f; memcpy(&f, &i, 4); return f; }
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fsub_rn(float a, float b) { return a - b; }
static inline float __fmul_rn(float a, float b) { return a * b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
