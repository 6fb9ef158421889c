// A stand-in for <hip/hip_runtime.h> that lets csrc/accel_kernels.h (and csrc/plong_kernels.h, which it includes) compile as host
// C++ (tests/test_accel_emul_cpu.py): the stand-in of tests/plong_emul/ with the two functions the gather and the best-over-trials
// kernel add.
#pragma once
#include "../../plong_emul/hip/hip_runtime.h"
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
// round to nearest, ties to even (the default rounding mode; nothing here changes it)
static inline long long __double2ll_rn(double x) { return std::llrint(x); }
