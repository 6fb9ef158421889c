// A stand-in for <hip/hip_runtime.h> that lets csrc/detrend_kernels.h compile as host C++ (tests/test_detrend_emul_cpu.py): the
// stand-in of tests/rfi_emul/ (a work-group is 256 host threads, __syncthreads a pthread barrier, __shfl_xor an exchange through a
// shared array between two barriers of the wave's own 64 threads, the dynamic LDS a global pointer) with the bit cast and the integer
// atomic add (on a count word in LDS) these kernels add.  The driver is compiled with -ffp-contract=off and the division is
// IEEE: every step of the contract is one correctly rounded float32 operation.
#pragma once
#include "../../rfi_emul/hip/hip_runtime.h"
static inline float __uint_as_float(uint32_t i) { float f; memcpy(&f, &i, 4); return f; }
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
