// A stand-in for <hip/hip_runtime.h> that lets csrc/fold_kernels.h compile unchanged as host C++ (tests/test_fold_emul_cpu.py): the
// stand-in of tests/rfi_emul/ (a work-group is 256 host threads, __syncthreads a pthread barrier, `__shared__` a static, __host__,
// gridDim, float2 / float4 and make_float4) and the correctly rounded division the dump normalises with.  The kernels have no
// shuffles and no dynamic LDS.  The driver is compiled with -ffp-contract=off and fmaf is libm's.
#pragma once
#include "../../rfi_emul/hip/hip_runtime.h"
static inline float __fdiv_rn(float a, float b) { return a / b; }
