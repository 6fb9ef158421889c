// A stand-in for <hip/hip_runtime.h> that lets csrc/dedisp_kernels.h compile unchanged as host C++ (tests/test_dedisp_emul_cpu.py):
// the stand-in of tests/plong_emul/ (a work-group is 256 host threads, __syncthreads a pthread barrier, `__shared__` a static).  The
// kernels have no shuffles and no dynamic LDS.  The driver is compiled with -ffp-contract=off and fmaf is libm's: a plain float
// operation is one IEEE operation and the fused one is correctly rounded.
#pragma once
#include "../../plong_emul/hip/hip_runtime.h"
