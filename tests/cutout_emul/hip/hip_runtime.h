// A stand-in for <hip/hip_runtime.h> that lets csrc/cutout_kernels.h (and csrc/dedisp_kernels.h, whose ingest it launches) compile as
// host C++ (tests/test_cutout_emul_cpu.py): the stand-in of tests/detrend_emul/ (a work-group is 256 host threads, __syncthreads a
// pthread barrier, `__shared__` a static, the dynamic LDS a global pointer, the integer atomic add on a count word in LDS).  The
// driver is compiled with -ffp-contract=off, fmaf is libm's and the division is IEEE: every step of the contract is one correctly
// rounded float32 operation.
#pragma once
#include "../../detrend_emul/hip/hip_runtime.h"
