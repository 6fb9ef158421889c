// A stand-in for <hip/hip_runtime.h> that lets csrc/toa_kernels.h compile as host C++ (tests/test_toa_emul_cpu.py): the stand-in of
// tests/rfi_emul/ (a work-group is 256 host threads, __syncthreads a pthread barrier, the dynamic LDS a global pointer, float2,
// float4 and their makers, the grid size).  The driver is compiled with -ffp-contract=off, fmaf is libm's and the division is IEEE:
// every step of the contract is one correctly rounded float32 operation.
#pragma once
#include "../../rfi_emul/hip/hip_runtime.h"
