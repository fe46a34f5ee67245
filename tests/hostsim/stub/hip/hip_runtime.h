// TEST-ONLY stand-in for <hip/hip_runtime.h> when the kernel headers are compiled for the host (tests/hostsim): everything they
// use of HIP - threadIdx / blockIdx, __syncthreads, __shared__ storage, the cross-lane intrinsics, the raw buffer builtins, float4 /
// uint4, __uint_as_float - comes from wave_emu.h,
// which the including unit pulls in first.
#pragma once
#include "../../wave_emu.h"
