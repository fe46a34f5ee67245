// emission_means.h — imputation read-out: a = C_t mu_t for the smoothed and the filtered means in one launch (model.py:279-288).
// One thread per (sequence step, output row); the grid (emission_blocks) sits beside the kernel for kvae_lgssm.hip and for the
// test-only emulated workgroups (tests/hostsim/wave_emu_step.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kvae_lgssm.h"

namespace kvae {
inline unsigned emission_blocks(int64_t BT, int p) { return (unsigned)((BT * p + 255) / 256); }
}  // namespace kvae

// (the kernel keeps the name it had in kvae_lgssm.hip: outside the namespace)
__global__ __launch_bounds__(256) void k_emission_means(kvae_stack C, const float *__restrict__ ms, const float *__restrict__ mf,
                                                        float *__restrict__ a_s, float *__restrict__ a_f, int64_t BT, int T, int n,
                                                        int p) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= BT * p) return;
  const int64_t q = idx / p;
  const int i = (int)(idx % p);
  const float *c = C.ptr + (q / T) * C.sb + (q % T) * C.st + (int64_t)i * n;
  float s = 0.f, f = 0.f;
  for (int k = 0; k < n; ++k) {
    const float ck = c[k];
    if (ms) s = fmaf(ck, ms[q * n + k], s);
    if (mf) f = fmaf(ck, mf[q * n + k], f);
  }
  if (a_s) a_s[idx] = s;
  if (a_f) a_f[idx] = f;
}
