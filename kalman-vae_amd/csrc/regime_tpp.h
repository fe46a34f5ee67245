// regime_tpp.h — the thread-per-sequence kernels of the regime chain (regime.h bodies with the regime count a compile-time
// constant; see kvae_lgssm_tpp.hip, which instantiates and launches them for K = 2..8).  A header of their own so that the
// test-only emulated workgroups (tests/hostsim) compile these very lines: sequence b = 64 * block + lane, ragged last block.
// Included at global scope after regime.h, by a unit that builds the bodies with a serial KV_PAR (KV_TPP, or KVAE_HOSTSIM).
#pragma once
#include "regime.h"

template <int KC>
__global__ __launch_bounds__(64) void k_regime_fwd_tpp(const float *logits, const float *init_logits, const float *gumbel,
                                                       const float *P, float *y_seq, float *log_q, float *log_p, int B, int T,
                                                       float tau, const float *tau_dev, int hard) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (tau_dev) tau = *tau_dev;
  kvae::RegimeLds L;
  kvae::regime_fwd_body(logits, init_logits, gumbel, P, y_seq, log_q, log_p, b, T, KC, tau, hard, L);
}
template <int KC>
__global__ __launch_bounds__(64) void k_regime_bwd_tpp(const float *logits, const float *init_logits, const float *gumbel,
                                                       const float *P, const float *y_seq, const float *g_y, const float *g_lq,
                                                       const float *g_lp, float *g_logits, float *g_init, int B, int T, float tau,
                                                       const float *tau_dev) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (tau_dev) tau = *tau_dev;
  kvae::RegimeLds L;
  kvae::regime_bwd_body(logits, init_logits, gumbel, P, y_seq, g_y, g_lq, g_lp, g_logits, g_init, b, T, KC, tau, L);
}
