// lgssm_swf.h — the causal switching Kalman filter with second-order generalised pseudo-Bayes collapse (GPB2, Murphy 1998) of the
// switching dynamics (include/kvae_lgssm.h kvae_lgssm_switching_filter, lgssm_ops.switching_filter, KalmanFilter.filter_regimes,
// KVAE.filter_regimes).  The equations are in the header of the C ABI; this file is their layout on a wavefront.
//
// One wavefront per sequence, laid out as the 8 x 8 grid of regime_grid.h / regime_decode.h: lane = 8 g + k owns the pair
// (previous regime i = k, current regime j = g).  A_j, B_j, Q_j, C, R and log P[i,j] are loaded once, padded with zeros to
// 4 x 4 (run-time n, m <= 4), and stay in registers for the whole sweep; only y_t, u_t, mask_t are streamed, one step ahead of
// the step that uses them, from a clamped address (the last step fetches itself again).
//   per step, on every lane: the filter step of pair (i, j) from (mu^i, Sigma^i) and the pair density - kvae_sw::predict and
//     kvae_sw::update (csrc/lgssm_sw_pair.h, where the per-pair statements of the four GPB2 kernels are written once).
//   reductions over i inside a column j: the eight lanes of group g, three DPP moves each (rgrid::oct_sum / oct_max): the column
//     maximum, the softmax weights W_{i|j}, log w'(j) and the fourteen sums of the collapse.  Every lane of the group ends with
//     the same bits ("on the groups").
//   reductions over j, and over all pairs: the eight groups, two DPP mirrors and two permlane swaps (rdec::xg8) - the step's
//     log-likelihood, the moment match of the K collapsed Gaussians and (after a group reduction) of the K^2 pair forecasts.
//   hand-over: lane (i = k, j = g) of the next step needs regime k's collapsed belief, which group k holds: fifteen __shfl from
//     lane 8 k - the transpose of the grid.
// Padding lanes (k >= K or g >= K) hold zero operands, log c = -inf and weight 0: every value on them is finite, they take every
// branch the live lanes take (all branches test kernel arguments only), and they store nothing.  No per-lane array is indexed at
// run time (every loop below is unrolled over constants), no LDS, no scratch.  Every multiply-add is an explicit fmaf and the
// unit is compiled with contraction off, so the bits of an output do not depend on which others are requested.
#pragma once
#include "lgssm_sw_pair.h"

namespace kvae_swf {

using kvae::rgrid::oct_sum;
using kvae_sw::padded;
using kvae_sw::wave_max;

constexpr int MAX_K = 8, MAX_N = 4, MAX_M = 4;

// What the smoother's forward (csrc/lgssm_sws.h, k_sws_fwd) keeps of every step: the collapsed per-regime beliefs - the values the
// sweep hands to step t + 1 - the pair weights W of that step, and the weights after the last step.  The forward of the
// differentiable log-likelihood (csrc/lgssm_swm.h, k_swm_fwd: HIST = 2) keeps the beliefs and, in place of W and w, the log weights
// log w' handed to step t + 1; its adjoint recomputes W, and the forecast (csrc/lgssm_swh.h, k_swh_fwd: HIST = 2 as well) starts
// every origin from them.  The filter's own sweep (HIST = 0) holds none of it and compiles to what it was.
struct History {
  float *mu;      // [B,T,K,n]
  float *Sigma;   // [B,T,K,n,n]
  float *W;       // [B,T,K,K], indexed (i, j)          (HIST = 1)
  float *w;       // [B,K]: regime_filt of step T - 1   (HIST = 1)
  float *lw;      // [B,T,K]: log w' of every step      (HIST = 2)
};

template <int HIST = 0>
__device__ inline void sweep_wave(const kvae_swf_problem &P, const History H = History{}) {
  const kvae_sw::Lane ln = kvae_sw::lane_of(P.K);
  const auto [lane, k, g, kc, gc, vk, vg, ve] = ln;
  const int T = P.T, K = P.K, n = P.n, m = P.m;
  const int64_t b = blockIdx.x;
  // ---- operands of the sweep: regime j = g's dynamics, the shared emission, log P[i = k, j = g] ----
  float A[4][4], Bm[4][4], Q[4][4];
  kvae_sw::Emission E;
  kvae_sw::load_dynamics(P, gc, vg, A, Bm, Q);
  kvae_sw::load_emission(P, ln, E);
  // ---- the carried belief of regime i = k ("along the lanes") ----
  const bool carried = P.state_log_w != nullptr;
  float mu[4], Sg[4][4], lw;
  {
    const float *m0 = carried ? P.state_mu + (b * K + kc) * n : P.mu0;
    const float *S0 = carried ? P.state_Sigma + (b * K + kc) * n * n : P.Sigma0;
    const float *w0 = carried ? P.state_log_w + b * K + kc : P.R;   // a valid address either way
    const float lw0 = *w0;
    lw = vk ? (carried ? lw0 : E.lPuni) : -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mu[r] = padded(m0, 1, n, 0, r, vk);
#pragma unroll
      for (int c = 0; c < 4; ++c) Sg[r][c] = padded(S0, n, n, r, c, vk);
    }
  }
  // ---- y_0, u_0, mask_0 ----
  const int64_t q0 = b * T;
  const float *maskp = P.mask ? P.mask + q0 : P.R;   // always a valid address (the note at mask_addr, csrc/lgssm_fwd.h)
  const int mstep = P.mask ? 1 : 0;
  float yn0 = P.y[q0 * 2], yn1 = P.y[q0 * 2 + 1], mkn = maskp[0], un[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) un[c] = padded(P.u + q0 * m, 1, m, 0, c, true);

  for (int t = 0; t < T; ++t) {
    const int64_t q = q0 + t;
    const float y0 = yn0, y1 = yn1, mk = P.mask ? mkn : 1.0f;
    const float u[4] = {un[0], un[1], un[2], un[3]};
    {   // the next step's, in flight while this one computes
      const int tn = t + 1 < T ? t + 1 : t;
      const int64_t qn = q0 + tn;
      yn0 = P.y[qn * 2], yn1 = P.y[qn * 2 + 1], mkn = maskp[tn * mstep];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = padded(P.u + qn * m, 1, m, 0, c, true);
    }
    const bool observed = mk != 0.0f, first = t == 0 && !carried;
    // ---- the Kalman step of pair (i, j): predict, forecast, S, the pair density, gain, Joseph update ----
    float mp[4], AS[4][4], Sp[4][4];
    kvae_sw::Update U;   // of Sf, the upper triangle is read
    kvae_sw::predict(A, Bm, Q, mu, Sg, u, mp, AS, Sp);
    kvae_sw::update(E.C, E.R, mp, Sp, y0, y1, mk, U);
    // ---- weights: log c_ij, the prior weight w(i) P[i,j], the column softmax ----
    const float lPt = first ? (ve ? E.lPuni : -INFINITY) : E.lPij, Pt = first ? (ve ? E.Puni : 0.0f) : E.Pij;
    const float lij = observed ? U.tl.ll : 0.0f;
    const float pw = ve ? expf(lw) * Pt : 0.0f;
    const float rp = oct_sum(pw);                                   // regime_pred(j), on the groups
    const kvae_sw::Weights wt = kvae_sw::weights(ln, lw, lPt, lij);
    const float W = wt.W, tot = wt.tot;
    const float lwn = (wt.cmx + logf(wt.se)) - tot;                 // log w'(j), on the groups
    const float rf = vg ? expf(lwn) : 0.0f;
    // ---- collapse over i ----
    float mc[4], Sc[4][4];
    kvae_sw::collapse_pairs(W, U.muf, U.Sf, mc, Sc);
    // ---- the step's outputs ----
    if (P.regime_pred && vg && k == 0) P.regime_pred[q * K + g] = rp;
    if (P.regime_filt && vg && k == 0) P.regime_filt[q * K + g] = rf;
    if (P.ll && lane == 0) P.ll[q] = observed ? tot : 0.0f;
    if (P.levels) {
      const float lv = wave_max(pw > 0.0f ? (float)U.tl.level : 0.0f);
      if (lane == 0) P.levels[q] = (int32_t)lv;
    }
    kvae_sw::forecast_outputs(ln, U, pw, q, P.a_pred, P.S_out);               // moment match of the K^2 pair forecasts
    kvae_sw::belief_outputs(ln, n, rf, mc, Sc, q, P.mus_filt, P.Sigmas_filt);   // moment match of the K collapsed Gaussians under w'
    if constexpr (HIST != 0) {   // the step's history: every live lane its own W, one lane per group the belief of regime j = g
      const bool w = vg && k == 0;
      const int64_t s = q * K + g;
      if constexpr (HIST == 1) {
        if (ve) H.W[(q * K + k) * K + g] = W;
        if (t == T - 1 && w) H.w[b * K + g] = rf;
      } else {
        if (w) H.lw[s] = lwn;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (w && r < n) H.mu[s * n + r] = mc[r];
#pragma unroll
        for (int c = r; c < 4; ++c)
          if (w && c < n) H.Sigma[(s * n + r) * n + c] = Sc[r][c], H.Sigma[(s * n + c) * n + r] = Sc[r][c];
      }
    }
    if (t == T - 1) {   // the carried state out: regime j = g, one lane per group
      const bool w = vg && k == 0;
      const int64_t s = b * K + g;
      if (P.out_log_w && w) P.out_log_w[s] = lwn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (P.out_mu && w && r < n) P.out_mu[s * n + r] = mc[r];
#pragma unroll
        for (int c = r; c < 4; ++c)
          if (P.out_Sigma && w && c < n) P.out_Sigma[(s * n + r) * n + c] = Sc[r][c], P.out_Sigma[(s * n + c) * n + r] = Sc[r][c];
      }
    }
    // ---- hand-over: lane (i = k, j = g) takes regime k's belief from group k ----
    kvae_sw::hand_over(k << 3, vk, -INFINITY, lwn, mc, Sc, lw, mu, Sg);
  }
}

// ---- seq_ll[b] = sum_t ll[b, t]: one wavefront per sequence, lane-strided partial sums in ascending t, then a fixed butterfly ----
__device__ inline void seq_wave(const kvae_swf_problem &P) {
  const int T = P.T, lane = (int)(threadIdx.x & 63);
  const int64_t b = blockIdx.x;
  const float *ll = P.ll + b * T;
  float acc = 0.f;
  for (int t = lane; t < T; t += 64) acc += ll[t];   // hidden steps hold 0
  for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
  if (lane == 0) P.seq_ll[b] = acc;
}

// ---- what both entry points (kvae_lgssm_swf.hip, the host simulation below) share --------------------------------------------
inline int swf_check(const kvae_swf_problem *P) {
  if (!P) return KVAE_ERR_NULL;
  if (!P->A || !P->Bm || !P->Q || !P->C || !P->R || !P->P || !P->y || !P->u) return KVAE_ERR_NULL;
  const bool any = P->state_log_w || P->state_mu || P->state_Sigma, all = P->state_log_w && P->state_mu && P->state_Sigma;
  if (!any && (!P->mu0 || !P->Sigma0)) return KVAE_ERR_NULL;
  if (P->seq_ll && !P->ll) return KVAE_ERR_NULL;   // the sequence sums read ll
  if (P->B < 1 || P->T < 1) return KVAE_ERR_DIMS;
  if (P->K < 1 || P->K > MAX_K || P->n < 1 || P->n > MAX_N || P->m < 1 || P->m > MAX_M || P->p != 2) return KVAE_ERR_ARG;
  if (any && !all) return KVAE_ERR_ARG;
  return KVAE_OK;
}
inline bool swf_wants_sweep(const kvae_swf_problem &P) {
  return P.regime_filt || P.regime_pred || P.ll || P.a_pred || P.S_out || P.mus_filt || P.Sigmas_filt || P.levels || P.out_log_w ||
         P.out_mu || P.out_Sigma;
}

}  // namespace kvae_swf

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_switching_filter (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) -----------
// The kernel bodies on emulated wavefronts, with the grids of kvae_lgssm_swf.hip; the launches are counted per body so that tests
// can assert which one ran.  Include this header with KVAE_WAVE_EMU in ONE translation unit per binary.
namespace kvae_swf {
inline int *emu_launches() {
  static int n[2] = {0, 0};   // 0 the sweep, 1 the sequence sums
  return n;
}
}  // namespace kvae_swf

extern "C" int kvae_lgssm_switching_filter(const kvae_swf_problem *prob, void *) {
  using namespace kvae_swf;
  const int rc = swf_check(prob);
  if (rc) return rc;
  const kvae_swf_problem &P = *prob;
  if (swf_wants_sweep(P)) {
    emu_launches()[0] += 1;
    wemu::launch((unsigned)P.B, [&] { sweep_wave<0>(P); });
  }
  if (P.seq_ll) {
    emu_launches()[1] += 1;
    wemu::launch((unsigned)P.B, [&] { seq_wave(P); });
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_switching_filter_launches(int which) { return which == 0 || which == 1 ? kvae_swf::emu_launches()[which] : -1; }
#endif

#if defined(KVAE_WAVE_EMU)
#include "lgssm_sws.h"    // likewise kvae_lgssm_switching_smoother
#endif
