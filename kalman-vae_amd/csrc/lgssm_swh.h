// lgssm_swh.h — multi-horizon forecasts of the generative switching model under GPB2 collapse (include/kvae_lgssm.h
// kvae_lgssm_switching_forecast, lgssm_ops.switching_forecast, KalmanFilter.forecast_regimes, KVAE.forecast_regimes).  The equations
// are in the header of the C ABI; this file is the forecast on a wavefront.  The forward pass is the filter's sweep
// (csrc/lgssm_swf.h, sweep_wave<2>), which keeps what every step hands to the next: the collapsed beliefs (mu^j_t, Sigma^j_t) and
// the log weights log w'_t(j).
//
// One wavefront per (sequence, origin) - the first kernel of the switching family whose parallelism is B T, not B - on the filter's
// 8 x 8 grid: lane = 8 g + k owns the pair (regime i = k at horizon h - 1, regime j = g at horizon h).  A_g, B_g, Q_g, C, R and
// log P[k, g] are loaded once and stay in registers; the origin's belief is loaded "along the lanes" exactly as the sweep loads a
// carried state; y_{t+h}, mask_{t+h} and u_{t+h} are fetched one horizon step ahead from clamped addresses.  A horizon step is the
// filter's hidden step - kvae_sw::predict, kvae_sw::update with gain times 0, kvae_sw::weights with l_ij = 0, the collapse, the
// hand-over: the same statements, so where the filter runs the same step (its own hidden steps) the bits are the same.  The density
// of the target frame is a second kvae_sw::weights over the pair densities - the filter's statement for ll - and feeds nothing else.
// Padding lanes hold finite values and store nothing; every branch tests kernel arguments, the horizon counter or a value every lane
// of the wavefront loaded from the same address; no per-lane array is indexed at run time; no LDS, no scratch, no atomics; every
// multiply-add is an explicit fmaf and the unit is compiled with contraction off, so the bits of an output do not depend on which
// others are requested.
#pragma once
#include "lgssm_swf.h"

namespace kvae_swh {

__device__ inline void forecast_wave(const kvae_swh_problem &F) {
  using namespace kvae_sw;
  const kvae_swf_problem &P = F.filt;
  const Lane ln = lane_of(P.K);
  const int T = P.T, K = P.K, n = P.n, m = P.m, H = F.H, To = T - F.t0;
  const int64_t b = (int64_t)blockIdx.x / To;
  const int o = (int)(blockIdx.x % To), t = F.t0 + o;
  // ---- operands: regime j = g's dynamics, the shared emission, log P[i = k, j = g] ----
  float A[4][4], Bm[4][4], Q[4][4];
  Emission E;
  load_dynamics(P, ln.gc, ln.vg, A, Bm, Q);
  load_emission(P, ln, E);
  // ---- the origin's belief of regime i = k, along the lanes ----
  float mu[4], Sg[4][4], lw;
  {
    const int64_t s = (b * T + t) * K + ln.kc;
    const float lw0 = F.hist_lw[s];
    lw = ln.vk ? lw0 : -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mu[r] = padded(F.hist_mu + s * n, 1, n, 0, r, ln.vk);
#pragma unroll
      for (int c = 0; c < 4; ++c) Sg[r][c] = padded(F.hist_Sigma + s * n * n, n, n, r, c, ln.vk);
    }
  }
  // ---- y, mask, u of step t + 1: the frame from an address clamped to the sequence, u_all holds T + H steps ----
  const int64_t q0 = b * T, v0 = b * ((int64_t)T + H), f0 = ((int64_t)blockIdx.x) * H;
  const float *maskp = P.mask ? P.mask + q0 : P.R;   // always a valid address (the note at mask_addr, csrc/lgssm_fwd.h)
  const int mstep = P.mask ? 1 : 0;
  const int tc = t + 1 < T ? t + 1 : T - 1;
  float yn0 = P.y[(q0 + tc) * 2], yn1 = P.y[(q0 + tc) * 2 + 1], mkn = maskp[tc * mstep], un[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) un[c] = padded(F.u_all + (v0 + t + 1) * m, 1, m, 0, c, true);

  for (int h = 1; h <= H; ++h) {
    const int64_t q = f0 + (h - 1);
    const bool target = t + h < T;                                   // a frame to score
    const bool observed = target && (P.mask ? mkn != 0.0f : true);
    const float y0 = target ? yn0 : 0.0f, y1 = target ? yn1 : 0.0f;
    const float u[4] = {un[0], un[1], un[2], un[3]};
    {   // the next horizon step's, in flight while this one computes
      const int hn = h + 1 <= H ? h + 1 : h;
      const int tn = t + hn < T ? t + hn : T - 1;
      yn0 = P.y[(q0 + tn) * 2], yn1 = P.y[(q0 + tn) * 2 + 1], mkn = maskp[tn * mstep];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = padded(F.u_all + (v0 + t + hn) * m, 1, m, 0, c, true);
    }
    // ---- the filter's hidden step of pair (i, j): predict, forecast, S, the pair density; the gain is multiplied by 0 ----
    float mp[4], AS[4][4], Sp[4][4];
    Update U;   // of Sf, the upper triangle is read
    predict(A, Bm, Q, mu, Sg, u, mp, AS, Sp);
    update(E.C, E.R, mp, Sp, y0, y1, 0.0f, U);
    const float pw = ln.ve ? expf(lw) * E.Pij : 0.0f;
    const float rp = oct_sum(pw);                                    // regime_fore(j), on the groups
    const Weights wt = weights(ln, lw, E.lPij, 0.0f);
    const float lwn = (wt.cmx + logf(wt.se)) - wt.tot;               // log w'(j), on the groups
    const float rf = ln.vg ? expf(lwn) : 0.0f;
    float mc[4], Sc[4][4];
    collapse_pairs(wt.W, U.muf, U.Sf, mc, Sc);
    // ---- the outputs of (origin, horizon) ----
    if (F.regime_fore && ln.vg && ln.k == 0) F.regime_fore[q * K + ln.g] = rp;
    if (F.ll_fore) {   // the density of the target frame: the filter's ll of an observed step
      const Weights wl = weights(ln, lw, E.lPij, observed ? U.tl.ll : 0.0f);
      if (ln.lane == 0) F.ll_fore[q] = observed ? wl.tot : 0.0f;
    }
    if (F.levels_fore) {
      const float lv = wave_max(pw > 0.0f ? (float)U.tl.level : 0.0f);
      if (ln.lane == 0) F.levels_fore[q] = (int32_t)lv;
    }
    forecast_outputs(ln, U, pw, q, F.a_fore, F.S_fore);
    belief_outputs(ln, n, rf, mc, Sc, q, F.mus_fore, F.Sigmas_fore);
    // ---- hand-over: lane (i = k, j = g) takes regime k's belief from group k ----
    hand_over(ln.k << 3, ln.vk, -INFINITY, lwn, mc, Sc, lw, mu, Sg);
  }
}

// ---- what both entry points (kvae_lgssm_swh.hip, the host simulation below) share --------------------------------------------
inline int swh_check(const kvae_swh_problem *F) {
  if (!F) return KVAE_ERR_NULL;
  const int rc = kvae_swf::swf_check(&F->filt);
  if (rc) return rc;
  if (!F->hist_lw || !F->hist_mu || !F->hist_Sigma || !F->u_all) return KVAE_ERR_NULL;
  if (F->H < 1) return KVAE_ERR_DIMS;
  if (F->t0 < 0 || F->t0 >= F->filt.T) return KVAE_ERR_ARG;
  if ((int64_t)F->filt.B * (F->filt.T - F->t0) > (int64_t)INT32_MAX) return KVAE_ERR_ARG;   // grid limit
  return KVAE_OK;
}
inline bool swh_wants_forecast(const kvae_swh_problem &F) {
  return F.regime_fore || F.a_fore || F.S_fore || F.mus_fore || F.Sigmas_fore || F.ll_fore || F.levels_fore;
}
inline kvae_swf::History swh_history(const kvae_swh_problem &F) { return kvae_swf::History{F.hist_mu, F.hist_Sigma, nullptr, nullptr, F.hist_lw}; }
inline unsigned swh_grid(const kvae_swh_problem &F) { return (unsigned)((int64_t)F.filt.B * (F.filt.T - F.t0)); }

}  // namespace kvae_swh

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_switching_forecast (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) ---------
// The kernel bodies on emulated wavefronts, with the grids of kvae_lgssm_swh.hip; the launches are counted per body.
namespace kvae_swh {
inline int *emu_launches() {
  static int n[3] = {0, 0, 0};   // 0 the forward, 1 the forecast, 2 the sequence sums
  return n;
}
}  // namespace kvae_swh

extern "C" int kvae_lgssm_switching_forecast(const kvae_swh_problem *prob, void *) {
  using namespace kvae_swh;
  const int rc = swh_check(prob);
  if (rc) return rc;
  const kvae_swh_problem &F = *prob;
  const bool fore = swh_wants_forecast(F);
  if (fore || kvae_swf::swf_wants_sweep(F.filt)) {
    emu_launches()[0] += 1;
    const kvae_swf::History H = swh_history(F);
    wemu::launch((unsigned)F.filt.B, [&] { kvae_swf::sweep_wave<2>(F.filt, H); });
  }
  if (fore) {
    emu_launches()[1] += 1;
    wemu::launch(swh_grid(F), [&] { forecast_wave(F); });
  }
  if (F.filt.seq_ll) {
    emu_launches()[2] += 1;
    wemu::launch((unsigned)F.filt.B, [&] { kvae_swf::seq_wave(F.filt); });
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_switching_forecast_launches(int which) { return which >= 0 && which <= 2 ? kvae_swh::emu_launches()[which] : -1; }
#endif

#if defined(KVAE_WAVE_EMU)
#include "lgssm_swv.h"    // likewise kvae_lgssm_switching_viterbi
#endif
