// lgssm_sws.h — the switching Kalman smoother with GPB2 collapse (Murphy 1998) over the generative switching model
// (include/kvae_lgssm.h kvae_lgssm_switching_smoother, lgssm_ops.switching_smoother, KalmanFilter.smooth_regimes,
// KVAE.smooth_regimes).  The equations are in the header of the C ABI; this file is the backward pass on a wavefront.  The forward
// pass is the filter's sweep (csrc/lgssm_swf.h, sweep_wave<1>), which keeps the collapsed beliefs (mu^j_t, Sigma^j_t), the pair
// weights W_t and the final weights w_{T-1}.
//
// One wavefront per sequence on the filter's 8 x 8 grid: lane = 8 g + k owns the pair (regime j = k at step t, regime g at step
// t + 1).  A_g, B_g, Q_g sit in registers in the filter's orientation, so the predict of the pair is the filter's own statements on
// the filter's own operands: mu_p, Sigma_p carry the bits the filter had at step t + 1.  (mu^k_t, Sigma^k_t), W_{t+1}[k,g] and
// u_{t+1} are streamed one step ahead from clamped addresses.
//   per step, on every lane: predict (kvae_sw::predict, the filter's), then the smoothed pair (mu_s, Sigma_s) from regime g's
//     smoothed belief of step t + 1, which sits "on the groups" (kvae_sw::smoothed_pair: Sigma_p is positive definite, Q_k must
//     be).  The steps are the functions of csrc/lgssm_sw_pair.h, which the E-step of EM (csrc/lgssm_em.h) is composed of as well.
//   reductions over g (the eight groups, rdec::xg8): M_t(k) and the fourteen sums of the collapse.  Every group ends with the same
//     bits: regime k's smoothed belief of step t "along the lanes".
//   reductions over k inside a group (rgrid::oct_sum): the column sum of W_{t+1}, which M_{t+1}(g) is divided by, and the moment
//     match of the K smoothed Gaussians under M_t.
//   hand-over: lane (k, g) of the next step needs regime g's belief, which lane g holds: fifteen __shfl - the transpose of the grid.
// Padding lanes hold finite values (zero beliefs, zero weights, Sigma_p = I) and store nothing; every branch tests kernel arguments
// (and the step counter) only; no per-lane array is indexed at run time; no LDS, no scratch; every multiply-add is an explicit
// fmaf and the unit is compiled with contraction off, so the bits of an output do not depend on which others are requested.
#pragma once
#include "lgssm_swf.h"

namespace kvae_sws {

__device__ inline void back_wave(const kvae_sws_problem &S) {
  using namespace kvae_sw;
  const kvae_swf_problem &P = S.filt;
  const Lane ln = lane_of(P.K);
  const int T = P.T;
  const int64_t q0 = (int64_t)blockIdx.x * T;
  const int64_t p0 = (int64_t)blockIdx.x * (T > 1 ? T - 1 : 1);   // regime_pairs holds T - 1 steps
  float A[4][4], Bm[4][4], Q[4][4];   // regime g's dynamics, in the filter's orientation
  load_dynamics(P, ln.gc, ln.vg, A, Bm, Q);
  Smoothed Z;      // regime k's smoothed belief of step t, along the lanes
  Transition N;    // the operands of the transition into step t, in flight
  last_belief(S, ln, Z);
  fetch(S, ln, T - 1, false, N);

  for (int t = T - 1;; --t) {
    float mm[4], V[4][4];
    step_outputs(S, ln, q0 + t, Z, false, mm, V);
    if (t == 0) break;
    // ---- hand-over: lane (k, g) takes regime g's smoothed belief of step t from lane g ("on the groups") ----
    float Mg, mg[4], Sgs[4][4];
    hand_over(ln.g, ln.vg, 0.0f, Z.M, Z.mu, Z.Sigma, Mg, mg, Sgs);
    // ---- the transition into step t: its operands, and the next one's in flight ----
    const Transition X = N;
    fetch(S, ln, t - 1, false, N);
    float mp[4], AS[4][4], Sp[4][4], Jt[4][4], mj[4], Sj[4][4];
    predict(A, Bm, Q, X.mu, X.Sigma, X.u, mp, AS, Sp);
    smoothed_pair(P.n, ln.vg, X.mu, X.Sigma, mp, AS, Sp, mg, Sgs, Jt, mj, Sj);
    const float pr = pair_marginal(ln.ve ? X.W : 0.0f, Mg, ln.vg);
    collapse(S, ln, p0 + t - 1, pr, mj, Sj, Z);
  }
}

// ---- what both entry points (kvae_lgssm_sws.hip, the host simulation below) share --------------------------------------------
inline int sws_check(const kvae_sws_problem *S) {
  if (!S) return KVAE_ERR_NULL;
  const int rc = kvae_swf::swf_check(&S->filt);
  if (rc) return rc;
  if (!S->hist_mu || !S->hist_Sigma || !S->hist_W || !S->hist_w) return KVAE_ERR_NULL;
  return KVAE_OK;
}
inline bool sws_wants_back(const kvae_sws_problem &S) { return S.regime_smooth || S.regime_pairs || S.mus_smooth || S.Sigmas_smooth; }
inline kvae_swf::History sws_history(const kvae_sws_problem &S) { return kvae_swf::History{S.hist_mu, S.hist_Sigma, S.hist_W, S.hist_w, nullptr}; }

}  // namespace kvae_sws

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_switching_smoother (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) ---------
// The kernel bodies on emulated wavefronts, with the grids of kvae_lgssm_sws.hip; the launches are counted per body.
namespace kvae_sws {
inline int *emu_launches() {
  static int n[3] = {0, 0, 0};   // 0 the forward, 1 the backward, 2 the sequence sums
  return n;
}
}  // namespace kvae_sws

extern "C" int kvae_lgssm_switching_smoother(const kvae_sws_problem *prob, void *) {
  using namespace kvae_sws;
  const int rc = sws_check(prob);
  if (rc) return rc;
  const kvae_sws_problem &S = *prob;
  const bool back = sws_wants_back(S);
  if (back || kvae_swf::swf_wants_sweep(S.filt)) {
    emu_launches()[0] += 1;
    const kvae_swf::History H = sws_history(S);
    wemu::launch((unsigned)S.filt.B, [&] { kvae_swf::sweep_wave<1>(S.filt, H); });
  }
  if (back) {
    emu_launches()[1] += 1;
    wemu::launch((unsigned)S.filt.B, [&] { back_wave(S); });
  }
  if (S.filt.seq_ll) {
    emu_launches()[2] += 1;
    wemu::launch((unsigned)S.filt.B, [&] { kvae_swf::seq_wave(S.filt); });
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_switching_smoother_launches(int which) { return which >= 0 && which <= 2 ? kvae_sws::emu_launches()[which] : -1; }

#include "lgssm_swm.h"    // likewise kvae_lgssm_switching_marginal and its adjoint
#endif
