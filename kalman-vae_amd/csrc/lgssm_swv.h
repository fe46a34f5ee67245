// lgssm_swv.h — the approximate Viterbi decoder of the generative switching model (Pavlovic, Rehg & MacCormick 2000;
// include/kvae_lgssm.h kvae_lgssm_switching_viterbi, lgssm_ops.switching_viterbi, KalmanFilter.viterbi_regimes,
// KVAE.viterbi_regimes).  The equations are in the header of the C ABI; this file is their layout on a wavefront.
//
// One wavefront per sequence on the filter's 8 x 8 grid (csrc/lgssm_swf.h): lane = 8 g + k owns the pair (previous regime i = k,
// current regime j = g).  A_g, B_g, Q_g, C, R and log P[k, g] are loaded once and stay in registers for the whole sweep; y_t, u_t,
// mask_t are streamed one step ahead from a clamped address.  Carried "along the lanes": the score J(k) of the survivor path that
// ends in regime k and its exact Kalman belief.
//   per step, on every lane: the filter's pair step - kvae_sw::predict and kvae_sw::update, the same statements; the pair density
//     from their nis and Cholesky factor with range-reduced logarithms (log_reduced below) - and c = (J(k) + log P[k, g]) + l_kg.
//   inside a column (the eight lanes of group g, three DPP moves each): the maximum J'(g) (rgrid::oct_max), the lowest lane that
//     attains it (rgrid::oct_min, as rdec::log_soft finds its `first`) and the SELECTION of that lane's belief: an OR of the bit
//     patterns with the other lanes zeroed (rdec::oct_or), fourteen of them - a copy, so a -0.0 stays -0.0 and no rounding enters.
//     Every lane of the group ends with the same bits ("on the groups").
//   hand-over: kvae_sw::hand_over, the transpose of the grid, and one more __shfl for the back-pointer, which puts the K
//     back-pointers of the step along the lanes: one more OR packs them, 4 bits per target, into the word lane 0 stores.
//   after the sweep: the maximum over j and its lowest arg max over the groups (rdec::xg8), a fence, and the same wavefront walks
//     the words back (rdec::walk_back, regime_decode.h's scheme) and gathers the survivor beliefs of (t, path_t) from the workspace.
// Padding lanes (k >= K or g >= K) hold zero operands and c = -inf: every belief on them is finite, they take every branch the
// live lanes take (all branches test kernel arguments, the step counter or a wave-uniform trip count), and they store nothing.  No
// per-lane array is indexed at run time, no LDS, no scratch, no atomics.  Every multiply-add is an explicit fmaf and the unit is
// compiled with contraction off; the sweep computes everything whatever is asked for, so the bits of an output do not depend on
// which others are requested.
#pragma once
#include "lgssm_swf.h"

namespace kvae_swv {

using kvae::rdec::bitsf;
using kvae::rdec::fbits;
using kvae::rdec::oct_or;
using kvae::rdec::xg8;
using kvae::rgrid::oct_max;
using kvae::rgrid::oct_min;

// the operands as the filter's problem: what kvae_sw::load_dynamics / load_emission and kvae_swf::swf_check read (constexpr: callable
// from the kernel and from the entry point alike)
constexpr kvae_swf_problem operands(const kvae_swv_problem &V) {
  kvae_swf_problem P{};
  P.B = V.B, P.T = V.T, P.K = V.K, P.n = V.n, P.m = V.m, P.p = V.p;
  P.A = V.A, P.Bm = V.Bm, P.Q = V.Q, P.C = V.C, P.R = V.R, P.P = V.P, P.mu0 = V.mu0, P.Sigma0 = V.Sigma0, P.y = V.y, P.u = V.u, P.mask = V.mask;
  P.state_log_w = V.state_score, P.state_mu = V.state_mu, P.state_Sigma = V.state_Sigma;
  return P;
}

// log x of a finite x > 0 by range reduction: x = m 2^e with m in [sqrt(1/2), sqrt(2)), log x = e ln 2 + log m, ln 2 split so that
// e times its head is exact.  The device's logf is log2 x - good to one ulp of ITS magnitude - times ln 2: for the Cholesky factors
// of S met here, |log2 x| in [4, 8), that is up to 3.3e-7 per logarithm, measured one-sided on gfx950; a score is a sum over T
// steps of two of them, so the error of path_log_joint would grow linearly in T.  With |log2 m| <= 1/2 it is below 3e-8.  (Selects,
// no branch.)
__device__ __forceinline__ float log_reduced(float x) {
  int e;
  const float m0 = frexpf(x, &e);                    // m0 in [1/2, 1)
  const bool low = m0 < 0.70710678f;
  const float m = low ? m0 + m0 : m0, fe = (float)(low ? e - 1 : e);
  return fmaf(fe, 0.693145751953125f, fmaf(fe, 1.42860682e-6f, logf(m)));
}

// the value of the lane of the group where sel holds (exactly one lane of every group), on the groups: its bits, untouched
__device__ __forceinline__ float pick(bool sel, float x) { return bitsf(oct_or(sel ? fbits(x) : 0u)); }

__device__ inline void viterbi_wave(const kvae_swv_problem &V) {
  const kvae_swf_problem P = operands(V);
  const kvae_sw::Lane ln = kvae_sw::lane_of(P.K);
  const auto [lane, k, g, kc, gc, vk, vg, ve] = ln;
  const int T = P.T, K = P.K, n = P.n, m = P.m;
  const int64_t b = blockIdx.x;
  // ---- operands of the sweep: regime j = g's dynamics, the shared emission, log P[i = k, j = g] ----
  float A[4][4], Bm[4][4], Q[4][4];
  kvae_sw::Emission E;
  kvae_sw::load_dynamics(P, gc, vg, A, Bm, Q);
  kvae_sw::load_emission(P, ln, E);
  // ---- the survivor that ends in regime i = k ("along the lanes"): its score and belief ----
  const bool carried = V.state_score != nullptr;
  float mu[4], Sg[4][4], J;
  {
    const float *m0 = carried ? V.state_mu + (b * K + kc) * n : P.mu0;
    const float *S0 = carried ? V.state_Sigma + (b * K + kc) * n * n : P.Sigma0;
    const float *j0 = carried ? V.state_score + b * K + kc : P.R;   // a valid address either way
    const float J0 = *j0;
    J = vk ? (carried ? J0 : 0.0f) : -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mu[r] = kvae_sw::padded(m0, 1, n, 0, r, vk);
#pragma unroll
      for (int c = 0; c < 4; ++c) Sg[r][c] = kvae_sw::padded(S0, n, n, r, c, vk);
    }
  }
  // ---- y_0, u_0, mask_0 ----
  const int64_t q0 = b * T;
  const float *maskp = P.mask ? P.mask + q0 : P.R;   // always a valid address (the note at mask_addr, csrc/lgssm_fwd.h)
  const int mstep = P.mask ? 1 : 0;
  float yn0 = P.y[q0 * 2], yn1 = P.y[q0 * 2 + 1], mkn = maskp[0], un[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) un[c] = kvae_sw::padded(P.u + q0 * m, 1, m, 0, c, true);
  const bool lead = vg && k == 0;   // one lane per live group stores what sits on the groups
  float Jn = -INFINITY;             // J'(g) of the last step, on the groups

  for (int t = 0; t < T; ++t) {
    const int64_t q = q0 + t;
    const float y0 = yn0, y1 = yn1, mk = P.mask ? mkn : 1.0f;
    const float u[4] = {un[0], un[1], un[2], un[3]};
    {   // the next step's, in flight while this one computes
      const int tn = t + 1 < T ? t + 1 : t;
      const int64_t qn = q0 + tn;
      yn0 = P.y[qn * 2], yn1 = P.y[qn * 2 + 1], mkn = maskp[tn * mstep];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = kvae_sw::padded(P.u + qn * m, 1, m, 0, c, true);
    }
    const bool observed = mk != 0.0f, first = t == 0 && !carried;
    // ---- the Kalman step of pair (i, j): the filter's ----
    float mp[4], AS[4][4], Sp[4][4];
    kvae_sw::Update U;   // of Sf, the upper triangle is read
    kvae_sw::predict(A, Bm, Q, mu, Sg, u, mp, AS, Sp);
    kvae_sw::update(E.C, E.R, mp, Sp, y0, y1, mk, U);
    // ---- the column: its maximum, the lowest i that attains it (j itself in a column without a finite entry) ----
    const float lPt = first ? (ve ? E.lPuni : -INFINITY) : E.lPij;
    // the pair density: pred_tail's statement over its own nis and factor, the two logarithms by log_reduced (see there)
    const float logdet = 2.0f * (log_reduced(U.tl.l00) + log_reduced(U.tl.l11));
    const float lij = observed ? -0.5f * ((U.tl.nis + logdet) + 2.0f * kvae_pred::LOG_2PI) : 0.0f;
    const float prior = ve ? J + lPt : -INFINITY;
    const float c = ve ? prior + lij : -INFINITY;
    Jn = oct_max(c);
    const bool dead = !(Jn > -INFINITY);
    const float hit = oct_min((ve && c == Jn) ? (float)k : 99.0f);
    const int arg = (dead || hit > 7.5f) ? g : (int)hit;   // (no hit: a NaN in the data; the index stays inside the column)
    const bool sel = k == arg;
    // ---- the survivor of regime j = g: the selected pair's belief, bit for bit, on the groups ----
    float mc[4], Sc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mc[r] = pick(sel, U.muf[r]);
#pragma unroll
      for (int cc = r; cc < 4; ++cc) Sc[r][cc] = pick(sel, U.Sf[r][cc]);
    }
    // ---- the step's outputs ----
    if (V.scores && lead) V.scores[q * K + g] = Jn;
    if (V.backptr && lead) V.backptr[q * K + g] = arg;
    if (V.levels) {
      const float lv = kvae_sw::wave_max(prior > -INFINITY ? (float)U.tl.level : 0.0f);
      if (lane == 0) V.levels[q] = (int32_t)lv;
    }
    if (V.ws_mu && V.mus_filt) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (lead && r < n) V.ws_mu[(q * K + g) * n + r] = mc[r];
    }
    if (V.ws_Sigma && V.Sigmas_filt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int cc = r; cc < 4; ++cc)
          if (lead && cc < n) V.ws_Sigma[((q * K + g) * n + r) * n + cc] = Sc[r][cc], V.ws_Sigma[((q * K + g) * n + cc) * n + r] = Sc[r][cc];
      }
    }
    if (t == T - 1) {   // the carried state out: regime j = g, one lane per group
      const int64_t s = b * K + g;
      if (V.out_score && lead) V.out_score[s] = Jn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (V.out_mu && lead && r < n) V.out_mu[s * n + r] = mc[r];
#pragma unroll
        for (int cc = r; cc < 4; ++cc)
          if (V.out_Sigma && lead && cc < n) V.out_Sigma[(s * n + r) * n + cc] = Sc[r][cc], V.out_Sigma[(s * n + cc) * n + r] = Sc[r][cc];
      }
    }
    // ---- hand-over: lane (i = k, j = g) takes regime k's survivor from group k; the back-pointers likewise, packed into a word ----
    {
      const int argk = (int)fbits(__shfl(bitsf((uint32_t)arg), k << 3, 64));
      const uint32_t word = oct_or(vk ? (uint32_t)argk << (4 * k) : 0u);
      if (V.ws_bp && lane == 0) V.ws_bp[q] = word;
    }
    kvae_sw::hand_over(k << 3, vk, -INFINITY, Jn, mc, Sc, J, mu, Sg);
  }
  // ---- the end of the path: the maximum over j and the lowest j that attains it, over the groups ----
  const float best = xg8<1>(vg ? Jn : -INFINITY);
  const float last = xg8<2>((vg && Jn == best) ? (float)g : 99.0f);
  const int st = last > 7.5f ? 0 : (int)last;
  if (V.path_log_joint && lane == 0) V.path_log_joint[b] = best;
  if (!(V.path || V.mus_filt || V.Sigmas_filt)) return;
  KV_DECODE_FENCE();   // the words lane 0 stored and the beliefs the group leaders stored, visible to the loads of every lane below
  kvae::rdec::walk_back(V.ws_bp + q0, T, st, lane, [&](int tl, int mine) {
    const int64_t q = q0 + tl, s = q * K + mine;
    if (V.path) V.path[q] = mine;
    if (V.mus_filt) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < n) V.mus_filt[q * n + r] = V.ws_mu[s * n + r];
    }
    if (V.Sigmas_filt) {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < n * n) V.Sigmas_filt[q * n * n + e] = V.ws_Sigma[s * n * n + e];
    }
  });
}

// ---- what both entry points (kvae_lgssm_swv.hip, the host simulation below) share --------------------------------------------
inline int swv_check(const kvae_swv_problem *V) {
  if (!V) return KVAE_ERR_NULL;
  const kvae_swf_problem P = operands(*V);
  const int rc = kvae_swf::swf_check(&P);
  if (rc) return rc;
  if ((V->path || V->mus_filt || V->Sigmas_filt) && !V->ws_bp) return KVAE_ERR_NULL;
  if ((V->mus_filt && !V->ws_mu) || (V->Sigmas_filt && !V->ws_Sigma)) return KVAE_ERR_NULL;
  return KVAE_OK;
}
inline bool swv_wants_sweep(const kvae_swv_problem &V) {
  return V.path || V.path_log_joint || V.scores || V.backptr || V.mus_filt || V.Sigmas_filt || V.levels || V.out_score || V.out_mu || V.out_Sigma;
}

}  // namespace kvae_swv

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_switching_viterbi (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) ----------
// The kernel body on emulated wavefronts, with the grid of kvae_lgssm_swv.hip; the launches are counted per body.
namespace kvae_swv {
inline int *emu_launches() {
  static int n[1] = {0};   // 0 the sweep with its backtrace
  return n;
}
}  // namespace kvae_swv

extern "C" int kvae_lgssm_switching_viterbi(const kvae_swv_problem *prob, void *) {
  using namespace kvae_swv;
  const int rc = swv_check(prob);
  if (rc) return rc;
  const kvae_swv_problem &V = *prob;
  if (swv_wants_sweep(V)) {
    emu_launches()[0] += 1;
    wemu::launch((unsigned)V.B, [&] { viterbi_wave(V); });
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_switching_viterbi_launches(int which) { return which == 0 ? kvae_swv::emu_launches()[0] : -1; }
#endif
