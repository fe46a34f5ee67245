// lgssm_swm.h — log p(a | u) of the switching model with the regimes summed out under GPB2 collapse, differentiable
// (include/kvae_lgssm.h kvae_lgssm_switching_marginal / kvae_lgssm_switching_marginal_bwd, lgssm_ops.switching_log_marginal,
// KalmanFilter.regime_log_marginal, the "regime_marginal" training objective).  The forward is the filter's sweep
// (csrc/lgssm_swf.h, sweep_wave<2>), which keeps what every step hands to the next: the collapsed beliefs (mu^j_t, Sigma^j_t) and the
// log weights log w'_t(j).  This file is its hand-derived adjoint on a wavefront, and the reduction of the per-sequence partials.
//
// One wavefront per sequence on the filter's 8 x 8 grid, in the filter's orientation: lane = 8 g + k owns the pair (previous regime
// i = k, current regime j = g).  A_j, B_j, Q_j, C, R and log P[i,j] stay in registers for the whole sweep; step t = T-1 .. 0 streams,
// one step ahead from clamped addresses, the belief and log weight that ENTERED it (history slot t - 1; (mu0, Sigma0, log 1/K) at
// t = 0) and y_t, u_t, mask_t, g_ll[b,t].
//   per step, on every lane: the pair step recomputed by the forward's own functions (kvae_sw::predict, update and weights of
//     csrc/lgssm_sw_pair.h: the level, S and W are the forward's bits), then its adjoint - the equations of DESIGN.md section 16.
//   the adjoints that arrive from step t + 1 - of log w'(j), mu'^j, Sigma'^j - sit "on the groups" (regime j = g); the adjoints
//     this step hands on - of log w(i), mu^i, Sigma^i, summed over j by rdec::xg8 - come out "along the lanes" (regime i = k);
//     the hand-over is the transpose of the grid, fifteen __shfl from lane g, as the smoother's backward.
//   reductions over i inside a group: rgrid::oct_sum; over j and over all pairs: rdec::xg8 / swf::wave_sum.
//   parameter gradients: every lane accumulates its own pair's contribution to gA_j, gB_j, gQ_j, gC and g_logP[i,j] over t in
//     registers (57 accumulators); after t = 0 the pairs are reduced (over i for the per-regime blocks, over all pairs for gC)
//     and the sequence's partial is written to ws[b, :], every element once.  A second launch (reduce_thread) sums ws over b in
//     ascending order, one thread per element: no atomics, two calls give the same bits.
// Padding lanes (k >= K or g >= K) hold zero operands, weight 0 and zero adjoints: every value on them is finite, they take every
// branch the live lanes take (all branches test kernel arguments and the step counter only), and they store nothing.  A pair with
// log c = -inf (a zero of P, a dead regime) gets an adjoint of exactly 0 by a select - nothing multiplies an inf.  No per-lane array
// is indexed at run time, no LDS, no scratch; the unit is compiled with contraction off.
#pragma once
#include "lgssm_sws.h"

namespace kvae_swm {

using kvae::rdec::xg8;
using kvae::rgrid::oct_sum;
using kvae_sw::padded;
using kvae_sw::wave_sum;


// ---- the layout of one sequence's partial, ws[b, :], in floats ----
struct Layout {
  int A, B, Q, C, P, mu0, Sigma0, G;   // offsets of the blocks gA | gB | gQ | gC | g_logP | g_mu0 | g_Sigma0, and the row length
};
constexpr Layout layout(int K, int n, int m) {   // constexpr: callable from the kernels and from the entry points
  Layout L{};
  L.A = 0, L.B = L.A + K * n * n, L.Q = L.B + K * n * m, L.C = L.Q + K * n * n, L.P = L.C + 2 * n, L.mu0 = L.P + K * K;
  L.Sigma0 = L.mu0 + n, L.G = L.Sigma0 + n * n;
  return L;
}

// the belief and log weight of regime i = k that ENTER step t: history slot t - 1, or (mu0, Sigma0, log 1/K) at t = 0 - what the
// forward's hand-over (or its first loads) put on this lane, bit for bit
__device__ __forceinline__ void entering(const kvae_swm_problem &M, int64_t q0, int t, int kc, bool vk, float lPuni, float (&mu)[4],
                                         float (&Sg)[4][4], float &lw) {
  const kvae_swf_problem &P = M.filt;
  const int K = P.K, n = P.n;
  const bool init = t == 0;
  const int64_t s = (q0 + (init ? 0 : t - 1)) * K + kc;
  const float *m0 = init ? P.mu0 : M.hist_mu + s * n;
  const float *S0 = init ? P.Sigma0 : M.hist_Sigma + s * n * n;
  const float lwv = M.hist_lw[s];   // a valid address either way
  lw = vk ? (init ? lPuni : lwv) : -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mu[r] = padded(m0, 1, n, 0, r, vk);
#pragma unroll
    for (int c = 0; c < 4; ++c) Sg[r][c] = padded(S0, n, n, r, c, vk);
  }
}

__device__ inline void back_wave(const kvae_swm_problem &M, const kvae_swm_grads &G) {
  const kvae_swf_problem &P = M.filt;
  const kvae_sw::Lane ln = kvae_sw::lane_of(P.K);
  const auto [lane, k, g, kc, gc, vk, vg, ve] = ln;
  const int T = P.T, K = P.K, n = P.n, m = P.m;
  const int64_t b = blockIdx.x;
  // ---- operands of the sweep, as the forward's ----
  float A[4][4], Bm[4][4], Q[4][4];
  kvae_sw::Emission E;
  kvae_sw::load_dynamics(P, gc, vg, A, Bm, Q);
  kvae_sw::load_emission(P, ln, E);
  const float (&C)[2][4] = E.C;
  const float lPuni = E.lPuni;
  const int64_t q0 = b * T;
  const float *maskp = P.mask ? P.mask + q0 : P.R;   // always a valid address
  const int mstep = P.mask ? 1 : 0;
  const float *gllp = G.g_ll ? G.g_ll + q0 : P.R;
  const int gstep = G.g_ll ? 1 : 0;
  const float gseq = G.g_seq ? G.g_seq[b] : 0.0f;
  // ---- the operands of step T - 1, in flight ----
  float mun[4], Sgn[4][4], lwnx, yn0, yn1, mkn, gln, un[4];
  {
    const int t = T - 1;
    entering(M, q0, t, kc, vk, lPuni, mun, Sgn, lwnx);
    yn0 = P.y[(q0 + t) * 2], yn1 = P.y[(q0 + t) * 2 + 1], mkn = maskp[t * mstep], gln = gllp[t * gstep];
#pragma unroll
    for (int c = 0; c < 4; ++c) un[c] = padded(P.u + (q0 + t) * m, 1, m, 0, c, true);
  }
  // ---- the adjoints that arrive from step t + 1, of regime j = g ("on the groups"): none after the last step ----
  float gl = 0.0f, gm[4], GS[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gm[r] = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) GS[r][c] = 0.0f;
  }
  // ---- this pair's share of the parameter gradients ----
  float aA[4][4], aB[4][4], aQ[4][4], aC[2][4], aP = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) aA[r][c] = 0.0f, aB[r][c] = 0.0f, aQ[r][c] = 0.0f;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int c = 0; c < 4; ++c) aC[q][c] = 0.0f;
  }
  float gmu_out[4], gSg_out[4][4];   // of regime i = k, along the lanes: after t = 0 the adjoints of (mu0, Sigma0) per regime

  for (int t = T - 1; t >= 0; --t) {
    const int64_t q = q0 + t;
    const float y0 = yn0, y1 = yn1, mk = P.mask ? mkn : 1.0f, gll = G.g_ll ? gln : 0.0f, lw = lwnx;
    const float u[4] = {un[0], un[1], un[2], un[3]};
    float mu[4], Sg[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mu[r] = mun[r];
#pragma unroll
      for (int c = 0; c < 4; ++c) Sg[r][c] = Sgn[r][c];
    }
    {   // the operands of step t - 1, in flight while this one computes (step 0 fetches itself again)
      const int tn = t > 0 ? t - 1 : 0;
      entering(M, q0, tn, kc, vk, lPuni, mun, Sgn, lwnx);
      yn0 = P.y[(q0 + tn) * 2], yn1 = P.y[(q0 + tn) * 2 + 1], mkn = maskp[tn * mstep], gln = gllp[tn * gstep];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = padded(P.u + (q0 + tn) * m, 1, m, 0, c, true);
    }
    const bool observed = mk != 0.0f, first = t == 0;
    const float om = observed ? gll + gseq : 0.0f;
    // ======== the pair step, recomputed: the functions of kvae_swf::sweep_wave ========
    float mp[4], AS[4][4], Sp[4][4];
    kvae_sw::Update U;
    kvae_sw::predict(A, Bm, Q, mu, Sg, u, mp, AS, Sp);
    kvae_sw::update(C, E.R, mp, Sp, y0, y1, mk, U);
    const float lPt = first ? (ve ? lPuni : -INFINITY) : E.lPij;
    const float lij = observed ? U.tl.ll : 0.0f;
    const kvae_sw::Weights wt = kvae_sw::weights(ln, lw, lPt, lij);
    const float logc = wt.logc, W = wt.W, tot = wt.tot;
    if (G.ll_recomputed && lane == 0) G.ll_recomputed[q] = observed ? tot : 0.0f;   // the forward's P.ll[q], bit for bit
    float d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = U.muf[r] - oct_sum(W * U.muf[r]);
    // ======== the adjoint of the collapse: Sigma'^j = sum_i W (Sigma_ij + d d^T), mu'^j = sum_i W mu_ij ========
    float GSd[4], gmuf[4], Gm[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) s = fmaf(GS[r][c], d[c], s);
      GSd[r] = s;
    }
    // the adjoint of W enters through W (gW - sum_i W gW) only, so anything common to the column may be taken off it: the moments
    // are centred on the collapsed ones (d for mu_ij, Sigma'^j recomputed as the forward forms it).  Uncentred, the common part -
    // large where Sigma_ij is (the first steps under a wide Sigma0) - cancels only in that difference.
    float gW = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gW = fmaf(gm[r], d[r], gW);
#pragma unroll
      for (int c = r; c < 4; ++c) {
        const float e = fmaf(d[r], d[c], U.Sf[r][c]);
        const float dev = e - oct_sum(W * e);
        gW = fmaf(r == c ? GS[r][c] : 2.0f * GS[r][c], dev, gW);
      }
      gmuf[r] = W * fmaf(2.0f, GSd[r], gm[r]);   // the terms through mu'^j inside d cancel: sum_i W d = 0
#pragma unroll
      for (int c = 0; c < 4; ++c) Gm[r][c] = W * GS[r][c];
    }
    // ======== the weights: W = softmax_i log c, log w'(j) = lse_i log c - lse_ij log c, ll = lse_ij log c ========
    const bool livec = ve && logc > -INFINITY;   // a zero of P, a dead regime, a padding lane: exactly 0, selected
    const float sW = oct_sum(W * gW);
    const float sgl = xg8<0>(gl);
    const float pi = livec ? expf(logc - tot) : 0.0f;
    const float glc = livec ? fmaf(om - sgl, pi, W * ((gW - sW) + gl)) : 0.0f;
    const float glw = xg8<0>(glc);               // the adjoint of log w(i), along the lanes
    aP += first ? 0.0f : glc;                    // the uniform-matrix step does not read P
    const float gli = observed ? glc : 0.0f;     // the adjoint of l_ij
    // ======== the pair's Kalman step ========
    const kvae_pred::Adj ad = kvae_pred::pred_adjoint(U.tl, U.S00, U.S11, U.res[0], U.res[1]);
    const float Si11 = 1.0f / U.ed, Si01 = -U.el / U.ed, Si00 = U.S11 / (U.S00 * U.ed);   // S^-1, by the gain's elimination
    float Kb[4][2], KbSi[4][2];   // Kb: the adjoint of Kt;  KbSi = Kb S^-1
#pragma unroll
    for (int r = 0; r < 4; ++r) Kb[r][0] = gmuf[r] * U.res[0], Kb[r][1] = gmuf[r] * U.res[1];
    // K R - M Sigma_p C^T = (mask - 1) Sigma_p C^T, because Kt S = Sigma_p C^T: 0 on an observed step (the gain is the stationary
    // point of the Joseph form).  Formed as written it is the difference of two equal matrices - rounding noise that 2 G amplifies
    // where Sigma_p >> R (the model's Sigma0 = 20 I against R = 0.03^2 I: gA off by 1.4e-5).
    const float mk1 = mk - 1.0f;
    float H[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) H[r][0] = mk1 * U.PCT[r][0], H[r][1] = mk1 * U.PCT[r][1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s0 = fmaf(Gm[r][e], H[e][0], s0), s1 = fmaf(Gm[r][e], H[e][1], s1);
      Kb[r][0] = mk * fmaf(2.0f, s0, Kb[r][0]), Kb[r][1] = mk * fmaf(2.0f, s1, Kb[r][1]);
      KbSi[r][0] = fmaf(Kb[r][1], Si01, Kb[r][0] * Si00), KbSi[r][1] = fmaf(Kb[r][1], Si11, Kb[r][0] * Si01);
    }
    float k00 = 0.f, k01 = 0.f, k10 = 0.f, k11 = 0.f;   // Kt^T Kb S^-1
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      k00 = fmaf(U.Kt[r][0], KbSi[r][0], k00), k01 = fmaf(U.Kt[r][0], KbSi[r][1], k01);
      k10 = fmaf(U.Kt[r][1], KbSi[r][0], k10), k11 = fmaf(U.Kt[r][1], KbSi[r][1], k11);
    }
    const float gS00 = fmaf(gli, ad.g00, -k00), gS11 = fmaf(gli, ad.g11, -k11), gS01 = fmaf(gli, ad.g01, -0.5f * (k01 + k10));
    float gr[2];
    {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) s0 = fmaf(U.Kg[r][0], gmuf[r], s0), s1 = fmaf(U.Kg[r][1], gmuf[r], s1);
      gr[0] = fmaf(-gli, ad.v0, s0), gr[1] = fmaf(-gli, ad.v1, s1);
    }
    float GM[4][4], gSp[4][4], gmp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(Gm[r][e], U.IKC[e][c], s);
        GM[r][c] = s;
      }
      gmp[r] = gmuf[r] - fmaf(C[1][r], gr[1], C[0][r] * gr[0]);
    }
    float Hc[2][4];   // gS C
#pragma unroll
    for (int c = 0; c < 4; ++c) Hc[0][c] = fmaf(gS01, C[1][c], gS00 * C[0][c]), Hc[1][c] = fmaf(gS11, C[1][c], gS01 * C[0][c]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = r; c < 4; ++c) {
        float s = 0.f;   // M^T G M
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(U.IKC[e][r], GM[e][c], s);
        const float ksc = fmaf(KbSi[r][1], C[1][c], KbSi[r][0] * C[0][c]), kcs = fmaf(KbSi[c][1], C[1][r], KbSi[c][0] * C[0][r]);
        s = fmaf(0.5f, ksc + kcs, s);
        s += fmaf(C[1][r], Hc[1][c], C[0][r] * Hc[0][c]);
        gSp[r][c] = s;
        gSp[c][r] = s;
      }
    }
    // ---- the pair's share of gC, gQ_j, gA_j, gB_j ----
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float g0 = 0.f, g1 = 0.f;   // -2 K^T (G M Sigma_p) + (Kb S^-1)^T Sigma_p
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float gms = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) gms = fmaf(GM[r][e], Sp[e][c], gms);
        g0 = fmaf(-2.0f * U.Kg[r][0], gms, g0), g1 = fmaf(-2.0f * U.Kg[r][1], gms, g1);
        g0 = fmaf(KbSi[r][0], Sp[r][c], g0), g1 = fmaf(KbSi[r][1], Sp[r][c], g1);
      }
      g0 = fmaf(2.0f, fmaf(gS01, U.CP[1][c], gS00 * U.CP[0][c]), g0), g1 = fmaf(2.0f, fmaf(gS11, U.CP[1][c], gS01 * U.CP[0][c]), g1);
      aC[0][c] += fmaf(-gr[0], mp[c], g0), aC[1][c] += fmaf(-gr[1], mp[c], g1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(gSp[r][e], AS[e][c], s);
        aA[r][c] += fmaf(2.0f, s, gmp[r] * mu[c]);
        aB[r][c] = fmaf(gmp[r], u[c], aB[r][c]);
        aQ[r][c] += gSp[r][c];
      }
    }
    // ---- the step's gY and gU: over all pairs ----
    if (G.gY) {
      const float g0 = wave_sum(gr[0]), g1 = wave_sum(gr[1]);
      if (lane == 0) G.gY[q * 2] = observed ? g0 : 0.0f, G.gY[q * 2 + 1] = observed ? g1 : 0.0f;
    }
    if (G.gU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) s = fmaf(Bm[r][c], gmp[r], s);
        const float v = wave_sum(s);
        if (lane == 0 && c < m) G.gU[q * m + c] = v;
      }
    }
    // ---- what the step hands on: the adjoints of (mu^i, Sigma^i), summed over j - along the lanes ----
    float AtG[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(A[e][r], gmp[e], s);
      gmu_out[r] = xg8<0>(s);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaf(A[e][r], gSp[e][c], a);
        AtG[r][c] = a;
      }
    }
    float X[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaf(AtG[r][e], A[e][c], a);
        X[r][c] = a;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = r; c < 4; ++c) {
        gSg_out[r][c] = xg8<0>(0.5f * (X[r][c] + X[c][r]));
        gSg_out[c][r] = gSg_out[r][c];
      }
    }
    // ---- hand-over: lane (i = k, j = g) of step t - 1 takes regime g's adjoints from lane g (the transpose of the grid) ----
    kvae_sw::hand_over(g, vg, 0.0f, glw, gmu_out, gSg_out, gl, gm, GS);
  }
  // ---- the sequence's partial: the pairs reduced, every element of ws[b, :] written once ----
  const Layout L = layout(K, n, m);
  float *ws = G.ws + b * (int64_t)L.G;
  const bool lead = vg && k == 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float va = oct_sum(aA[r][c]), vb = oct_sum(aB[r][c]), vq = oct_sum(aQ[r][c]);
      if (lead && r < n && c < n) ws[L.A + (g * n + r) * n + c] = va, ws[L.Q + (g * n + r) * n + c] = vq;
      if (lead && r < n && c < m) ws[L.B + (g * n + r) * m + c] = vb;
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = wave_sum(aC[q][c]);
      if (lane == 0 && c < n) ws[L.C + q * n + c] = v;
    }
  }
  if (ve) ws[L.P + k * K + g] = aP;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float v = oct_sum(gmu_out[r]);   // over the K regimes that all start at (mu0, Sigma0)
    if (lane == 0 && r < n) ws[L.mu0 + r] = v;
#pragma unroll
    for (int c = r; c < 4; ++c) {
      const float s = oct_sum(gSg_out[r][c]);
      if (lane == 0 && c < n) ws[L.Sigma0 + r * n + c] = s, ws[L.Sigma0 + c * n + r] = s;
    }
  }
}

// ---- out[e] = sum_b ws[b, e], b ascending: one thread per element of the partial, the block picked by the layout ----
__device__ inline void reduce_thread(const kvae_swm_problem &M, const kvae_swm_grads &G) {
  const kvae_swf_problem &P = M.filt;
  const Layout L = layout(P.K, P.n, P.m);
  const int e = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  kvae_sw::Block k{G.gA, L.A};
  offer(k, e, G.gB, L.B), offer(k, e, G.gQ, L.Q), offer(k, e, G.gC, L.C), offer(k, e, G.g_logP, L.P);
  offer(k, e, G.g_mu0, L.mu0), offer(k, e, G.g_Sigma0, L.Sigma0);
  kvae_sw::reduce_rows(G.ws, P.B, L.G, e, k);
}

// ---- what both entry points (kvae_lgssm_swm.hip, the host simulation below) share --------------------------------------------
inline int swm_check(const kvae_swm_problem *M) {
  if (!M) return KVAE_ERR_NULL;
  const int rc = kvae_swf::swf_check(&M->filt);
  if (rc) return rc;
  if (M->filt.state_log_w || M->filt.state_mu || M->filt.state_Sigma) return KVAE_ERR_ARG;   // no gradient through a carried state
  if (!M->hist_lw || !M->hist_mu || !M->hist_Sigma) return KVAE_ERR_NULL;
  return KVAE_OK;
}
inline int swm_bwd_check(const kvae_swm_problem *M, const kvae_swm_grads *G) {
  const int rc = swm_check(M);
  if (rc) return rc;
  if (!G || (!G->g_ll && !G->g_seq) || !G->ws) return KVAE_ERR_NULL;
  return KVAE_OK;
}
inline bool swm_wants_params(const kvae_swm_grads &G) { return G.gA || G.gB || G.gQ || G.gC || G.g_logP || G.g_mu0 || G.g_Sigma0; }
inline bool swm_wants_back(const kvae_swm_grads &G) { return swm_wants_params(G) || G.gY || G.gU || G.ll_recomputed; }
inline kvae_swf::History swm_history(const kvae_swm_problem &M) { return kvae_swf::History{M.hist_mu, M.hist_Sigma, nullptr, nullptr, M.hist_lw}; }
inline unsigned swm_reduce_grid(const kvae_swm_problem &M) { return (unsigned)((layout(M.filt.K, M.filt.n, M.filt.m).G + 63) / 64); }

}  // namespace kvae_swm

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's entry points (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) --------------------------
// The kernel bodies on emulated wavefronts, with the grids of kvae_lgssm_swm.hip; the launches are counted per body.
namespace kvae_swm {
inline int *emu_launches() {
  static int n[4] = {0, 0, 0, 0};   // 0 the forward, 1 the sequence sums, 2 the backward, 3 the reduction
  return n;
}
}  // namespace kvae_swm

extern "C" int kvae_lgssm_switching_marginal(const kvae_swm_problem *prob, void *) {
  using namespace kvae_swm;
  const int rc = swm_check(prob);
  if (rc) return rc;
  const kvae_swm_problem &M = *prob;
  emu_launches()[0] += 1;
  const kvae_swf::History H = swm_history(M);
  wemu::launch((unsigned)M.filt.B, [&] { kvae_swf::sweep_wave<2>(M.filt, H); });
  if (M.filt.seq_ll) {
    emu_launches()[1] += 1;
    wemu::launch((unsigned)M.filt.B, [&] { kvae_swf::seq_wave(M.filt); });
  }
  return KVAE_OK;
}
extern "C" int kvae_lgssm_switching_marginal_bwd(const kvae_swm_problem *prob, const kvae_swm_grads *g, void *) {
  using namespace kvae_swm;
  const int rc = swm_bwd_check(prob, g);
  if (rc) return rc;
  const kvae_swm_problem &M = *prob;
  const kvae_swm_grads &G = *g;
  if (!swm_wants_back(G)) return KVAE_OK;
  emu_launches()[2] += 1;
  wemu::launch((unsigned)M.filt.B, [&] { back_wave(M, G); });
  if (swm_wants_params(G)) {
    emu_launches()[3] += 1;
    wemu::launch(swm_reduce_grid(M), [&] { reduce_thread(M, G); });
  }
  return KVAE_OK;
}
extern "C" int64_t kvae_lgssm_switching_marginal_ws_floats(int32_t B, int32_t K, int32_t n, int32_t m) {
  return B < 1 || K < 1 || n < 1 || m < 1 ? 0 : (int64_t)B * kvae_swm::layout(K, n, m).G;
}
extern "C" int kvae_wemu_switching_marginal_launches(int which) { return which >= 0 && which <= 3 ? kvae_swm::emu_launches()[which] : -1; }

#include "lgssm_em.h"     // likewise kvae_lgssm_switching_em
#endif
