// lgssm_em.h — the E-step of EM for the switching dynamics (include/kvae_lgssm.h kvae_lgssm_switching_em,
// lgssm_ops.switching_em_statistics, KalmanFilter.em_statistics / em_step, kvae.train.em.fit_dynamics_em): the switching Kalman
// smoother's backward pass (csrc/lgssm_sws.h) with the expected sufficient statistics accumulated on the fly.  The equations are
// in the header of the C ABI.  The forward pass is the filter's sweep with its history kept (csrc/lgssm_swf.h, sweep_wave<1>).
//
// back_wave below is composed of the steps kvae_sws::back_wave is composed of (csrc/lgssm_sw_pair.h: so every smoother output
// carries that kernel's bits) on the same 8 x 8 grid - lane = 8 g + k owns the pair (source regime k, destination regime g) - and
// differs in three places:
//   the loop runs one transition further, INTO t = 0: the source belief is (mu0, Sigma0) on every lane, the weights are
//     hist_W[:, 0] (the uniform-matrix step), the input is u_0; nothing is collapsed after it.
//   every transition adds the pair's share xi (.) to the lane's accumulators (N, S11, S10, S00, counts: 80 registers at
//     n = m = 4, each one explicit fmaf per step), and every observed step adds the emission sums from the moment match
//     (m_t, V_t) that mus_smooth / Sigmas_smooth are - the same value on all 64 lanes.
//   after the step into t = 0 the shares are reduced over the source regime (oct_sum, inside a group), z0 / z0z0 over all pairs
//     (wave_sum), and the sequence's row of ws is written, every element once, symmetric blocks mirrored from the upper triangle.
// A second launch (reduce_thread) sums ws over b in ascending order, one thread per element.  No atomics.  Padding lanes hold
// finite values (xi = 0 there) and store nothing; every branch tests kernel arguments and the step counter only; no per-lane array
// is indexed at run time; no LDS, no scratch; the unit is compiled with contraction off.
#pragma once
#include "lgssm_sws.h"

namespace kvae_em {

using kvae::rgrid::oct_sum;
using kvae_sw::wave_sum;

// offsets of the blocks in a row of ws (floats), in the order of kvae_em_stats; G = the row
struct Layout {
  int N, S11, S10, S00, counts, Syz, Szz, Syy, Nobs, z0, z0z0, G;
};
constexpr Layout layout(int K, int n, int m) {   // constexpr: callable from the kernels and from the entry points
  Layout L{};
  const int x = n + m;
  L.N = 0, L.S11 = L.N + K, L.S10 = L.S11 + K * n * n, L.S00 = L.S10 + K * n * x, L.counts = L.S00 + K * x * x;
  L.Syz = L.counts + K * K, L.Szz = L.Syz + 2 * n, L.Syy = L.Szz + n * n, L.Nobs = L.Syy + 4, L.z0 = L.Nobs + 1;
  L.z0z0 = L.z0 + n, L.G = L.z0z0 + n * n;
  return L;
}

__device__ inline void back_wave(const kvae_sws_problem &S, const kvae_em_stats &E) {
  using namespace kvae_sw;
  const kvae_swf_problem &P = S.filt;
  const Lane ln = lane_of(P.K);
  const auto [lane, k, g, kc, gc, vk, vg, ve] = ln;
  const int T = P.T, K = P.K, n = P.n, m = P.m;
  const int64_t b = blockIdx.x, q0 = b * T;
  const int64_t p0 = b * (T > 1 ? T - 1 : 1);   // regime_pairs holds T - 1 steps
  float A[4][4], Bm[4][4], Q[4][4];   // regime g's dynamics, in the filter's orientation
  load_dynamics(P, gc, vg, A, Bm, Q);
  Smoothed Z;      // regime k's smoothed belief of step t, along the lanes
  Transition N;    // the operands of the transition into step t, in flight: the source is the prior at t = 0
  last_belief(S, ln, Z);
  fetch(S, ln, T - 1, true, N);
  // ---- the lane's accumulators: the share of pair (k, g) over t; the emission sums (the same on every lane) ----
  float aN = 0.f, aP = 0.f;
  float a11[4][4], a10z[4][4], a10u[4][4], a00z[4][4], a00zu[4][4], a00u[4][4];   // a11, a00z, a00u: the upper triangle only
  float eyz[2][4], ezz[4][4], eyy[3] = {0.f, 0.f, 0.f}, eno = 0.f;                // ezz: the upper triangle only
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) a11[r][c] = a10z[r][c] = a10u[r][c] = a00z[r][c] = a00zu[r][c] = a00u[r][c] = ezz[r][c] = 0.f;
    eyz[0][r] = eyz[1][r] = 0.f;
  }
  float z0[4] = {0.f, 0.f, 0.f, 0.f}, z0z0[4][4] = {};   // assigned on the step into t = 0, which every T >= 1 reaches

  for (int t = T - 1;; --t) {
    const int64_t q = q0 + t;
    // ---- the outputs of step t, and the emission sums from the moment match (m_t, V_t) ----
    float mm[4], V[4][4];
    step_outputs(S, ln, q, Z, true, mm, V);
    {
      const float mk = P.mask ? P.mask[q] : 1.0f;
      const bool seen = mk != 0.0f;
      const float ob = seen ? 1.0f : 0.0f;   // the weight of the step in the emission sums
      const float y0r = P.y[q * 2], y1r = P.y[q * 2 + 1];
      const float y0 = seen ? y0r : 0.0f, y1 = seen ? y1r : 0.0f;   // selected, not multiplied: whatever a hidden y holds adds 0
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        eyz[0][r] = fmaf(y0, mm[r], eyz[0][r]);
        eyz[1][r] = fmaf(y1, mm[r], eyz[1][r]);
#pragma unroll
        for (int c = r; c < 4; ++c) ezz[r][c] = fmaf(ob, fmaf(mm[r], mm[c], V[r][c]), ezz[r][c]);
      }
      eyy[0] = fmaf(y0, y0, eyy[0]);
      eyy[1] = fmaf(y0, y1, eyy[1]);
      eyy[2] = fmaf(y1, y1, eyy[2]);
      eno += ob;
    }
    // ---- hand-over: lane (k, g) takes regime g's smoothed belief of step t from lane g ("on the groups") ----
    float Mg, mg[4], Sgs[4][4];
    hand_over(g, vg, 0.0f, Z.M, Z.mu, Z.Sigma, Mg, mg, Sgs);
    // ---- the transition into t: its operands, and the next one's in flight ----
    const Transition X = N;
    const float (&u)[4] = X.u;
    fetch(S, ln, t >= 1 ? t - 1 : 0, true, N);
    float mp[4], AS[4][4], Sp[4][4], Jt[4][4], mj[4], Sj[4][4];
    predict(A, Bm, Q, X.mu, X.Sigma, u, mp, AS, Sp);
    smoothed_pair(n, vg, X.mu, X.Sigma, mp, AS, Sp, mg, Sgs, Jt, mj, Sj);
    const float pr = pair_marginal(ve ? X.W : 0.0f, Mg, vg);
    // ---- the pair's share of the statistics of this transition: xi = pr, 0 on the padding lanes ----
    aN += pr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float cr = 0.f;   // (Sigma_s^g J^T)[r][c]: Cov(z_t, z_{t-1}) of the pair
#pragma unroll
        for (int e = 0; e < 4; ++e) cr = fmaf(Sgs[r][e], Jt[e][c], cr);
        a10z[r][c] = fmaf(pr, fmaf(mg[r], mj[c], cr), a10z[r][c]);
        a10u[r][c] = fmaf(pr, mg[r] * u[c], a10u[r][c]);
        a00zu[r][c] = fmaf(pr, mj[r] * u[c], a00zu[r][c]);
        if (c >= r) {
          a11[r][c] = fmaf(pr, fmaf(mg[r], mg[c], Sgs[r][c]), a11[r][c]);
          a00z[r][c] = fmaf(pr, fmaf(mj[r], mj[c], Sj[r][c]), a00z[r][c]);
          a00u[r][c] = fmaf(pr, u[r] * u[c], a00u[r][c]);
        }
      }
    }
    if (t == 0) {
      // ---- the step into t = 0: the smoothed moments of z_{-1}, over all pairs ----
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        z0[r] = wave_sum(pr * mj[r]);
#pragma unroll
        for (int c = r; c < 4; ++c) z0z0[r][c] = wave_sum(pr * fmaf(mj[r], mj[c], Sj[r][c]));
      }
      break;
    }
    aP += pr;
    collapse(S, ln, p0 + t - 1, pr, mj, Sj, Z);
  }
  // ---- the sequence's row: the shares reduced over the source regime, every element of ws[b, :] written once ----
  const Layout Lw = layout(K, n, m);
  float *ws = E.ws + b * (int64_t)Lw.G;
  const int x = n + m;
  const bool lead = vg && k == 0;
  {
    const float v = oct_sum(aN);
    if (lead) ws[Lw.N + gc] = v;
  }
  if (ve) ws[Lw.counts + k * K + g] = aP;
  float *w11 = ws + Lw.S11 + gc * n * n, *w10 = ws + Lw.S10 + gc * n * x, *w00 = ws + Lw.S00 + gc * x * x;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float vz = oct_sum(a10z[r][c]), vu = oct_sum(a10u[r][c]), vzu = oct_sum(a00zu[r][c]);
      if (lead && r < n && c < n) w10[r * x + c] = vz;
      if (lead && r < n && c < m) w10[r * x + n + c] = vu;
      if (lead && r < n && c < m) w00[r * x + n + c] = vzu, w00[(n + c) * x + r] = vzu;
      if (c >= r) {
        const float v1 = oct_sum(a11[r][c]), v0 = oct_sum(a00z[r][c]), vuu = oct_sum(a00u[r][c]);
        if (lead && c < n) w11[r * n + c] = v1, w11[c * n + r] = v1;
        if (lead && c < n) w00[r * x + c] = v0, w00[c * x + r] = v0;
        if (lead && c < m) w00[(n + r) * x + n + c] = vuu, w00[(n + c) * x + n + r] = vuu;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r < n) ws[Lw.Syz + r] = eyz[0][r], ws[Lw.Syz + n + r] = eyz[1][r], ws[Lw.z0 + r] = z0[r];
#pragma unroll
      for (int c = r; c < 4; ++c) {
        if (c < n) {
          ws[Lw.Szz + r * n + c] = ezz[r][c], ws[Lw.Szz + c * n + r] = ezz[r][c];
          ws[Lw.z0z0 + r * n + c] = z0z0[r][c], ws[Lw.z0z0 + c * n + r] = z0z0[r][c];
        }
      }
    }
    ws[Lw.Syy] = eyy[0], ws[Lw.Syy + 1] = eyy[1], ws[Lw.Syy + 2] = eyy[1], ws[Lw.Syy + 3] = eyy[2];
    ws[Lw.Nobs] = eno;
  }
}

// ---- out[e] = sum_b ws[b, e], b ascending: one thread per element of the row, the block picked by the layout; nseq = B ----
__device__ inline void reduce_thread(const kvae_sws_problem &S, const kvae_em_stats &E) {
  const kvae_swf_problem &P = S.filt;
  const Layout L = layout(P.K, P.n, P.m);
  const int e = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  if (e == 0 && E.nseq) E.nseq[0] = (float)P.B;
  kvae_sw::Block k{E.N, L.N};
  offer(k, e, E.S11, L.S11), offer(k, e, E.S10, L.S10), offer(k, e, E.S00, L.S00), offer(k, e, E.counts, L.counts);
  offer(k, e, E.Syz, L.Syz), offer(k, e, E.Szz, L.Szz), offer(k, e, E.Syy, L.Syy), offer(k, e, E.Nobs, L.Nobs);
  offer(k, e, E.z0, L.z0), offer(k, e, E.z0z0, L.z0z0);
  kvae_sw::reduce_rows(E.ws, P.B, L.G, e, k);
}

// ---- what both entry points (kvae_lgssm_em.hip, the host simulation below) share ---------------------------------------------
inline int em_check(const kvae_sws_problem *S, const kvae_em_stats *E) {
  const int rc = kvae_sws::sws_check(S);
  if (rc) return rc;
  if (S->filt.state_log_w || S->filt.state_mu || S->filt.state_Sigma) return KVAE_ERR_ARG;   // the step into t = 0 needs the prior
  if (!E || !E->ws) return KVAE_ERR_NULL;
  return KVAE_OK;
}
inline bool em_wants_stats(const kvae_em_stats &E) {
  return E.N || E.S11 || E.S10 || E.S00 || E.counts || E.Syz || E.Szz || E.Syy || E.Nobs || E.z0 || E.z0z0 || E.nseq;
}
inline unsigned em_reduce_grid(const kvae_sws_problem &S) { return (unsigned)((layout(S.filt.K, S.filt.n, S.filt.m).G + 63) / 64); }
inline int64_t em_ws_floats(int32_t B, int32_t K, int32_t n, int32_t m) {
  return B < 1 || K < 1 || n < 1 || m < 1 ? 0 : (int64_t)B * layout(K, n, m).G;
}

}  // namespace kvae_em

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_switching_em (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) ----------------
// The kernel bodies on emulated wavefronts, with the grids of kvae_lgssm_em.hip; the launches are counted per body.
namespace kvae_em {
inline int *emu_launches() {
  static int n[4] = {0, 0, 0, 0};   // 0 the forward, 1 the backward, 2 the reduction, 3 the sequence sums
  return n;
}
}  // namespace kvae_em

extern "C" int kvae_lgssm_switching_em(const kvae_sws_problem *prob, const kvae_em_stats *st, void *) {
  using namespace kvae_em;
  const int rc = em_check(prob, st);
  if (rc) return rc;
  const kvae_sws_problem &S = *prob;
  const kvae_em_stats &E = *st;
  const bool stats = em_wants_stats(E), back = stats || kvae_sws::sws_wants_back(S);
  if (back || kvae_swf::swf_wants_sweep(S.filt)) {
    emu_launches()[0] += 1;
    const kvae_swf::History H = kvae_sws::sws_history(S);
    wemu::launch((unsigned)S.filt.B, [&] { kvae_swf::sweep_wave<1>(S.filt, H); });
  }
  if (back) {
    emu_launches()[1] += 1;
    wemu::launch((unsigned)S.filt.B, [&] { back_wave(S, E); });
  }
  if (stats) {
    emu_launches()[2] += 1;
    wemu::launch(em_reduce_grid(S), [&] { reduce_thread(S, E); });
  }
  if (S.filt.seq_ll) {
    emu_launches()[3] += 1;
    wemu::launch((unsigned)S.filt.B, [&] { kvae_swf::seq_wave(S.filt); });
  }
  return KVAE_OK;
}
extern "C" int64_t kvae_lgssm_switching_em_ws_floats(int32_t B, int32_t K, int32_t n, int32_t m) { return kvae_em::em_ws_floats(B, K, n, m); }
extern "C" int kvae_wemu_switching_em_launches(int which) { return which >= 0 && which <= 3 ? kvae_em::emu_launches()[which] : -1; }
#endif

#if defined(KVAE_WAVE_EMU)
#include "lgssm_spf.h"    // likewise kvae_lgssm_switching_pf
#endif
