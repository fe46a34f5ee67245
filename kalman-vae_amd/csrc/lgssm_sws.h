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
//   per step, on every lane: predict, J^T = Sigma_p^-T (A Sigma) by elimination in natural order without pivoting (Sigma_p is
//     positive definite: Q_k must be; the zero padding of n < 4 gets a unit diagonal, so the padded rows of J^T stay 0), the
//     smoothed pair (mu_s, Sigma_s) from regime g's smoothed belief of step t + 1, which sits "on the groups".
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

using kvae::rdec::xg8;
using kvae::rgrid::oct_sum;
using kvae_swf::padded;

// the upper triangle of a row-major [n, n] matrix padded to 4 x 4, mirrored
__device__ __forceinline__ void load_sym(const float *S, int n, bool live, float (&out)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = r; c < 4; ++c) {
      out[r][c] = padded(S, n, n, r, c, live);
      out[c][r] = out[r][c];
    }
  }
}

// kvae_em::back_wave (csrc/lgssm_em.h, the E-step of EM) is a sibling of this body that repeats its statements in its order and
// must give the bits of its outputs (tests/em_cases.py per_sequence compares them): a change here is made there too.
__device__ inline void back_wave(const kvae_sws_problem &S) {
  const kvae_swf_problem &P = S.filt;
  const int lane = (int)(threadIdx.x & 63), k = lane & 7, g = lane >> 3;
  const int T = P.T, K = P.K, n = P.n, m = P.m;
  const int64_t b = blockIdx.x;
  const bool vk = k < K, vg = g < K, ve = vk && vg;
  const int kc = vk ? k : 0, gc = vg ? g : 0;
  // ---- regime g's dynamics, in the filter's orientation ----
  float A[4][4], Bm[4][4], Q[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      A[r][c] = padded(P.A + gc * n * n, n, n, r, c, vg);
      Bm[r][c] = padded(P.Bm + gc * n * m, n, m, r, c, vg);
      Q[r][c] = padded(P.Q + gc * n * n, n, n, r, c, vg);
    }
  }
  const int64_t q0 = b * T;
  const int64_t p0 = b * (T > 1 ? T - 1 : 1);   // regime_pairs holds T - 1 steps
  // ---- t = T - 1: regime k's filtered belief is its smoothed one, M = the final weights ("along the lanes") ----
  float Mk, ms[4], Ss[4][4];
  {
    const int64_t s = (q0 + T - 1) * K + kc;
    const float w = S.hist_w[b * K + kc];
    Mk = vk ? w : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) ms[r] = padded(S.hist_mu + s * n, 1, n, 0, r, vk);
    load_sym(S.hist_Sigma + s * n * n, n, vk, Ss);
  }
  // ---- the operands of step T - 2, in flight: (mu^k, Sigma^k) of that step, W and u of the step after it ----
  float mun[4], Sgn[4][4], Wn, un[4];
  {
    const int ts = T > 1 ? T - 2 : 0, tw = T > 1 ? T - 1 : 0;
    const int64_t s = (q0 + ts) * K + kc;
#pragma unroll
    for (int r = 0; r < 4; ++r) mun[r] = padded(S.hist_mu + s * n, 1, n, 0, r, vk);
    load_sym(S.hist_Sigma + s * n * n, n, vk, Sgn);
    Wn = S.hist_W[ve ? ((q0 + tw) * K + k) * K + g : 0];
#pragma unroll
    for (int c = 0; c < 4; ++c) un[c] = padded(P.u + (q0 + tw) * m, 1, m, 0, c, true);
  }

  for (int t = T - 1;; --t) {
    const int64_t q = q0 + t;
    // ---- the outputs of step t: M_t, and the moment match of the K smoothed Gaussians under it (inside a group) ----
    if (S.regime_smooth && lane < K) S.regime_smooth[q * K + lane] = Mk;
    if (S.mus_smooth || S.Sigmas_smooth) {
      float mm[4], dd[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mm[r] = oct_sum(Mk * ms[r]);
        dd[r] = ms[r] - mm[r];
        if (S.mus_smooth && lane == 0 && r < n) S.mus_smooth[q * n + r] = mm[r];
      }
      if (S.Sigmas_smooth) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int c = r; c < 4; ++c) {
            const float v = oct_sum(Mk * fmaf(dd[r], dd[c], Ss[r][c]));
            if (lane == 0 && c < n) S.Sigmas_smooth[q * n * n + r * n + c] = v, S.Sigmas_smooth[q * n * n + c * n + r] = v;
          }
        }
      }
    }
    if (t == 0) break;
    // ---- hand-over: lane (k, g) takes regime g's smoothed belief of step t from lane g ("on the groups") ----
    float Mg, mg[4], Sgs[4][4];
    {
      const float v = __shfl(Mk, g, 64);
      Mg = vg ? v : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = __shfl(ms[r], g, 64);
      mg[r] = vg ? v : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = r; c < 4; ++c) {
        const float v = __shfl(Ss[r][c], g, 64);
        Sgs[r][c] = vg ? v : 0.0f;
        Sgs[c][r] = Sgs[r][c];
      }
    }
    // ---- step t - 1: its operands, and the next step's in flight ----
    const float W = ve ? Wn : 0.0f;
    const float u[4] = {un[0], un[1], un[2], un[3]};
    float mu[4], Sg[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mu[r] = mun[r];
#pragma unroll
      for (int c = 0; c < 4; ++c) Sg[r][c] = Sgn[r][c];
    }
    {
      const int ts = t >= 2 ? t - 2 : 0, tw = ts + 1;   // tw <= T - 1: t >= 1 here, so T >= 2
      const int64_t s = (q0 + ts) * K + kc;
#pragma unroll
      for (int r = 0; r < 4; ++r) mun[r] = padded(S.hist_mu + s * n, 1, n, 0, r, vk);
      load_sym(S.hist_Sigma + s * n * n, n, vk, Sgn);
      Wn = S.hist_W[ve ? ((q0 + tw) * K + k) * K + g : 0];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = padded(P.u + (q0 + tw) * m, 1, m, 0, c, true);
    }
    // ---- predict of the pair: the filter's statements (csrc/lgssm_swf.h) ----
    float mp[4], AS[4][4], Sp[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) acc = fmaf(A[r][c], mu[c], acc);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc = fmaf(Bm[r][c], u[c], acc);
      mp[r] = acc;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(A[r][e], Sg[e][c], s);
        AS[r][c] = s;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(AS[r][e], A[c][e], s);
        Sp[r][c] = s + Q[r][c];
      }
    }
    // ---- X = J^T = Sigma_p^-T (A Sigma): elimination in natural order, no pivoting; padding gets a unit diagonal ----
    float L[4][4], X[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        L[r][c] = (r == c && (r >= n || !vg)) ? 1.0f : Sp[c][r];
        X[r][c] = AS[r][c];
      }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const float f = L[r][p] / L[p][p];
#pragma unroll
        for (int c = p + 1; c < 4; ++c) L[r][c] = fmaf(-f, L[p][c], L[r][c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) X[r][c] = fmaf(-f, X[p][c], X[r][c]);
      }
    }
#pragma unroll
    for (int r = 3; r >= 0; --r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = X[r][c];
#pragma unroll
        for (int e = r + 1; e < 4; ++e) s = fmaf(-L[r][e], X[e][c], s);
        X[r][c] = s / L[r][r];
      }
    }
    // ---- the smoothed pair: mu_s = mu + J (mu_s^g - mu_p), Sigma_s = sym(Sigma + J (Sigma_s^g - Sigma_p) J^T) ----
    float dm[4], D[4][4], JD[4][4], mj[4], F[4][4], Sj[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dm[r] = mg[r] - mp[r];
#pragma unroll
      for (int c = 0; c < 4; ++c) D[r][c] = Sgs[r][c] - Sp[r][c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float acc = mu[r];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc = fmaf(X[c][r], dm[c], acc);
      mj[r] = acc;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(X[e][r], D[e][c], s);
        JD[r][c] = s;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = fmaf(JD[r][e], X[e][c], s);
        F[r][c] = Sg[r][c] + s;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = r; c < 4; ++c) Sj[r][c] = 0.5f * (F[r][c] + F[c][r]);   // the upper triangle: the lower has the same bits
    }
    // ---- weights: the pair marginal, M_{t-1}(k) over the groups, V_{g|k} (one-hot at g = k where M_{t-1}(k) = 0) ----
    // A column of the rounded W sums to 1 within a few ulp only, and nearly the same column comes back step after step, so
    // W * M alone lets the total mass of M drift linearly in T (1e-6 over 70 steps).  Dividing M_{t+1}(g) by the column's own sum
    // (1 in exact arithmetic; inside the group, three DPP moves) keeps sum_j pairs_t(j, g) = M_{t+1}(g) to rounding.
    const float cs = oct_sum(W);
    const float pr = W * (Mg / (vg ? cs : 1.0f));
    const float Mn = xg8<0>(pr);
    const bool dead = !(Mn > 0.0f);
    const float V = dead ? (k == g ? 1.0f : 0.0f) : pr / Mn;
    if (S.regime_pairs && ve) S.regime_pairs[((p0 + t - 1) * K + k) * K + g] = pr;
    // ---- collapse over g: regime k's smoothed belief of step t - 1, along the lanes ----
    float d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ms[r] = xg8<0>(V * mj[r]);
      d[r] = mj[r] - ms[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = r; c < 4; ++c) {
        Ss[r][c] = xg8<0>(V * fmaf(d[r], d[c], Sj[r][c]));
        Ss[c][r] = Ss[r][c];
      }
    }
    Mk = Mn;
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
