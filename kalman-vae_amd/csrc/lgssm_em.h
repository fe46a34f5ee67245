// lgssm_em.h — the E-step of EM for the switching dynamics (include/kvae_lgssm.h kvae_lgssm_switching_em,
// lgssm_ops.switching_em_statistics, KalmanFilter.em_statistics / em_step, kvae.train.em.fit_dynamics_em): the switching Kalman
// smoother's backward pass (csrc/lgssm_sws.h) with the expected sufficient statistics accumulated on the fly.  The equations are
// in the header of the C ABI.  The forward pass is the filter's sweep with its history kept (csrc/lgssm_swf.h, sweep_wave<1>).
//
// back_wave below is a SIBLING of kvae_sws::back_wave: it repeats that body's statements in that body's order (so every smoother
// output carries that kernel's bits; the tests compare them) on the same 8 x 8 grid - lane = 8 g + k owns the pair (source regime
// k, destination regime g) - and differs in three places:
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

using kvae::rdec::xg8;
using kvae::rgrid::oct_sum;
using kvae_swf::padded;
using kvae_swf::wave_sum;
using kvae_sws::load_sym;

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
  // ---- the operands of the transition into T - 1, in flight: the source belief (step T - 2; the prior at T = 1), W and u of T - 1 ----
  float mun[4], Sgn[4][4], Wn, un[4];
  {
    const bool pri = T == 1;
    const int64_t s = (q0 + (pri ? 0 : T - 2)) * K + kc;
    const float *pm = pri ? P.mu0 : S.hist_mu + s * n, *pS = pri ? P.Sigma0 : S.hist_Sigma + s * n * n;
#pragma unroll
    for (int r = 0; r < 4; ++r) mun[r] = padded(pm, 1, n, 0, r, vk);
    load_sym(pS, n, vk, Sgn);
    Wn = S.hist_W[ve ? ((q0 + T - 1) * K + k) * K + g : 0];
#pragma unroll
    for (int c = 0; c < 4; ++c) un[c] = padded(P.u + (q0 + T - 1) * m, 1, m, 0, c, true);
  }
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
    // ---- the outputs of step t: M_t, and the moment match of the K smoothed Gaussians under it (inside a group) ----
    if (S.regime_smooth && lane < K) S.regime_smooth[q * K + lane] = Mk;
    {
      const float mk = P.mask ? P.mask[q] : 1.0f;
      const bool seen = mk != 0.0f;
      const float ob = seen ? 1.0f : 0.0f;   // the weight of the step in the emission sums
      const float y0r = P.y[q * 2], y1r = P.y[q * 2 + 1];
      const float y0 = seen ? y0r : 0.0f, y1 = seen ? y1r : 0.0f;   // selected, not multiplied: whatever a hidden y holds adds 0
      float mm[4], dd[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mm[r] = oct_sum(Mk * ms[r]);
        dd[r] = ms[r] - mm[r];
        if (S.mus_smooth && lane == 0 && r < n) S.mus_smooth[q * n + r] = mm[r];
        eyz[0][r] = fmaf(y0, mm[r], eyz[0][r]);
        eyz[1][r] = fmaf(y1, mm[r], eyz[1][r]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = r; c < 4; ++c) {
          const float v = oct_sum(Mk * fmaf(dd[r], dd[c], Ss[r][c]));
          if (S.Sigmas_smooth && lane == 0 && c < n) S.Sigmas_smooth[q * n * n + r * n + c] = v, S.Sigmas_smooth[q * n * n + c * n + r] = v;
          ezz[r][c] = fmaf(ob, fmaf(mm[r], mm[c], v), ezz[r][c]);
        }
      }
      eyy[0] = fmaf(y0, y0, eyy[0]);
      eyy[1] = fmaf(y0, y1, eyy[1]);
      eyy[2] = fmaf(y1, y1, eyy[2]);
      eno += ob;
    }
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
    // ---- the transition into t: its operands, and the next one's in flight ----
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
      const int tn = t >= 1 ? t - 1 : 0;   // the transition into tn: source step tn - 1, the prior at tn = 0
      const bool pri = tn == 0;
      const int64_t s = (q0 + (pri ? 0 : tn - 1)) * K + kc;
      const float *pm = pri ? P.mu0 : S.hist_mu + s * n, *pS = pri ? P.Sigma0 : S.hist_Sigma + s * n * n;
#pragma unroll
      for (int r = 0; r < 4; ++r) mun[r] = padded(pm, 1, n, 0, r, vk);
      load_sym(pS, n, vk, Sgn);
      Wn = S.hist_W[ve ? ((q0 + tn) * K + k) * K + g : 0];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = padded(P.u + (q0 + tn) * m, 1, m, 0, c, true);
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
    // ---- weights: the pair marginal xi (the column-sum division: the note in csrc/lgssm_sws.h) ----
    const float cs = oct_sum(W);
    const float pr = W * (Mg / (vg ? cs : 1.0f));
    // ---- the pair's share of the statistics of this transition: xi = pr, 0 on the padding lanes ----
    aN += pr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float cr = 0.f;   // (Sigma_s^g J^T)[r][c]: Cov(z_t, z_{t-1}) of the pair
#pragma unroll
        for (int e = 0; e < 4; ++e) cr = fmaf(Sgs[r][e], X[e][c], cr);
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
    // ---- M_{t-1}(k) over the groups, V_{g|k} (one-hot at g = k where M_{t-1}(k) = 0) ----
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
  if (e >= L.G) return;
  if (e == 0 && E.nseq) E.nseq[0] = (float)P.B;
  float *out = e < L.S11 ? E.N : e < L.S10 ? E.S11 : e < L.S00 ? E.S10 : e < L.counts ? E.S00 : e < L.Syz ? E.counts : e < L.Szz ? E.Syz
             : e < L.Syy ? E.Szz : e < L.Nobs ? E.Syy : e < L.z0 ? E.Nobs : e < L.z0z0 ? E.z0 : E.z0z0;
  const int base = e < L.S11 ? L.N : e < L.S10 ? L.S11 : e < L.S00 ? L.S10 : e < L.counts ? L.S00 : e < L.Syz ? L.counts : e < L.Szz ? L.Syz
                 : e < L.Syy ? L.Szz : e < L.Nobs ? L.Syy : e < L.z0 ? L.Nobs : e < L.z0z0 ? L.z0 : L.z0z0;
  if (!out) return;   // a block nobody asked for is not read
  float acc = 0.f;
  for (int b = 0; b < P.B; ++b) acc += E.ws[(int64_t)b * L.G + e];
  out[e - base] = acc;
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
