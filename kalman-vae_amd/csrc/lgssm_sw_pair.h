// lgssm_sw_pair.h — the per-pair statements of the GPB2 kernels on the 8 x 8 lane grid, written once: the switching filter
// (csrc/lgssm_swf.h), the switching smoother (csrc/lgssm_sws.h), the adjoint of the regime marginal (csrc/lgssm_swm.h), the E-step
// of EM (csrc/lgssm_em.h) and the multi-horizon forecast (csrc/lgssm_swh.h) are composed of them, so where two kernels must give
// the same bits (the smoother's predict and the filter's, the adjoint's recomputed step and the forward's, the E-step's smoother
// outputs and the smoother's, the forecast's horizon step and the filter's hidden step) they run the same statements.  lane = 8 g + k owns the pair (regime k on the side that is "along the lanes", regime g "on the groups"); A_g, B_g,
// Q_g sit in registers padded with zeros to 4 x 4 (run-time n, m <= 4).
// Everything here is a __forceinline__ function over references to float[4] / float[4][4] (or a small struct of them): after
// inlining a result that a caller does not read is dead code.  No per-lane array is indexed at run time (every loop is unrolled
// over constants), no LDS, no scratch.  Every multiply-add is an explicit fmaf and the units are compiled with contraction off, so
// the bits of a result do not depend on the caller.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/kvae_lgssm.h"
#include "lgssm_pred.h"
#include "regime_decode.h"

namespace kvae_sw {

using kvae::rdec::xg8;
using kvae::rgrid::oct_max;
using kvae::rgrid::oct_sum;

// all 64 lanes: the eight lanes of a group, then the eight groups
__device__ __forceinline__ float wave_sum(float x) { return xg8<0>(oct_sum(x)); }
__device__ __forceinline__ float wave_max(float x) { return xg8<1>(oct_max(x)); }

// element (r, c) of a row-major [rows, cols] matrix padded to 4 x 4: loaded from a valid address, selected afterwards
__device__ __forceinline__ float padded(const float *M, int rows, int cols, int r, int c, bool live) {
  const bool in = live && r < rows && c < cols;
  const float v = M[in ? r * cols + c : 0];
  return in ? v : 0.0f;
}

// a vector of n floats padded to 4
__device__ __forceinline__ void load_vec(const float *v, int n, bool live, float (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) out[r] = padded(v, 1, n, 0, r, live);
}

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

// the lane's place on the grid: the padding lanes (k >= K or g >= K) read regime 0 and select zeros
struct Lane {
  int lane, k, g, kc, gc;
  bool vk, vg, ve;
};
__device__ __forceinline__ Lane lane_of(int K) {
  const int lane = (int)(threadIdx.x & 63), k = lane & 7, g = lane >> 3;
  const bool vk = k < K, vg = g < K;
  return Lane{lane, k, g, vk ? k : 0, vg ? g : 0, vk, vg, vk && vg};
}

// regime g's dynamics
__device__ __forceinline__ void load_dynamics(const kvae_swf_problem &P, int gc, bool vg, float (&A)[4][4], float (&Bm)[4][4],
                                              float (&Q)[4][4]) {
  const int n = P.n, m = P.m;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      A[r][c] = padded(P.A + gc * n * n, n, n, r, c, vg);
      Bm[r][c] = padded(P.Bm + gc * n * m, n, m, r, c, vg);
      Q[r][c] = padded(P.Q + gc * n * n, n, n, r, c, vg);
    }
  }
}

// the shared emission, the transition matrix at (i = k, j = g) and the uniform matrix of a sweep's first step
struct Emission {
  float C[2][4], R[2][2];
  float Pij, lPij, Puni, lPuni;
};
__device__ __forceinline__ void load_emission(const kvae_swf_problem &P, const Lane &ln, Emission &E) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int c = 0; c < 4; ++c) E.C[q][c] = padded(P.C, 2, P.n, q, c, true);
    E.R[q][0] = P.R[2 * q], E.R[q][1] = P.R[2 * q + 1];
  }
  const float Pr = P.P[ln.ve ? ln.k * P.K + ln.g : 0];
  E.Pij = ln.ve ? Pr : 0.0f, E.lPij = ln.ve ? logf(Pr) : -INFINITY;
  E.Puni = 1.0f / (float)P.K, E.lPuni = logf(E.Puni);
}

// ---- predict of the pair: mu_p = A mu + B u, AS = A Sigma, Sigma_p = AS A^T + Q ----
__device__ __forceinline__ void predict(const float (&A)[4][4], const float (&Bm)[4][4], const float (&Q)[4][4], const float (&mu)[4],
                                        const float (&Sg)[4][4], const float (&u)[4], float (&mp)[4], float (&AS)[4][4],
                                        float (&Sp)[4][4]) {
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
}

// ---- the measurement update of the pair - the statements of filter_gain / filter_step_core (csrc/lgssm_fwd.h), the 2 x 2 solve by
// elimination without pivoting (S is positive definite) - and the pair density by pred_tail (csrc/lgssm_pred.h) ----
struct Update {
  float ap[2], res[2], CP[2][4], PCT[4][2];   // the forecast C mu_p, y - forecast, C Sigma_p, Sigma_p C^T
  float S00, S01, S11, el, ed;                // S = C Sigma_p C^T + R; its elimination: el = S01 / S00, ed the second pivot
  kvae_pred::Tail tl;                         // log N(res; 0, S) and the level it was computed at
  float Kt[4][2], Kg[4][2];                   // Kt = Sigma_p C^T S^-1, K = mask * Kt
  float IKC[4][4], muf[4], Sf[4][4];          // I - K C, the filtered pair (Joseph form, symmetrised)
};
__device__ __forceinline__ void update(const float (&C)[2][4], const float (&R)[2][2], const float (&mp)[4], const float (&Sp)[4][4],
                                       float y0, float y1, float mk, Update &U) {
#pragma unroll
  for (int qq = 0; qq < 2; ++qq) {
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(C[qq][e], mp[e], acc);
    U.ap[qq] = acc;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s1 = fmaf(C[qq][e], Sp[e][c], s1), s2 = fmaf(Sp[c][e], C[qq][e], s2);
      U.CP[qq][c] = s1, U.PCT[c][qq] = s2;
    }
  }
  U.res[0] = y0 - U.ap[0], U.res[1] = y1 - U.ap[1];
  float s00 = 0.f, s01a = 0.f, s01b = 0.f, s11 = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s00 = fmaf(U.CP[0][e], C[0][e], s00), s01a = fmaf(U.CP[0][e], C[1][e], s01a);
    s01b = fmaf(U.CP[1][e], C[0][e], s01b), s11 = fmaf(U.CP[1][e], C[1][e], s11);
  }
  U.S00 = s00 + R[0][0], U.S11 = s11 + R[1][1];   // 0.5 (x + x) = x
  U.S01 = 0.5f * ((s01a + R[0][1]) + (s01b + R[1][0]));
  U.tl = kvae_pred::pred_tail(U.S00, U.S01, U.S11, U.res[0], U.res[1]);
  // ---- gain (S^-1 PCT^T by elimination), update, Joseph form ----
  U.el = U.S01 / U.S00, U.ed = fmaf(-U.el, U.S01, U.S11);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float x1 = fmaf(-U.el, U.PCT[r][0], U.PCT[r][1]) / U.ed;
    const float x0 = fmaf(-U.S01, x1, U.PCT[r][0]) / U.S00;
    U.Kt[r][0] = x0, U.Kt[r][1] = x1;
    U.Kg[r][0] = mk * x0, U.Kg[r][1] = mk * x1;
  }
  float KR[4][2], T1[4][4], F0[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) U.IKC[r][c] = (r == c ? 1.0f : 0.0f) - fmaf(U.Kg[r][1], C[1][c], U.Kg[r][0] * C[0][c]);
    KR[r][0] = fmaf(U.Kg[r][1], R[1][0], U.Kg[r][0] * R[0][0]), KR[r][1] = fmaf(U.Kg[r][1], R[1][1], U.Kg[r][0] * R[0][1]);
    U.muf[r] = fmaf(U.Kg[r][1], U.res[1], fmaf(U.Kg[r][0], U.res[0], mp[r]));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(U.IKC[r][e], Sp[e][c], s);
      T1[r][c] = s;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s = fmaf(T1[r][e], U.IKC[c][e], s);
      F0[r][c] = s + fmaf(KR[r][1], U.Kg[c][1], KR[r][0] * U.Kg[c][0]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = r; c < 4; ++c) {
      U.Sf[r][c] = 0.5f * (F0[r][c] + F0[c][r]);
      U.Sf[c][r] = U.Sf[r][c];
    }
  }
}

// ---- the weights of a step: log c_ij, the column softmax W_{i|j} (one-hot at i = j in a dead column) and logsumexp_ij ----
struct Weights {
  float logc, cmx, se, W, tot;   // cmx, se: the maximum of column j and the sum of exp(log c - cmx) over it, on the groups
};
__device__ __forceinline__ Weights weights(const Lane &ln, float lw, float lPt, float lij) {
  Weights w;
  w.logc = ln.ve ? (lw + lPt) + lij : -INFINITY;
  w.cmx = oct_max(w.logc);
  const bool dead = !(w.cmx > -INFINITY);                           // an impossible regime: W one-hot at i = j
  const float ex = dead ? (ln.k == ln.g ? 1.0f : 0.0f) : expf(w.logc - w.cmx);
  w.se = oct_sum(ex);
  w.W = ex / w.se;
  const float mx = xg8<1>(w.cmx);
  w.tot = mx + logf(xg8<0>(ln.vg ? w.se * expf(w.cmx - mx) : 0.0f));   // logsumexp_ij; a dead column adds 1 * exp(-inf) = 0
  return w;
}

// ---- the transpose of the grid: a scalar, a vector and the upper triangle of a symmetric matrix from lane src, fifteen __shfl;
// a lane that is not live takes pad for the scalar and zeros for the rest ----
__device__ __forceinline__ void hand_over(int src, bool live, float pad, float s, const float (&v)[4], const float (&S)[4][4], float &so,
                                          float (&vo)[4], float (&So)[4][4]) {
  {
    const float x = __shfl(s, src, 64);
    so = live ? x : pad;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float x = __shfl(v[r], src, 64);
    vo[r] = live ? x : 0.0f;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = r; c < 4; ++c) {
      const float x = __shfl(S[r][c], src, 64);
      So[r][c] = live ? x : 0.0f;
      So[c][r] = So[r][c];
    }
  }
}

// ---- the collapse of a step over i, inside column j: regime j's belief (mc, the upper triangle of Sc), on the groups ----
__device__ __forceinline__ void collapse_pairs(float W, const float (&muf)[4], const float (&Sf)[4][4], float (&mc)[4], float (&Sc)[4][4]) {
  float d[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mc[r] = oct_sum(W * muf[r]);
    d[r] = muf[r] - mc[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = r; c < 4; ++c) Sc[r][c] = oct_sum(W * fmaf(d[r], d[c], Sf[r][c]));
  }
}

// ---- the moment match of the K^2 pair forecasts under the prior weights pw = w(i) P[i,j]: row q of a_pred [., 2] and of
// S [., 2, 2]; either may be NULL ----
__device__ __forceinline__ void forecast_outputs(const Lane &ln, const Update &U, float pw, int64_t q, float *a_pred, float *S_out) {
  if (a_pred || S_out) {
    const float a0 = wave_sum(pw * U.ap[0]), a1 = wave_sum(pw * U.ap[1]);
    if (a_pred && ln.lane == 0) a_pred[q * 2] = a0, a_pred[q * 2 + 1] = a1;
    if (S_out) {
      const float e0 = U.ap[0] - a0, e1 = U.ap[1] - a1;
      const float o00 = wave_sum(pw * fmaf(e0, e0, U.S00)), o01 = wave_sum(pw * fmaf(e0, e1, U.S01));
      const float o11 = wave_sum(pw * fmaf(e1, e1, U.S11));
      if (ln.lane == 0) {
        float *o = S_out + q * 4;
        o[0] = o00, o[1] = o01, o[2] = o01, o[3] = o11;
      }
    }
  }
}

// ---- the moment match of the K collapsed Gaussians (mc, Sc: on the groups) under wj = w'(j): row q of mus [., n] and of
// Sigmas [., n, n]; either may be NULL.  The operands are already equal inside a group (wj = 0 on the groups past K), so the sum
// over the groups is all there is ----
__device__ __forceinline__ void belief_outputs(const Lane &ln, int n, float wj, const float (&mc)[4], const float (&Sc)[4][4], int64_t q,
                                               float *mus, float *Sigmas) {
  if (mus || Sigmas) {
    float mm[4], dd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mm[r] = xg8<0>(wj * mc[r]);
      dd[r] = mc[r] - mm[r];
      if (mus && ln.lane == 0 && r < n) mus[q * n + r] = mm[r];
    }
    if (Sigmas) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = r; c < 4; ++c) {
          const float v = xg8<0>(wj * fmaf(dd[r], dd[c], Sc[r][c]));
          if (ln.lane == 0 && c < n) Sigmas[q * n * n + r * n + c] = v, Sigmas[q * n * n + c * n + r] = v;
        }
      }
    }
  }
}

// =====================================================================================================================================
// the backward pass of the smoother: lane = 8 g + k owns the pair (regime k at step t - 1, regime g at step t)
// =====================================================================================================================================

// regime k's smoothed belief of a step, "along the lanes": M(k) and the Gaussian
struct Smoothed {
  float M, mu[4], Sigma[4][4];
};
// step T - 1: the filtered belief is the smoothed one, M = the final weights
__device__ __forceinline__ void last_belief(const kvae_sws_problem &S, const Lane &ln, Smoothed &Z) {
  const kvae_swf_problem &P = S.filt;
  const int64_t b = blockIdx.x, s = (b * P.T + P.T - 1) * P.K + ln.kc;
  const float w = S.hist_w[b * P.K + ln.kc];
  Z.M = ln.vk ? w : 0.0f;
  load_vec(S.hist_mu + s * P.n, P.n, ln.vk, Z.mu);
  load_sym(S.hist_Sigma + s * P.n * P.n, P.n, ln.vk, Z.Sigma);
}

// the operands of the transition into step t, streamed one step ahead: regime k's filtered belief of step t - 1 (clamped to step 0;
// with prior the transition into step 0 exists and its source is (mu0, Sigma0)), W[k,g] and u of step t
struct Transition {
  float mu[4], Sigma[4][4], W, u[4];
};
__device__ __forceinline__ void fetch(const kvae_sws_problem &S, const Lane &ln, int t, bool prior, Transition &X) {
  const kvae_swf_problem &P = S.filt;
  const int K = P.K, n = P.n, m = P.m;
  const int64_t q0 = (int64_t)blockIdx.x * P.T;
  const bool pri = prior && t == 0;
  const int64_t s = (q0 + (t >= 1 ? t - 1 : 0)) * K + ln.kc;
  const float *pm = pri ? P.mu0 : S.hist_mu + s * n, *pS = pri ? P.Sigma0 : S.hist_Sigma + s * n * n;
  load_vec(pm, n, ln.vk, X.mu);
  load_sym(pS, n, ln.vk, X.Sigma);
  X.W = S.hist_W[ln.ve ? ((q0 + t) * K + ln.k) * K + ln.g : 0];
#pragma unroll
  for (int c = 0; c < 4; ++c) X.u[c] = padded(P.u + (q0 + t) * m, 1, m, 0, c, true);
}

// the smoother's outputs of step q: M, and the moment match of the K smoothed Gaussians under it (inside a group) - mm and the upper
// triangle of V, computed where an output asks for them or the caller does (the E-step's emission sums)
__device__ __forceinline__ void step_outputs(const kvae_sws_problem &S, const Lane &ln, int64_t q, const Smoothed &Z, bool wanted,
                                             float (&mm)[4], float (&V)[4][4]) {
  const int K = S.filt.K, n = S.filt.n;
  const bool lead = ln.lane == 0;
  if (S.regime_smooth && ln.lane < K) S.regime_smooth[q * K + ln.lane] = Z.M;
  if (wanted || S.mus_smooth || S.Sigmas_smooth) {
    float dd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mm[r] = oct_sum(Z.M * Z.mu[r]);
      dd[r] = Z.mu[r] - mm[r];
      if (S.mus_smooth && lead && r < n) S.mus_smooth[q * n + r] = mm[r];
    }
    if (wanted || S.Sigmas_smooth) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = r; c < 4; ++c) {
          V[r][c] = oct_sum(Z.M * fmaf(dd[r], dd[c], Z.Sigma[r][c]));
          if (S.Sigmas_smooth && lead && c < n) S.Sigmas_smooth[q * n * n + r * n + c] = V[r][c], S.Sigmas_smooth[q * n * n + c * n + r] = V[r][c];
        }
      }
    }
  }
}

// ---- the smoothed pair from regime g's smoothed belief (mg, Sgs) of step t: X = J^T = Sigma_p^-T (A Sigma) by elimination in
// natural order without pivoting (the zero padding of n < 4 gets a unit diagonal, so the padded rows of J^T stay 0), then
// mu_s = mu + J (mu_s^g - mu_p), Sigma_s = sym(Sigma + J (Sigma_s^g - Sigma_p) J^T), of which Sj holds the upper triangle ----
__device__ __forceinline__ void smoothed_pair(int n, bool vg, const float (&mu)[4], const float (&Sg)[4][4], const float (&mp)[4],
                                              const float (&AS)[4][4], const float (&Sp)[4][4], const float (&mg)[4],
                                              const float (&Sgs)[4][4], float (&X)[4][4], float (&mj)[4], float (&Sj)[4][4]) {
  float L[4][4];
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
  float dm[4], D[4][4], JD[4][4], F[4][4];
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
}

// ---- the pair marginal of (step t - 1 regime k, step t regime g) ----
// A column of the rounded W sums to 1 within a few ulp only, and nearly the same column comes back step after step, so W * M alone
// lets the total mass of M drift linearly in T (1e-6 over 70 steps).  Dividing M_t(g) by the column's own sum (1 in exact
// arithmetic; inside the group, three DPP moves) keeps sum_k pairs(k, g) = M_t(g) to rounding.
__device__ __forceinline__ float pair_marginal(float W, float Mg, bool vg) {
  const float cs = oct_sum(W);
  return W * (Mg / (vg ? cs : 1.0f));
}

// ---- collapse over g: M_{t-1}(k) over the groups, V_{g|k} (one-hot at g = k where M_{t-1}(k) = 0), regime k's smoothed belief
// of step t - 1, along the lanes; the pair marginal goes to row p of regime_pairs ----
__device__ __forceinline__ void collapse(const kvae_sws_problem &S, const Lane &ln, int64_t p, float pr, const float (&mj)[4],
                                         const float (&Sj)[4][4], Smoothed &Z) {
  const float Mn = xg8<0>(pr);
  const bool dead = !(Mn > 0.0f);
  const float V = dead ? (ln.k == ln.g ? 1.0f : 0.0f) : pr / Mn;
  if (S.regime_pairs && ln.ve) S.regime_pairs[(p * S.filt.K + ln.k) * S.filt.K + ln.g] = pr;
  float d[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Z.mu[r] = xg8<0>(V * mj[r]);
    d[r] = mj[r] - Z.mu[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = r; c < 4; ++c) {
      Z.Sigma[r][c] = xg8<0>(V * fmaf(d[r], d[c], Sj[r][c]));
      Z.Sigma[c][r] = Z.Sigma[r][c];
    }
  }
  Z.M = Mn;
}

// ---- out[e - off] = sum_b ws[b, e], b ascending, for the block (out, off) that holds e: one thread per element e of a row of ws,
// G floats long.  The caller offers the blocks of its layout in ascending order of their offsets; the last one that starts at or
// before e is e's.  A block nobody asked for (out == NULL) is not read. ----
struct Block {
  float *out;
  int off;
};
__device__ __forceinline__ void offer(Block &k, int e, float *out, int off) {
  if (e >= off) k.out = out, k.off = off;
}
__device__ __forceinline__ void reduce_rows(const float *ws, int B, int G, int e, const Block &k) {
  if (e >= G || !k.out) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += ws[(int64_t)b * G + e];
  k.out[e - k.off] = acc;
}

}  // namespace kvae_sw
