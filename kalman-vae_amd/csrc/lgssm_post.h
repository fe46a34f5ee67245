// lgssm_post.h — joint posterior samples of latent paths (include/kvae_lgssm.h kvae_lgssm_posterior_sample,
// KalmanFilter.sample_posterior, KVAE.sample_imputations): backward sampling over the filter's outputs, in three launches.
//
//   gains launch (parallel over the B*T items): nothing in
//       J_t = Sigma_{t|t} A_{t+1}^T Sigma_{t+1|t}^{-1}                      (the RTS gain, reference kalman_filter.py:221-229)
//       P_t = (I - J_t A_{t+1}) Sigma_{t|t} (I - J_t A_{t+1})^T + J_t Q_{t+1} J_t^T   (Joseph form), symmetrised
//       L_t = chol(P_t)   (the _safe_cholesky ladder of kalman_filter.py:282-303, PER ITEM; the level goes to levels_out)
//       c_t = mu_{t|t} - J_t mu_{t+1|t}
//     depends on the recursion, so every (b, t) is an independent item; item T-1 is J = 0, L = chol(Sigma_{T-1|T-1}),
//     c = mu_{T-1|T-1}.  An item writes the record J | L | c (2 n^2 + n floats) to the workspace.
//   path launch (sequential in t, parallel over the B*S paths): z_t = c_t + J_t z_{t+1} + L_t eps_t from z_T = 0.  The only
//     loop-carried value is z, and every operand of every step is known before the loop starts: the records and draws of the
//     next RING steps are in flight while a step is computed.
//   emission launch (parallel over the B*S*T rows): a_t = C_t z_t + L_R eta_t.  Kept out of the path loop on purpose: its loads
//     of C_t are not known RING steps ahead without more registers, and a load issued inside a step makes that step wait for
//     everything issued before it (loads return in order) - measured, the loop with the emission inside ran at one memory
//     round trip per step.
//
// Gains layout.  An item is worked by LPI lanes (16 at n = 4: four items per wavefront, one lane per matrix element; 64
// otherwise); its matrices sit in LDS and the body is a sequence of phases separated by __syncthreads (workgroups are one
// wavefront).  The solve is Gauss-Jordan with partial pivoting on [Sigma_{t+1|t}^T | (Sigma_{t|t} A^T)^T] - Sigma_{t+1|t} can
// be indefinite in fp32 - with the row exchanges kept as a packed permutation in every lane.  Control flow is uniform over the
// wavefront: the ladder runs while ANY item of the wavefront still needs a level (__any), finished items idle.
//
// Path layout.  Paths are numbered r = b*S + s, so the S paths of a sequence are neighbours in one wavefront (their J | L | c
// loads are the same address: one fetch) and sequences are packed when S is small.  n = 4: lane = path, z in registers, 16-byte
// loads.  n = 16: a path is a 16-lane ROW (four paths per wavefront), lane i owns row i of J_t, L_t and z_i, and the matvec takes
// the other z_j by DPP row broadcast - sixteen moves and four dependent FMAs per step, no LDS.  Run-time n, or operands that are
// not 16-byte aligned: lane = path, z in LDS (lane-private column, ping-pong), scalar loads.  No per-lane array is indexed at
// run time, so nothing lives in scratch.  No atomics, every output written once.
//
// Cross-lane traffic: LDS + __syncthreads + __any in the gains, DPP row_newbcast in the n = 16 paths - all of which the
// wavefront emulator (tests/hostsim/wave_emu.h) runs unchanged.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/kvae_lgssm.h"

namespace kvae_post {

constexpr int MAXD = KVAE_MAX_DIM;
constexpr int LEVELS = 5;          // jitter 1e-6 * 10^level, level 0..4; LEVELS = the clamped-diagonal fallback
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ const float *stack_at(const kvae_stack &s, int64_t b, int64_t t) { return s.ptr + b * s.sb + t * s.st; }

// the jitter of kalman_filter.py:289-296: a Python double, rounded to fp32 when multiplied into eye()
__device__ __forceinline__ float jitter_of(int level) {
  switch (level) {
    case 0: return (float)(1e-6);
    case 1: return (float)(1e-6 * 10.0);
    case 2: return (float)(1e-6 * 10.0 * 10.0);
    case 3: return (float)(1e-6 * 10.0 * 10.0 * 10.0);
    default: return (float)(1e-6 * 10.0 * 10.0 * 10.0 * 10.0);
  }
}

// ---- gains ------------------------------------------------------------------------------------------------------------------
template <int NM>
struct GainItem {
  float Sf[NM * NM], A[NM * NM], Q[NM * NM];   // Sigma_{t|t}, A_{t+1}, Q_{t+1}
  float aug[NM * 2 * NM];                      // [Sigma_{t+1|t}^T | (Sigma_{t|t} A^T)^T], eliminated in place
  float J[NM * NM], G[NM * NM], T1[NM * NM], T2[NM * NM], Pr[NM * NM], Ps[NM * NM], L[NM * NM];
  float muf[NM], mup[NM], c[NM];
};
template <int NC, int LPI>
struct GainLds {
  GainItem<NC ? NC : MAXD> item[64 / LPI];
};

// NC: compile-time n (0 = P.n); LPI lanes per item
template <int NC, int LPI>
__device__ void gains_wave(const kvae_psample_problem &P, GainLds<NC, LPI> &lds) {
  constexpr int IPW = 64 / LPI;
  const int n = NC ? NC : P.n, nn = n * n, ld = 2 * n, T = P.T;
  const int lane = (int)(threadIdx.x & 63), slot = lane / LPI, li = lane % LPI;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * IPW + slot;
  const bool live = it < items;
  if (!live) it = items - 1;   // a slot past the end repeats the last item and stores nothing
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const bool last = t == T - 1;
  const int64_t nx = last ? it : it + 1;   // step t+1 (item T-1 reads its own step: results unused, J = 0)
  auto &I = lds.item[slot];

  // ---- load ----
  {
    const float *Sf = P.Sigmas_filt + it * nn, *Sp = P.Sigmas_pred + nx * nn;
    const float *A = stack_at(P.A, b, last ? t : t + 1), *Q = stack_at(P.Q, b, last ? t : t + 1);
    for (int e = li; e < nn; e += LPI) {
      const int i = e / n, j = e - i * n;
      I.Sf[e] = Sf[e], I.A[e] = A[e], I.Q[e] = Q[e];
      I.aug[i * ld + j] = Sp[j * n + i];
      I.L[e] = 0.f;
    }
    for (int e = li; e < n; e += LPI) I.muf[e] = P.mus_filt[it * n + e], I.mup[e] = P.mus_pred[nx * n + e];
  }
  __syncthreads();
  for (int e = li; e < nn; e += LPI) {   // right-hand side (Sigma_{t|t} A^T)^T
    const int i = e / n, j = e - i * n;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(I.Sf[j * n + k], I.A[i * n + k], s);
    I.aug[i * ld + n + j] = s;
  }
  __syncthreads();

  // ---- X = Sigma_{t+1|t}^{-T} (Sigma_{t|t} A^T)^T = J^T: Gauss-Jordan, first-maximum partial pivoting ----
  uint64_t perm = 0xFEDCBA9876543210ull;   // row of position i: 4 bits each, the same in every lane of the item
  auto row_of = [&](int i) -> int { return (int)((perm >> (4 * i)) & 15ull); };
  for (int c = 0; c < n; ++c) {
    int piv = c;
    float best = fabsf(I.aug[row_of(c) * ld + c]);
    for (int i = c + 1; i < n; ++i) {
      const float v = fabsf(I.aug[row_of(i) * ld + c]);
      if (v > best) best = v, piv = i;
    }
    if (piv != c) {
      const uint64_t x = (perm >> (4 * c)) & 15ull, y = (perm >> (4 * piv)) & 15ull;
      perm &= ~((15ull << (4 * c)) | (15ull << (4 * piv)));
      perm |= (y << (4 * c)) | (x << (4 * piv));
    }
    const int pc = row_of(c);
    const float rinv = 1.0f / I.aug[pc * ld + c];
    const int cols = ld - c - 1;
    for (int e = li; e < (n - 1) * cols; e += LPI) {   // every other row, columns right of the pivot
      const int ii = e / cols, j = c + 1 + (e - ii * cols);
      const int pr = row_of(ii < c ? ii : ii + 1);
      const float f = I.aug[pr * ld + c] * rinv;
      I.aug[pr * ld + j] = fmaf(-f, I.aug[pc * ld + j], I.aug[pr * ld + j]);
    }
    __syncthreads();
  }
  for (int e = li; e < nn; e += LPI) {
    const int c = e / n, j = e - c * n;
    const int pc = row_of(c);
    I.J[j * n + c] = last ? 0.f : I.aug[pc * ld + n + j] / I.aug[pc * ld + c];
  }
  __syncthreads();

  // ---- G = I - J A, T2 = J Q, c = mu_f - J mu_p ----
  for (int e = li; e < nn; e += LPI) {
    const int i = e / n, j = e - i * n;
    float g = i == j ? 1.f : 0.f, q = 0.f;
    for (int k = 0; k < n; ++k) g = fmaf(-I.J[i * n + k], I.A[k * n + j], g), q = fmaf(I.J[i * n + k], I.Q[k * n + j], q);
    I.G[e] = g, I.T2[e] = q;
  }
  for (int i = li; i < n; i += LPI) {
    float v = I.muf[i];
    for (int k = 0; k < n; ++k) v = fmaf(-I.J[i * n + k], I.mup[k], v);
    I.c[i] = v;
  }
  __syncthreads();
  for (int e = li; e < nn; e += LPI) {   // T1 = G Sigma_{t|t}
    const int i = e / n, j = e - i * n;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(I.G[i * n + k], I.Sf[k * n + j], s);
    I.T1[e] = s;
  }
  __syncthreads();
  for (int e = li; e < nn; e += LPI) {   // P = T1 G^T + T2 J^T
    const int i = e / n, j = e - i * n;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(I.T1[i * n + k], I.G[j * n + k], s);
    for (int k = 0; k < n; ++k) s = fmaf(I.T2[i * n + k], I.J[j * n + k], s);
    I.Pr[e] = s;
  }
  __syncthreads();
  for (int e = li; e < nn; e += LPI) {
    const int i = e / n, j = e - i * n;
    I.Ps[e] = 0.5f * (I.Pr[e] + I.Pr[j * n + i]);
  }
  __syncthreads();

  // ---- the ladder: left-looking Cholesky of Ps + jitter I, one phase per column; uniform over the wavefront ----
  int level = -1;
  for (int lv = 0; lv < LEVELS; ++lv) {
    const float jit = jitter_of(lv);
    bool ok = true;
    for (int c = 0; c < n; ++c) {
      float d = I.Ps[c * n + c] + jit;
      for (int k = 0; k < c; ++k) d = fmaf(-I.L[c * n + k], I.L[c * n + k], d);
      if (!(d > 0.0f)) ok = false;   // a pivot <= 0 or NaN fails this level (as LAPACK potrf's info != 0)
      if (level < 0 && ok) {
        const float sd = sqrtf(d);
        for (int row = c + li; row < n; row += LPI) {
          if (row == c) {
            I.L[c * n + c] = sd;
          } else {
            float s = I.Ps[row * n + c];
            for (int k = 0; k < c; ++k) s = fmaf(-I.L[row * n + k], I.L[c * n + k], s);
            I.L[row * n + c] = s / sd;
          }
        }
      }
      __syncthreads();
    }
    if (level < 0 && ok) level = lv;
    if (!__any(level < 0)) break;
  }
  if (level < 0) {   // torch.diag_embed(sqrt(diag(P).clamp(min=1e-6)))
    for (int e = li; e < nn; e += LPI) {
      const int i = e / n, j = e - i * n;
      I.L[e] = i == j ? sqrtf(fmaxf(I.Ps[e], 1e-6f)) : 0.f;
    }
    level = LEVELS;
  }
  __syncthreads();

  if (live) {
    float *out = P.ws + it * (2 * nn + n);
    for (int e = li; e < nn; e += LPI) out[e] = I.J[e], out[nn + e] = I.L[e];
    for (int e = li; e < n; e += LPI) out[2 * nn + e] = I.c[e];
    if (li == 0) P.levels_out[it] = level;
  }
}

// ---- paths ------------------------------------------------------------------------------------------------------------------
constexpr int RING = 4;   // steps whose operands are in flight ahead of the one being computed (registers rotated by name)

// z <- c + J z + L eps, everything in the lane's registers (J, L as rows of 16-byte words); noise == false drops the draw
__device__ __forceinline__ void reg_step4(const f4 *J, const f4 *L, const f4 &c, const f4 &e, bool noise, f4 &z) {
  f4 zn;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = c[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) v = fmaf(J[i][k], z[k], v);
    if (noise) {
#pragma unroll
      for (int k = 0; k <= i; ++k) v = fmaf(L[i][k], e[k], v);   // L is lower triangular
    }
    zn[i] = v;
  }
  z = zn;
}

// n = 4, ws / eps / z_out 16-byte aligned.  Lane = path.  The loop is unrolled RING times so that the ring slots are named
// registers: slot d holds step t0 - d, and is refilled with step t0 - d - RING as soon as it has been used.
__device__ inline void paths_n4_wave(const kvae_psample_problem &P) {
  constexpr int REC = 36;
  const int T = P.T, S = P.S;
  const int64_t R = (int64_t)P.B * S;
  int64_t r = (int64_t)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  const bool live = r < R, noise = P.eps != nullptr;
  if (!live) r = R - 1;
  const int64_t b = r / S;
  struct Ops { f4 J[4], L[4], c, e; };
  auto load = [&](int t) {
    Ops o;
    t = t < 0 ? 0 : t;   // past the start: a valid address, never used
    const f4 *w = reinterpret_cast<const f4 *>(P.ws + (b * T + t) * REC);
#pragma unroll
    for (int q = 0; q < 4; ++q) o.J[q] = w[q], o.L[q] = w[4 + q];
    o.c = w[8];
    o.e = noise ? *reinterpret_cast<const f4 *>(P.eps + (r * T + t) * 4) : f4{0.f, 0.f, 0.f, 0.f};
    return o;
  };
  Ops ring[RING];
#pragma unroll
  for (int d = 0; d < RING; ++d) ring[d] = load(T - 1 - d);
  f4 z = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = T - 1; t0 >= 0; t0 -= RING) {
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int t = t0 - d;
      if (t >= 0) {
        reg_step4(ring[d].J, ring[d].L, ring[d].c, ring[d].e, noise, z);
        if (live) *reinterpret_cast<f4 *>(P.z_out + (r * T + t) * 4) = z;
      }
      ring[d] = load(t - RING);
    }
  }
}

template <int K>
__device__ __forceinline__ float row_bcast(float v) {   // lane K of the caller's 16-lane row (DPP row_newbcast)
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x150 + K, 0xf, 0xf, true));
}
// acc[k % 4] += row[k] * (x of lane k of the row), k = K .. 15: four partial sums keep the dependent chain at four FMAs
template <int K>
__device__ __forceinline__ void row_dot(const f4 *row, float x, float (&acc)[4]) {
  acc[K % 4] = fmaf(row[K / 4][K % 4], row_bcast<K>(x), acc[K % 4]);
  if constexpr (K + 1 < 16) row_dot<K + 1>(row, x, acc);
}

// n = 16, ws 16-byte aligned.  A path is a 16-lane row: lane i owns row i of J_t and L_t and element i of c, eps, z; the
// matvecs take z (eps) of the other lanes by DPP row broadcast - no LDS, no barrier.  Four paths per wavefront, the same ring.
__device__ inline void paths_n16_wave(const kvae_psample_problem &P) {
  constexpr int REC = 2 * 256 + 16;
  const int T = P.T, S = P.S, lane = (int)(threadIdx.x & 63), i = lane & 15;
  const int64_t R = (int64_t)P.B * S;
  int64_t r = (int64_t)blockIdx.x * 4 + (lane >> 4);
  const bool live = r < R, noise = P.eps != nullptr;
  if (!live) r = R - 1;
  const int64_t b = r / S;
  struct Ops { f4 J[4], L[4]; float c, e; };
  auto load = [&](int t) {
    Ops o;
    t = t < 0 ? 0 : t;
    const float *rec = P.ws + (b * T + t) * REC;
    const f4 *Jr = reinterpret_cast<const f4 *>(rec + 16 * i), *Lr = reinterpret_cast<const f4 *>(rec + 256 + 16 * i);
#pragma unroll
    for (int q = 0; q < 4; ++q) o.J[q] = Jr[q], o.L[q] = Lr[q];
    o.c = rec[512 + i];
    o.e = noise ? P.eps[(r * T + t) * 16 + i] : 0.f;
    return o;
  };
  Ops ring[RING];
#pragma unroll
  for (int d = 0; d < RING; ++d) ring[d] = load(T - 1 - d);
  float z = 0.f;
  for (int t0 = T - 1; t0 >= 0; t0 -= RING) {
#pragma unroll
    for (int d = 0; d < RING; ++d) {
      const int t = t0 - d;
      if (t >= 0) {   // uniform over the wavefront: every lane of a row reaches the DPP moves
        float acc[4] = {ring[d].c, 0.f, 0.f, 0.f};
        if (noise) row_dot<0>(ring[d].L, ring[d].e, acc);   // off the chain: does not depend on z
        row_dot<0>(ring[d].J, z, acc);
        z = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        if (live) P.z_out[(r * T + t) * 16 + i] = z;
      }
      ring[d] = load(t - RING);
    }
  }
}

struct PathLds {
  float z[2][MAXD][64];   // z_{t+1} / z_t of the lane's path: a lane-private column, no bank conflicts, no barrier
};

// run-time n, any alignment: lane = path, z in LDS
__device__ inline void paths_lds_wave(const kvae_psample_problem &P, PathLds &lds) {
  const int n = P.n, nn = n * n, T = P.T, S = P.S, lane = (int)(threadIdx.x & 63);
  const int64_t R = (int64_t)P.B * S;
  int64_t r = (int64_t)blockIdx.x * 64 + lane;
  const bool live = r < R;
  if (!live) r = R - 1;
  const int64_t b = r / S;
  for (int j = 0; j < n; ++j) lds.z[T & 1][j][lane] = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const int cur = t & 1, prv = cur ^ 1;   // z_{t+1} sits in buffer (t+1) & 1
    const int64_t row = r * T + t;
    const float *rec = P.ws + (b * T + t) * (2 * nn + n);
    const float *e = P.eps ? P.eps + row * n : nullptr;
    for (int i = 0; i < n; ++i) {
      float v = rec[2 * nn + i];
      for (int j = 0; j < n; ++j) v = fmaf(rec[i * n + j], lds.z[prv][j][lane], v);
      if (e)
        for (int j = 0; j <= i; ++j) v = fmaf(rec[nn + i * n + j], e[j], v);
      lds.z[cur][i][lane] = v;
      if (live) P.z_out[row * n + i] = v;
    }
  }
}

// ---- emission: a_t = C_t z_t + L_R eta_t, one lane per (path, step), after the paths (nothing here is sequential) -----------
__device__ inline void emit_wave(const kvae_psample_problem &P) {
  const int n = P.n, p = P.p, T = P.T;
  const int64_t rows = (int64_t)P.B * P.S * T, stride = (int64_t)gridDim.x * 64;
  for (int64_t row = (int64_t)blockIdx.x * 64 + (int)(threadIdx.x & 63); row < rows; row += stride) {
    const int64_t r = row / T, b = r / P.S;
    const int t = (int)(row - r * T);
    const float *Ct = stack_at(P.C, b, t), *z = P.z_out + row * n;
    const float *eta = P.eta ? P.eta + row * p : nullptr;
    for (int i = 0; i < p; ++i) {
      float v = 0.f;
      for (int j = 0; j < n; ++j) v = fmaf(Ct[i * n + j], z[j], v);
      if (eta)
        for (int j = 0; j <= i; ++j) v = fmaf(P.LR[i * p + j], eta[j], v);
      P.a_out[row * p + i] = v;
    }
  }
}

// ---- what both entry points (kvae_lgssm_post.hip, the host simulation below) share ----------------------------------------
inline int64_t post_ws_floats(const kvae_psample_problem *P) {
  if (!P || P->B < 1 || P->T < 1 || P->n < 1 || P->n > MAXD) return 0;
  return (int64_t)P->B * P->T * (2 * P->n * P->n + P->n);
}
inline bool post_runs(const kvae_psample_problem &P, int stage) { return P.stages == 0 || (P.stages & stage); }
inline int post_check(const kvae_psample_problem *P) {
  if (!P) return KVAE_ERR_NULL;
  const auto bad = [](int v) { return v < 1 || v > KVAE_MAX_DIM; };
  if (P->B < 1 || P->S < 1 || P->T < 1 || bad(P->n) || bad(P->p)) return KVAE_ERR_DIMS;
  if (P->stages < 0 || P->stages > 3) return KVAE_ERR_ARG;
  if (!P->ws) return KVAE_ERR_NULL;
  if (post_runs(*P, KVAE_PSAMPLE_GAINS) &&
      (!P->mus_filt || !P->Sigmas_filt || !P->mus_pred || !P->Sigmas_pred || !P->A.ptr || !P->Q.ptr || !P->levels_out))
    return KVAE_ERR_NULL;
  if (post_runs(*P, KVAE_PSAMPLE_PATHS) && (!P->C.ptr || !P->z_out || !P->a_out || (P->eta && !P->LR))) return KVAE_ERR_NULL;
  if (P->A.sb < 0 || P->A.st < 0 || P->C.sb < 0 || P->C.st < 0 || P->Q.sb < 0 || P->Q.st < 0) return KVAE_ERR_ARG;
  if ((int64_t)P->B * P->S > (int64_t)INT32_MAX || (int64_t)P->B * P->T > (int64_t)INT32_MAX) return KVAE_ERR_ARG;   // grid limits
  return KVAE_OK;
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// gains: 0 = n 4 (four items per wavefront), 1 = n 16, 2 = run-time n
inline int post_gain_kind(const kvae_psample_problem &P) { return P.n == 4 ? 0 : (P.n == 16 ? 1 : 2); }
inline unsigned post_gain_grid(const kvae_psample_problem &P) {
  const int64_t items = (int64_t)P.B * P.T, ipw = P.n == 4 ? 4 : 1;
  return (unsigned)((items + ipw - 1) / ipw);
}
// paths: 0 = n 4, lane per path; 1 = n 16, 16-lane row per path; 2 = LDS (run-time n, or 16-byte accesses impossible)
inline int post_path_kind(const kvae_psample_problem &P) {
  if (P.n == 4 && aligned16(P.ws) && aligned16(P.z_out) && (!P.eps || aligned16(P.eps))) return 0;
  return P.n == 16 && aligned16(P.ws) ? 1 : 2;
}
inline unsigned post_path_grid(const kvae_psample_problem &P) {
  const int64_t R = (int64_t)P.B * P.S, per = post_path_kind(P) == 1 ? 4 : 64;
  return (unsigned)((R + per - 1) / per);
}
// the emission strides over the rows with at most EMIT_WAVES wavefronts (four per CU)
constexpr int64_t EMIT_WAVES = 1024;
inline unsigned post_emit_grid(const kvae_psample_problem &P) {
  const int64_t w = ((int64_t)P.B * P.S * P.T + 63) / 64;
  return (unsigned)(w < EMIT_WAVES ? w : EMIT_WAVES);
}

}  // namespace kvae_post

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_posterior_sample (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) -----------
// Both kernel bodies on emulated wavefronts, with the grids and the instantiation choice of kvae_lgssm_post.hip; the launches
// are counted so that tests can assert the emulated kernels are what ran.  Include this header with KVAE_WAVE_EMU in ONE
// translation unit per binary (the definitions below are not inline).
#include <memory>

namespace kvae_post {
inline int &emu_launches() {
  static int n = 0;
  return n;
}
template <int NC, int LPI>
inline void gains_emu(const kvae_psample_problem &P) {
  auto L = std::make_unique<GainLds<NC, LPI>>();   // one wavefront at a time: the LDS of the workgroup in flight
  memset(L.get(), 0xFF, sizeof(*L));
  wemu::launch(post_gain_grid(P), [&] { gains_wave<NC, LPI>(P, *L); });
}
}  // namespace kvae_post

extern "C" int64_t kvae_lgssm_posterior_sample_ws_floats(const kvae_psample_problem *prob) { return kvae_post::post_ws_floats(prob); }
extern "C" int kvae_lgssm_posterior_sample(const kvae_psample_problem *prob, void *) {
  using namespace kvae_post;
  const int rc = post_check(prob);
  if (rc) return rc;
  const kvae_psample_problem &P = *prob;
  emu_launches() += 1;
  if (post_runs(P, KVAE_PSAMPLE_GAINS)) switch (post_gain_kind(P)) {
    case 0: gains_emu<4, 16>(P); break;
    case 1: gains_emu<16, 64>(P); break;
    default: gains_emu<0, 64>(P); break;
  }
  if (post_runs(P, KVAE_PSAMPLE_PATHS)) switch (post_path_kind(P)) {
    case 0: wemu::launch(post_path_grid(P), [&] { paths_n4_wave(P); }); break;
    case 1: wemu::launch(post_path_grid(P), [&] { paths_n16_wave(P); }); break;
    default: {
      auto L = std::make_unique<PathLds>();
      memset(L.get(), 0xFF, sizeof(*L));
      wemu::launch(post_path_grid(P), [&] { paths_lds_wave(P, *L); });
    }
  }
  if (post_runs(P, KVAE_PSAMPLE_PATHS)) wemu::launch(post_emit_grid(P), [&] { emit_wave(P); });
  return KVAE_OK;
}
extern "C" int kvae_wemu_posterior_launches(void) { return kvae_post::emu_launches(); }
#endif
