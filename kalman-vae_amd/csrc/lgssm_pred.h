// lgssm_pred.h — the exact predictive density of the latents (include/kvae_lgssm.h kvae_lgssm_predictive,
// KalmanFilter.predictive, KVAE.score / KVAE.log_likelihood): the prediction-error decomposition over the filter's own outputs.
//
//   item launch (parallel over the B*T items; nothing depends on the recursion - the filter has already run):
//       a_pred_t = C_t mu_{t|t-1}
//       S_t      = sym(C_t Sigma_{t|t-1} C_t^T + R)                    (0.5 (S + S^T), reference kalman_filter.py:62-79)
//       r_t      = y_t - a_pred_t
//       L_t      = chol(S_t)   (the _safe_cholesky ladder of kalman_filter.py:282-303, PER ITEM; the level is an output)
//       nis_t    = |L_t^{-1} r_t|^2,   ll_t = -0.5 (nis_t + 2 log det L_t + p log 2 pi)   (both 0 where mask_t == 0)
//   sequence launch (one wavefront per sequence, after the items): seq_ll_b = sum_t ll[b, t] - lane-strided partial sums in
//     ascending t, then a fixed butterfly.  No atomics, every output written once, two calls give the same bits.
//
// p = 2 throughout (as the filter kernels): the factor is l00 = sqrt(s00), l10 = s01 / l00, l11^2 = s11 - l10^2, a level failing
// where a pivot is not > 0 (the criterion of the ladder in csrc/lgssm_post.h).
//
// Item layout - three bodies, as the path launch of csrc/lgssm_post.h:
//   n = 4:  lane = item.  16-byte loads of the four rows of Sigma_{t|t-1}, of mu and of the two rows of C, an 8-byte load of y;
//           an 8-byte store of a_pred and a 16-byte store of S.  64 items per wavefront, no LDS, no cross-lane traffic.
//   n = 16: an item is a 16-lane ROW (four items per wavefront).  Lane i owns row i of Sigma_{t|t-1} (64 contiguous bytes) and
//           forms (Sigma C^T)[i][0..1] with two 16-term dot products (four partial sums each); the 2x2 C (Sigma C^T) and C mu
//           are six DPP row reductions, after which every lane of the row holds the same S and a_pred and runs the same tail.
//   run-time n <= 16, or operands that are not 16-byte aligned: lane = item, 4-byte loads, loops over n.
// No per-lane array is indexed at run time, so nothing lives in scratch.  A slot past the last item repeats the last item and
// stores nothing, so control flow around the DPP moves is uniform.  Every multiply-add is an explicit fmaf: the bits do not
// depend on which outputs are requested, and the n = 4 and run-time bodies sum in the same order.
//
// The adjoint (kvae_lgssm_predictive_bwd, KalmanFilter.log_marginal, the "marginal" training objective) is the second half of this
// header: one (b, t)-parallel launch, the same three bodies, S, r and the level recomputed by the statements above.
//
// Cross-lane traffic: DPP quad_perm / row_half_mirror / row_mirror in the n = 16 items, __shfl_xor in the sequence sums - all of
// which the wavefront emulator (tests/hostsim/wave_emu.h) runs unchanged.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/kvae_lgssm.h"

namespace kvae_pred {

constexpr int LEVELS = 5;                      // jitter 1e-6 * 10^level, level 0..4; LEVELS = the clamped-diagonal fallback
constexpr float LOG_2PI = 1.8378770664093453f;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

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

// ---- the tail every body shares: ladder, solve, density ------------------------------------------------------------------
struct Tail {
  float ll, nis;
  int level;
  float l00, l10, l11;   // the factor the level found (the adjoint below solves with it again)
};
// S = [[s00, s01], [s01, s11]] (symmetrised), r = y - a_pred
__device__ __forceinline__ Tail pred_tail(float s00, float s01, float s11, float r0, float r1) {
  float l00 = 0.f, l10 = 0.f, l11 = 0.f;
  int level = -1;
  for (int lv = 0; lv < LEVELS && level < 0; ++lv) {
    const float jit = jitter_of(lv);
    const float d0 = s00 + jit;
    if (!(d0 > 0.0f)) continue;   // a pivot <= 0 or NaN fails this level (as LAPACK potrf's info != 0)
    const float a = sqrtf(d0), b = s01 / a;
    const float d1 = fmaf(-b, b, s11 + jit);
    if (!(d1 > 0.0f)) continue;
    l00 = a, l10 = b, l11 = sqrtf(d1), level = lv;
  }
  if (level < 0) {   // torch.diag_embed(sqrt(diag(S).clamp(min=1e-6)))
    l00 = sqrtf(fmaxf(s00, 1e-6f)), l10 = 0.f, l11 = sqrtf(fmaxf(s11, 1e-6f));
    level = LEVELS;
  }
  const float w0 = r0 / l00;
  const float w1 = fmaf(-l10, w0, r1) / l11;
  Tail out;
  out.nis = fmaf(w1, w1, w0 * w0);
  const float logdet = 2.0f * (logf(l00) + logf(l11));
  out.ll = -0.5f * ((out.nis + logdet) + 2.0f * LOG_2PI);
  out.level = level;
  out.l00 = l00, out.l10 = l10, out.l11 = l11;
  return out;
}

__device__ __forceinline__ bool wants_tail(const kvae_pred_problem &P) { return P.ll || P.nis || P.levels; }
__device__ __forceinline__ bool wants_S(const kvae_pred_problem &P) { return P.S_out || wants_tail(P); }

// the scalar outputs of one item, by the one lane that owns it
__device__ __forceinline__ void store_tail(const kvae_pred_problem &P, int64_t it, const Tail &tl) {
  const bool observed = !P.mask || P.mask[it] != 0.0f;
  if (P.ll) P.ll[it] = observed ? tl.ll : 0.0f;
  if (P.nis) P.nis[it] = observed ? tl.nis : 0.0f;
  if (P.levels) P.levels[it] = tl.level;
}

// ---- n = 4: lane = item, 16-byte loads ----------------------------------------------------------------------------------------
__device__ __forceinline__ float dot4(const f4 &a, const f4 &b) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) s = fmaf(a[k], b[k], s);
  return s;
}

__device__ inline void items_n4_wave(const kvae_pred_problem &P) {
  const int T = P.T;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  const bool live = it < items;
  if (!live) it = items - 1;   // a lane past the end repeats the last item and stores nothing
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const f4 *Sg = reinterpret_cast<const f4 *>(P.Sigmas_pred + it * 16);
  const f4 *Cp = reinterpret_cast<const f4 *>(stack_at(P.C, b, t));
  const f4 sg0 = Sg[0], sg1 = Sg[1], sg2 = Sg[2], sg3 = Sg[3];
  const f4 mu = *reinterpret_cast<const f4 *>(P.mus_pred + it * 4);
  const f4 c0 = Cp[0], c1 = Cp[1];
  const f2 y = *reinterpret_cast<const f2 *>(P.y + it * 2);
  const float a0 = dot4(c0, mu), a1 = dot4(c1, mu);
  if (live && P.a_pred) *reinterpret_cast<f2 *>(P.a_pred + it * 2) = f2{a0, a1};
  if (!wants_S(P)) return;
  const f4 g0 = {dot4(sg0, c0), dot4(sg1, c0), dot4(sg2, c0), dot4(sg3, c0)};   // (Sigma C^T)[:, 0]
  const f4 g1 = {dot4(sg0, c1), dot4(sg1, c1), dot4(sg2, c1), dot4(sg3, c1)};
  const float S00 = dot4(c0, g0) + P.R[0], S01 = dot4(c0, g1) + P.R[1], S10 = dot4(c1, g0) + P.R[2], S11 = dot4(c1, g1) + P.R[3];
  const float s01 = 0.5f * (S01 + S10);
  if (live && P.S_out) *reinterpret_cast<f4 *>(P.S_out + it * 4) = f4{S00, s01, s01, S11};
  if (!wants_tail(P)) return;
  const Tail tl = pred_tail(S00, s01, S11, y[0] - a0, y[1] - a1);
  if (live) store_tail(P, it, tl);
}

// ---- n = 16: a 16-lane row per item ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the 16 lanes of a row (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror): every lane gets the same bits
__device__ __forceinline__ float row_sum(float x) {
  x += dpp<0xB1>(x);
  x += dpp<0x4E>(x);
  x += dpp<0x141>(x);
  x += dpp<0x140>(x);
  return x;
}
// 16-term dot product of two rows held as four 16-byte words: four partial sums keep the dependent chain at four FMAs
__device__ __forceinline__ float dot16(const f4 *a, const f4 *b) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = fmaf(a[q][k], b[q][k], acc[k]);
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__device__ inline void items_n16_wave(const kvae_pred_problem &P) {
  const int T = P.T, lane = (int)(threadIdx.x & 63), i = lane & 15;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * 4 + (lane >> 4);
  const bool live = it < items;
  if (!live) it = items - 1;   // uniform control flow: every lane of every row reaches the DPP moves
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const float *Ct = stack_at(P.C, b, t);
  const f4 *Sr = reinterpret_cast<const f4 *>(P.Sigmas_pred + it * 256 + 16 * i);
  const f4 *C0 = reinterpret_cast<const f4 *>(Ct), *C1 = reinterpret_cast<const f4 *>(Ct + 16);
  f4 sg[4], c0[4], c1[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) sg[q] = Sr[q], c0[q] = C0[q], c1[q] = C1[q];
  const float ci0 = Ct[i], ci1 = Ct[16 + i], mui = P.mus_pred[it * 16 + i];   // the lane's own column of C
  const float y0 = P.y[it * 2], y1 = P.y[it * 2 + 1];
  const float a0 = row_sum(ci0 * mui), a1 = row_sum(ci1 * mui);
  if (live && P.a_pred && i < 2) P.a_pred[it * 2 + i] = i == 0 ? a0 : a1;
  if (!wants_S(P)) return;   // uniform over the grid
  const float g0 = dot16(sg, c0), g1 = dot16(sg, c1);   // (Sigma C^T)[i][0..1]
  const float S00 = row_sum(ci0 * g0) + P.R[0], S01 = row_sum(ci0 * g1) + P.R[1];
  const float S10 = row_sum(ci1 * g0) + P.R[2], S11 = row_sum(ci1 * g1) + P.R[3];
  const float s01 = 0.5f * (S01 + S10);
  if (live && P.S_out && i < 4) P.S_out[it * 4 + i] = i == 0 ? S00 : (i == 3 ? S11 : s01);
  if (!wants_tail(P)) return;
  const Tail tl = pred_tail(S00, s01, S11, y0 - a0, y1 - a1);   // the same in every lane of the row
  if (live && i == 0) store_tail(P, it, tl);
}

// ---- run-time n, any alignment: lane = item, 4-byte loads -----------------------------------------------------------------------
__device__ inline void items_rt_wave(const kvae_pred_problem &P) {
  const int T = P.T, n = P.n;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  const bool live = it < items;
  if (!live) it = items - 1;
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const float *Sg = P.Sigmas_pred + it * n * n, *mu = P.mus_pred + it * n, *Ct = stack_at(P.C, b, t);
  float a0 = 0.f, a1 = 0.f;
  for (int j = 0; j < n; ++j) a0 = fmaf(Ct[j], mu[j], a0), a1 = fmaf(Ct[n + j], mu[j], a1);
  if (live && P.a_pred) P.a_pred[it * 2] = a0, P.a_pred[it * 2 + 1] = a1;
  if (!wants_S(P)) return;
  float S00 = 0.f, S01 = 0.f, S10 = 0.f, S11 = 0.f;
  for (int i = 0; i < n; ++i) {
    float g0 = 0.f, g1 = 0.f;   // (Sigma C^T)[i][0..1]
    for (int j = 0; j < n; ++j) {
      const float s = Sg[i * n + j];
      g0 = fmaf(s, Ct[j], g0), g1 = fmaf(s, Ct[n + j], g1);
    }
    S00 = fmaf(Ct[i], g0, S00), S01 = fmaf(Ct[i], g1, S01), S10 = fmaf(Ct[n + i], g0, S10), S11 = fmaf(Ct[n + i], g1, S11);
  }
  S00 += P.R[0], S01 += P.R[1], S10 += P.R[2], S11 += P.R[3];
  const float s01 = 0.5f * (S01 + S10);
  if (live && P.S_out) {
    float *o = P.S_out + it * 4;
    o[0] = S00, o[1] = s01, o[2] = s01, o[3] = S11;
  }
  if (!wants_tail(P)) return;
  const Tail tl = pred_tail(S00, s01, S11, P.y[it * 2] - a0, P.y[it * 2 + 1] - a1);
  if (live) store_tail(P, it, tl);
}

// ---- seq_ll[b] = sum_t ll[b, t]: one wavefront per sequence, fixed order ------------------------------------------------------
__device__ inline void seq_wave(const kvae_pred_problem &P) {
  const int T = P.T, lane = (int)(threadIdx.x & 63);
  const int64_t b = blockIdx.x;
  const float *ll = P.ll + b * T;
  float acc = 0.f;
  for (int t = lane; t < T; t += 64) acc += ll[t];   // hidden steps hold 0
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);   // both partners add the same two numbers: same bits
  if (lane == 0) P.seq_ll[b] = acc;
}

// ---- what both entry points (kvae_lgssm_pred.hip, the host simulation below) share -------------------------------------------
inline int pred_check(const kvae_pred_problem *P, bool outputs = true) {   // outputs false: the adjoint ignores the output pointers
  if (!P) return KVAE_ERR_NULL;
  const auto bad = [](int v) { return v < 1 || v > KVAE_MAX_DIM; };
  if (P->B < 1 || P->T < 1 || bad(P->n) || bad(P->p)) return KVAE_ERR_DIMS;
  if (P->p != 2) return KVAE_ERR_DIMS;   // the only emission width built
  if (!P->mus_pred || !P->Sigmas_pred || !P->C.ptr || !P->R || !P->y) return KVAE_ERR_NULL;
  if (outputs && P->seq_ll && !P->ll) return KVAE_ERR_NULL;   // the sequence sums read ll
  if (P->C.sb < 0 || P->C.st < 0) return KVAE_ERR_ARG;
  if ((int64_t)P->B * P->T > (int64_t)INT32_MAX) return KVAE_ERR_ARG;   // grid limit
  return KVAE_OK;
}
inline bool aligned(const void *p, unsigned bytes) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }
inline bool pred_wants_items(const kvae_pred_problem &P) { return P.ll || P.nis || P.a_pred || P.S_out || P.levels; }
// 0 = n 4, lane per item; 1 = n 16, 16-lane row per item; 2 = run-time n, or 16-byte accesses impossible
inline int pred_kind(const kvae_pred_problem &P) {
  const bool vec = aligned(P.Sigmas_pred, 16) && aligned(P.C.ptr, 16) && P.C.sb % 4 == 0 && P.C.st % 4 == 0;
  if (P.n == 4 && vec && aligned(P.mus_pred, 16) && aligned(P.y, 8) && aligned(P.a_pred, 8) && aligned(P.S_out, 16)) return 0;
  return P.n == 16 && vec ? 1 : 2;
}
inline unsigned pred_item_grid(const kvae_pred_problem &P) {
  const int64_t items = (int64_t)P.B * P.T, per = pred_kind(P) == 1 ? 4 : 64;
  return (unsigned)((items + per - 1) / per);
}

// ==== the adjoint: kvae_lgssm_predictive_bwd =====================================================================================
// Per item, with the weight w = g_ll[b,t] + g_seq[b] (0 on hidden steps), S~ = S + jitter(level) I, v = S~^-1 r, G = 0.5 (v v^T - S~^-1):
//     g_mu = w C^T v      g_Sigma = w C^T G C      gC = w (v mu^T + G C (Sigma + Sigma^T))      gY = -w v
// S, r and the level are recomputed by the forward's own statements (the same bits), v and S~^-1 from the factor pred_tail hands back.
// Level 5 (clamped diagonal, d_i = max(s_ii, 1e-6)): G_01 = 0 and G_ii = 0 where s_ii < 1e-6 (the backward of torch.clamp).
// Nothing recurrent: every item is independent, every output element is written by exactly one lane, once - no atomics, two calls
// give the same bits; an output that is NULL is skipped and the others keep their bits (every multiply-add is written out).
// The three bodies mirror the forward's; every element is formed by the same expression in all three:
//     h_a[k] = fmaf(G_a1, C[1][k], G_a0 C[0][k])                                  (H = G C, 2 x n)
//     g_mu[j] = w fmaf(C[1][j], v1, C[0][j] v0)        g_Sigma[i][j] = w fmaf(C[1][i], h_1[j], C[0][i] h_0[j])
//     gC[a][j] = w (v_a mu[j] + sum_k h_a[k] (Sigma[k][j] + Sigma[j][k])), k ascending in one fmaf chain
struct Adj {
  float v0, v1, g00, g01, g11;
};
__device__ __forceinline__ Adj pred_adjoint(const Tail &tl, float s00, float s11, float r0, float r1) {
  const float w0 = r0 / tl.l00;
  const float w1 = fmaf(-tl.l10, w0, r1) / tl.l11;   // L w = r, as pred_tail
  Adj a;
  a.v1 = w1 / tl.l11;                                // L^T v = w
  a.v0 = fmaf(-tl.l10, a.v1, w0) / tl.l00;
  const float q = 1.0f / tl.l00, e = 1.0f / tl.l11;  // L^-1 = [[q, 0], [m, e]],  S~^-1 = L^-T L^-1
  const float m = -(tl.l10 * q) * e;
  const float i00 = fmaf(m, m, q * q), i01 = m * e, i11 = e * e;
  a.g00 = 0.5f * (a.v0 * a.v0 - i00), a.g01 = 0.5f * (a.v0 * a.v1 - i01), a.g11 = 0.5f * (a.v1 * a.v1 - i11);
  if (tl.level == LEVELS) {   // the clamped diagonal: s_01 is not read, and s_ii only where the clamp lets it through
    a.g01 = 0.0f;
    if (!(s00 >= 1e-6f)) a.g00 = 0.0f;
    if (!(s11 >= 1e-6f)) a.g11 = 0.0f;
  }
  return a;
}
__device__ __forceinline__ float *gstack_at(const kvae_gstack &s, int64_t b, int64_t t) { return s.ptr + b * s.sb + t * s.st; }
// (observed, w) of one item
__device__ __forceinline__ float item_weight(const kvae_pred_problem &P, const kvae_pred_grads &G, int64_t it, int64_t b, bool &observed) {
  observed = !P.mask || P.mask[it] != 0.0f;
  return (G.g_ll ? G.g_ll[it] : 0.0f) + (G.g_seq ? G.g_seq[b] : 0.0f);
}

__device__ inline void bwd_n4_wave(const kvae_pred_problem &P, const kvae_pred_grads &G) {
  const int T = P.T;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  const bool live = it < items;
  if (!live) it = items - 1;   // a lane past the end repeats the last item and stores nothing
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const f4 *Sg = reinterpret_cast<const f4 *>(P.Sigmas_pred + it * 16);
  const f4 *Cp = reinterpret_cast<const f4 *>(stack_at(P.C, b, t));
  const f4 sg0 = Sg[0], sg1 = Sg[1], sg2 = Sg[2], sg3 = Sg[3];
  const f4 mu = *reinterpret_cast<const f4 *>(P.mus_pred + it * 4);
  const f4 c0 = Cp[0], c1 = Cp[1];
  const f2 y = *reinterpret_cast<const f2 *>(P.y + it * 2);
  // S, r and the level: the statements of items_n4_wave
  const float a0 = dot4(c0, mu), a1 = dot4(c1, mu);
  const f4 g0 = {dot4(sg0, c0), dot4(sg1, c0), dot4(sg2, c0), dot4(sg3, c0)};
  const f4 g1 = {dot4(sg0, c1), dot4(sg1, c1), dot4(sg2, c1), dot4(sg3, c1)};
  const float S00 = dot4(c0, g0) + P.R[0], S01 = dot4(c0, g1) + P.R[1], S10 = dot4(c1, g0) + P.R[2], S11 = dot4(c1, g1) + P.R[3];
  const float s01 = 0.5f * (S01 + S10);
  const float r0 = y[0] - a0, r1 = y[1] - a1;
  const Tail tl = pred_tail(S00, s01, S11, r0, r1);
  const Adj ad = pred_adjoint(tl, S00, S11, r0, r1);
  bool observed;
  const float w = item_weight(P, G, it, b, observed);
  if (!live) return;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  if (G.gY) *reinterpret_cast<f2 *>(G.gY + it * 2) = observed ? f2{-(w * ad.v0), -(w * ad.v1)} : f2{0.f, 0.f};
  if (G.g_mus_pred) {
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = w * fmaf(c1[j], ad.v1, c0[j] * ad.v0);
    *reinterpret_cast<f4 *>(G.g_mus_pred + it * 4) = observed ? o : zero;
  }
  if (!G.g_Sigmas_pred && !G.gC.ptr) return;
  f4 h0, h1;
#pragma unroll
  for (int k = 0; k < 4; ++k) h0[k] = fmaf(ad.g01, c1[k], ad.g00 * c0[k]), h1[k] = fmaf(ad.g11, c1[k], ad.g01 * c0[k]);
  if (G.g_Sigmas_pred) {
    f4 *o = reinterpret_cast<f4 *>(G.g_Sigmas_pred + it * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f4 row;
#pragma unroll
      for (int j = 0; j < 4; ++j) row[j] = w * fmaf(c1[i], h1[j], c0[i] * h0[j]);
      o[i] = observed ? row : zero;
    }
  }
  if (G.gC.ptr) {
    const f4 sg[4] = {sg0, sg1, sg2, sg3};   // indexed by unrolled constants only: registers
    f4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e0 = ad.v0 * mu[j], e1 = ad.v1 * mu[j];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float ss = sg[k][j] + sg[j][k];
        e0 = fmaf(h0[k], ss, e0), e1 = fmaf(h1[k], ss, e1);
      }
      o0[j] = w * e0, o1[j] = w * e1;
    }
    f4 *o = reinterpret_cast<f4 *>(gstack_at(G.gC, b, t));
    o[0] = observed ? o0 : zero, o[1] = observed ? o1 : zero;
  }
}

__device__ inline void bwd_n16_wave(const kvae_pred_problem &P, const kvae_pred_grads &G) {
  const int T = P.T, lane = (int)(threadIdx.x & 63), i = lane & 15;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * 4 + (lane >> 4);
  const bool live = it < items;
  if (!live) it = items - 1;   // uniform control flow: every lane of every row reaches the DPP moves
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const float *Ct = stack_at(P.C, b, t);
  const float *Sit = P.Sigmas_pred + it * 256;
  const f4 *Sr = reinterpret_cast<const f4 *>(Sit + 16 * i);
  const f4 *C0 = reinterpret_cast<const f4 *>(Ct), *C1 = reinterpret_cast<const f4 *>(Ct + 16);
  f4 sg[4], c0[4], c1[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) sg[q] = Sr[q], c0[q] = C0[q], c1[q] = C1[q];
  const float ci0 = Ct[i], ci1 = Ct[16 + i], mui = P.mus_pred[it * 16 + i];
  const float y0 = P.y[it * 2], y1 = P.y[it * 2 + 1];
  // S, r and the level: the statements of items_n16_wave
  const float a0 = row_sum(ci0 * mui), a1 = row_sum(ci1 * mui);
  const float g0 = dot16(sg, c0), g1 = dot16(sg, c1);
  const float S00 = row_sum(ci0 * g0) + P.R[0], S01 = row_sum(ci0 * g1) + P.R[1];
  const float S10 = row_sum(ci1 * g0) + P.R[2], S11 = row_sum(ci1 * g1) + P.R[3];
  const float s01 = 0.5f * (S01 + S10);
  const float r0 = y0 - a0, r1 = y1 - a1;
  const Tail tl = pred_tail(S00, s01, S11, r0, r1);      // the same in every lane of the row
  const Adj ad = pred_adjoint(tl, S00, S11, r0, r1);
  bool observed;
  const float w = item_weight(P, G, it, b, observed);
  if (!live) return;                                     // no cross-lane traffic below
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  if (G.gY && i < 2) G.gY[it * 2 + i] = observed ? -(w * (i == 0 ? ad.v0 : ad.v1)) : 0.0f;
  if (G.g_mus_pred) G.g_mus_pred[it * 16 + i] = observed ? w * fmaf(ci1, ad.v1, ci0 * ad.v0) : 0.0f;
  if (!G.g_Sigmas_pred && !G.gC.ptr) return;
  f4 h0[4], h1[4];                                       // H = G C, whole in every lane
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      h0[q][k] = fmaf(ad.g01, c1[q][k], ad.g00 * c0[q][k]), h1[q][k] = fmaf(ad.g11, c1[q][k], ad.g01 * c0[q][k]);
  }
  if (G.g_Sigmas_pred) {                                 // lane i: row i, 64 contiguous bytes
    f4 *o = reinterpret_cast<f4 *>(G.g_Sigmas_pred + it * 256 + 16 * i);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f4 row;
#pragma unroll
      for (int k = 0; k < 4; ++k) row[k] = w * fmaf(ci1, h1[q][k], ci0 * h0[q][k]);
      o[q] = observed ? row : zero;
    }
  }
  if (G.gC.ptr) {                                        // lane i: column i of gC; Sigma[k][i] read again (the 16 lanes of a row
    float e0 = ad.v0 * mui, e1 = ad.v1 * mui;            // read 64 contiguous bytes per k, lines this row has just loaded)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float ss = Sit[(4 * q + k) * 16 + i] + sg[q][k];
        e0 = fmaf(h0[q][k], ss, e0), e1 = fmaf(h1[q][k], ss, e1);
      }
    }
    float *o = gstack_at(G.gC, b, t);
    o[i] = observed ? w * e0 : 0.0f, o[16 + i] = observed ? w * e1 : 0.0f;
  }
}

__device__ inline void bwd_rt_wave(const kvae_pred_problem &P, const kvae_pred_grads &G) {
  const int T = P.T, n = P.n;
  const int64_t items = (int64_t)P.B * T;
  int64_t it = (int64_t)blockIdx.x * 64 + (int)(threadIdx.x & 63);
  if (it >= items) return;   // no cross-lane traffic in this body
  const int64_t b = it / T;
  const int t = (int)(it - b * T);
  const float *Sg = P.Sigmas_pred + it * n * n, *mu = P.mus_pred + it * n, *Ct = stack_at(P.C, b, t);
  // S, r and the level: the statements of items_rt_wave
  float a0 = 0.f, a1 = 0.f;
  for (int j = 0; j < n; ++j) a0 = fmaf(Ct[j], mu[j], a0), a1 = fmaf(Ct[n + j], mu[j], a1);
  float S00 = 0.f, S01 = 0.f, S10 = 0.f, S11 = 0.f;
  for (int i = 0; i < n; ++i) {
    float g0 = 0.f, g1 = 0.f;
    for (int j = 0; j < n; ++j) {
      const float s = Sg[i * n + j];
      g0 = fmaf(s, Ct[j], g0), g1 = fmaf(s, Ct[n + j], g1);
    }
    S00 = fmaf(Ct[i], g0, S00), S01 = fmaf(Ct[i], g1, S01), S10 = fmaf(Ct[n + i], g0, S10), S11 = fmaf(Ct[n + i], g1, S11);
  }
  S00 += P.R[0], S01 += P.R[1], S10 += P.R[2], S11 += P.R[3];
  const float s01 = 0.5f * (S01 + S10);
  const float r0 = P.y[it * 2] - a0, r1 = P.y[it * 2 + 1] - a1;
  const Tail tl = pred_tail(S00, s01, S11, r0, r1);
  const Adj ad = pred_adjoint(tl, S00, S11, r0, r1);
  bool observed;
  const float w = item_weight(P, G, it, b, observed);
  if (G.gY) G.gY[it * 2] = observed ? -(w * ad.v0) : 0.0f, G.gY[it * 2 + 1] = observed ? -(w * ad.v1) : 0.0f;
  if (G.g_mus_pred)
    for (int j = 0; j < n; ++j) G.g_mus_pred[it * n + j] = observed ? w * fmaf(Ct[n + j], ad.v1, Ct[j] * ad.v0) : 0.0f;
  if (G.g_Sigmas_pred) {
    float *o = G.g_Sigmas_pred + it * n * n;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const float h0 = fmaf(ad.g01, Ct[n + j], ad.g00 * Ct[j]), h1 = fmaf(ad.g11, Ct[n + j], ad.g01 * Ct[j]);
        o[i * n + j] = observed ? w * fmaf(Ct[n + i], h1, Ct[i] * h0) : 0.0f;
      }
  }
  if (G.gC.ptr) {
    float *o = gstack_at(G.gC, b, t);
    for (int j = 0; j < n; ++j) {
      float e0 = ad.v0 * mu[j], e1 = ad.v1 * mu[j];
      for (int k = 0; k < n; ++k) {
        const float h0 = fmaf(ad.g01, Ct[n + k], ad.g00 * Ct[k]), h1 = fmaf(ad.g11, Ct[n + k], ad.g01 * Ct[k]);
        const float ss = Sg[k * n + j] + Sg[j * n + k];
        e0 = fmaf(h0, ss, e0), e1 = fmaf(h1, ss, e1);
      }
      o[j] = observed ? w * e0 : 0.0f, o[n + j] = observed ? w * e1 : 0.0f;
    }
  }
}

// ---- what both entry points of the adjoint share --------------------------------------------------------------------------------
inline int pred_bwd_check(const kvae_pred_problem *P, const kvae_pred_grads *G) {
  const int rc = pred_check(P, false);
  if (rc) return rc;
  if (!G || (!G->g_ll && !G->g_seq)) return KVAE_ERR_NULL;
  if (G->gC.sb < 0 || G->gC.st < 0) return KVAE_ERR_ARG;
  return KVAE_OK;
}
inline bool pred_bwd_wants(const kvae_pred_grads &G) { return G.g_mus_pred || G.g_Sigmas_pred || G.gY || G.gC.ptr; }
// pred_kind over the inputs (the forward's output pointers are ignored), then the alignment of what this call writes
inline int pred_bwd_kind(const kvae_pred_problem &P, const kvae_pred_grads &G) {
  kvae_pred_problem in = P;
  in.a_pred = nullptr, in.S_out = nullptr;
  const int kind = pred_kind(in);
  if (kind == 0 && aligned(G.g_mus_pred, 16) && aligned(G.g_Sigmas_pred, 16) && aligned(G.gY, 8) && aligned(G.gC.ptr, 16) &&
      G.gC.sb % 4 == 0 && G.gC.st % 4 == 0)
    return 0;
  if (kind == 1 && aligned(G.g_Sigmas_pred, 16)) return 1;
  return 2;
}
inline unsigned pred_bwd_grid(const kvae_pred_problem &P, const kvae_pred_grads &G) {
  const int64_t items = (int64_t)P.B * P.T, per = pred_bwd_kind(P, G) == 1 ? 4 : 64;
  return (unsigned)((items + per - 1) / per);
}

}  // namespace kvae_pred

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_predictive (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) ---------------
// The kernel bodies on emulated wavefronts, with the grids and the body choice of kvae_lgssm_pred.hip; the launches are counted
// per body so that tests can assert which one ran.  Include this header with KVAE_WAVE_EMU in ONE translation unit per binary
// (the definitions below are not inline).
namespace kvae_pred {
inline int *emu_launches() {
  static int n[4] = {0, 0, 0, 0};   // 0 n = 4, 1 n = 16, 2 run-time n, 3 sequence sums
  return n;
}
}  // namespace kvae_pred

extern "C" int kvae_lgssm_predictive(const kvae_pred_problem *prob, void *) {
  using namespace kvae_pred;
  const int rc = pred_check(prob);
  if (rc) return rc;
  const kvae_pred_problem &P = *prob;
  if (pred_wants_items(P)) {
    const int kind = pred_kind(P);
    emu_launches()[kind] += 1;
    switch (kind) {
      case 0: wemu::launch(pred_item_grid(P), [&] { items_n4_wave(P); }); break;
      case 1: wemu::launch(pred_item_grid(P), [&] { items_n16_wave(P); }); break;
      default: wemu::launch(pred_item_grid(P), [&] { items_rt_wave(P); }); break;
    }
  }
  if (P.seq_ll) {
    emu_launches()[3] += 1;
    wemu::launch((unsigned)P.B, [&] { seq_wave(P); });
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_predictive_launches(int which) { return which >= 0 && which < 4 ? kvae_pred::emu_launches()[which] : -1; }

// ---- the host simulation's kvae_lgssm_predictive_bwd: the same grids and body choice, launches counted per body -------------
namespace kvae_pred {
inline int *emu_bwd_launches() {
  static int n[3] = {0, 0, 0};   // 0 n = 4, 1 n = 16, 2 run-time n
  return n;
}
}  // namespace kvae_pred

extern "C" int kvae_lgssm_predictive_bwd(const kvae_pred_problem *prob, const kvae_pred_grads *g, void *) {
  using namespace kvae_pred;
  const int rc = pred_bwd_check(prob, g);
  if (rc) return rc;
  const kvae_pred_problem &P = *prob;
  const kvae_pred_grads &G = *g;
  if (!pred_bwd_wants(G)) return KVAE_OK;
  const int kind = pred_bwd_kind(P, G);
  emu_bwd_launches()[kind] += 1;
  switch (kind) {
    case 0: wemu::launch(pred_bwd_grid(P, G), [&] { bwd_n4_wave(P, G); }); break;
    case 1: wemu::launch(pred_bwd_grid(P, G), [&] { bwd_n16_wave(P, G); }); break;
    default: wemu::launch(pred_bwd_grid(P, G), [&] { bwd_rt_wave(P, G); }); break;
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_predictive_bwd_launches(int which) { return which >= 0 && which < 3 ? kvae_pred::emu_bwd_launches()[which] : -1; }
#endif
