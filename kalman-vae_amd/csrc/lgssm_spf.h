// lgssm_spf.h — the Rao-Blackwellised particle filter of the generative switching model (include/kvae_lgssm.h
// kvae_lgssm_switching_pf, lgssm_ops.switching_pf, KalmanFilter.particle_filter_regimes, KVAE.particle_filter_regimes).  The
// equations are in the header of the C ABI; this file is their layout on a workgroup.
//
// One workgroup of N / 64 wavefronts per (sequence b, replicate g), lane = particle: its regime, log weight and Kalman belief
// (mu, Sigma) stay in registers for the whole sweep.  A_k, B_k, Q_k (zero-padded to 4 x 4) and log P are loaded once into LDS;
// the loop over the regimes j reads them at a uniform address (an LDS broadcast), the update under the drawn regime reads the
// chosen regime's at a per-lane address.  y_t, u_t, mask_t and the two draws are streamed one step ahead of the step that uses
// them, from a clamped address (the last step fetches itself again).
//   per step, on every lane: K predicts and pair densities (kvae_sw::predict / kvae_sw::update of csrc/lgssm_sw_pair.h, of which
//     only the density is read: the rest is dead code), the fully adapted weights, the draw, one measurement update.
//   sums over the particles, in a fixed order: inside a wavefront a butterfly of six __shfl_xor (both partners add the same two
//     numbers: every lane ends with the same bits), across the wavefronts one LDS row per wavefront, summed in ascending order by
//     every lane (block_sum / block_max): the logsumexp of the weights, the K Rao-Blackwellised sums with the ESS, the 4 + 10
//     moment sums.
//   resampling: an inclusive scan of the weights (six __shfl inside a wavefront, the wavefront totals through LDS; monotone up to
//     rounding only, see the search below), a binary search of the scan in LDS per lane, and the gather of the ancestor's 14
//     floats and its regime through LDS (15 KB at N = 256).
// Every branch tests kernel arguments or a value every lane of the workgroup holds with the same bits (mask_t, the ESS), so
// __syncthreads is never divergent.  No per-lane array is indexed at run time (every loop over one is unrolled over constants),
// no scratch.  Every multiply-add is an explicit fmaf and the unit is compiled with contraction off, so the bits of an output do
// not depend on which others are requested, and two calls give the same bits.
#pragma once
#include "lds_decl.h"
#include "lgssm_swf.h"

namespace kvae_spf {

using kvae_sw::padded;

constexpr int MAX_K = 8, MAX_N = 4, MAX_M = 4, MAX_PARTICLES = 256, MAX_WAVES = MAX_PARTICLES / 64;

// ---- sums and maxima over the particles of the workgroup: v[0..M) on every lane, the same bits on every lane afterwards ----
template <int M, bool MAX>
__device__ __forceinline__ void block_reduce(float (&v)[M], float (&red)[MAX_WAVES][16], int wave, int lane, int nw) {
  static_assert(M <= 16, "one LDS row per wavefront");
#pragma unroll
  for (int i = 0; i < M; ++i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float o = __shfl_xor(v[i], s, 64);
      v[i] = MAX ? fmaxf(v[i], o) : v[i] + o;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < M; ++i) red[wave][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < M; ++i) {
    float s = red[0][i];
    for (int w = 1; w < nw; ++w) s = MAX ? fmaxf(s, red[w][i]) : s + red[w][i];
    v[i] = s;
  }
  __syncthreads();   // red is free again
}

// regime k's dynamics out of LDS (k uniform: a broadcast; k per lane: the drawn regime's)
__device__ __forceinline__ void dynamics_of(const float (&dA)[MAX_K][16], const float (&dB)[MAX_K][16], const float (&dQ)[MAX_K][16], int k,
                                            float (&A)[4][4], float (&Bm)[4][4], float (&Q)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) A[r][c] = dA[k][4 * r + c], Bm[r][c] = dB[k][4 * r + c], Q[r][c] = dQ[k][4 * r + c];
  }
}

__device__ inline void sweep_block(const kvae_spf_problem &P) {
  const int T = P.T, K = P.K, N = P.N, n = P.n, m = P.m;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = N >> 6;
  const int64_t bg = blockIdx.x, b = bg / P.G;
  KV_LDS16(float, dA, [MAX_K][16]);
  KV_LDS16(float, dB, [MAX_K][16]);
  KV_LDS16(float, dQ, [MAX_K][16]);
  KV_LDS(float, lP, [MAX_K][MAX_K]);
  KV_LDS(float, red, [MAX_WAVES][16]);
  KV_LDS(float, cum, [MAX_PARTICLES]);
  KV_LDS(float, stage, [14][MAX_PARTICLES]);
  KV_LDS(int32_t, stage_r, [MAX_PARTICLES]);
  // ---- the dynamics and log P, once ----
  for (int e = tid; e < MAX_K * 16; e += N) {
    const int k = e >> 4, r = (e >> 2) & 3, c = e & 3;
    const bool vk = k < K;
    dA[k][e & 15] = padded(P.A + (vk ? k : 0) * n * n, n, n, r, c, vk);
    dB[k][e & 15] = padded(P.Bm + (vk ? k : 0) * n * m, n, m, r, c, vk);
    dQ[k][e & 15] = padded(P.Q + (vk ? k : 0) * n * n, n, n, r, c, vk);
  }
  for (int e = tid; e < MAX_K * MAX_K; e += N) {
    const int i = e >> 3, j = e & 7;
    const bool v = i < K && j < K;
    const float pr = P.P[v ? i * K + j : 0];
    lP[i][j] = v ? logf(pr) : -INFINITY;
  }
  float Cm[2][4], Rm[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int c = 0; c < 4; ++c) Cm[q][c] = padded(P.C, 2, n, q, c, true);
    Rm[q][0] = P.R[2 * q], Rm[q][1] = P.R[2 * q + 1];
  }
  const float lPuni = logf(1.0f / (float)K), nlogN = -logf((float)N);
  // ---- the particle: carried in, or (regime 0, weight 1 / N, (mu0, Sigma0)) ----
  const bool carried = P.state_log_w != nullptr;
  const int64_t part = bg * N + tid;
  float mu[4], Sg[4][4], lw;
  int reg;
  {
    const float *m0 = carried ? P.state_mu + part * n : P.mu0;
    const float *S0 = carried ? P.state_Sigma + part * n * n : P.Sigma0;
    lw = carried ? P.state_log_w[part] : nlogN;
    reg = carried ? P.state_regime[part] : 0;
    reg = reg < 0 ? 0 : (reg >= K ? K - 1 : reg);   // an index into LDS: never past the table, whatever the caller handed over
    kvae_sw::load_vec(m0, n, true, mu);
    kvae_sw::load_sym(S0, n, true, Sg);
  }
  __syncthreads();   // the tables are in LDS
  // ---- y_0, u_0, mask_0 and the draws of step 0 ----
  const int64_t q0 = b * T, g0 = bg * T;
  const float *maskp = P.mask ? P.mask + q0 : P.R;   // always a valid address
  const int mstep = P.mask ? 1 : 0;
  float yn0 = P.y[q0 * 2], yn1 = P.y[q0 * 2 + 1], mkn = maskp[0], un[4];
  float thn = P.pf_regime[g0 * N + tid], phn = P.pf_resample[g0];
#pragma unroll
  for (int c = 0; c < 4; ++c) un[c] = padded(P.u + q0 * m, 1, m, 0, c, true);
  const bool always = P.ess_threshold >= 1.0f, never = !(P.ess_threshold > 0.0f);

  for (int t = 0; t < T; ++t) {
    const int64_t q = g0 + t;
    const float y0 = yn0, y1 = yn1, mk = P.mask ? mkn : 1.0f, theta = thn, phi = phn;
    const float u[4] = {un[0], un[1], un[2], un[3]};
    {   // the next step's, in flight while this one computes
      const int tn = t + 1 < T ? t + 1 : t;
      const int64_t qn = q0 + tn;
      yn0 = P.y[qn * 2], yn1 = P.y[qn * 2 + 1], mkn = maskp[tn * mstep];
      thn = P.pf_regime[(g0 + tn) * N + tid], phn = P.pf_resample[g0 + tn];
#pragma unroll
      for (int c = 0; c < 4; ++c) un[c] = padded(P.u + qn * m, 1, m, 0, c, true);
    }
    const bool observed = mk != 0.0f, first = t == 0 && !carried;
    // ---- every regime j: predict, the pair density, log c_j ----
    float lc[MAX_K], lvl = 0.0f;
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
      lc[j] = -INFINITY;
      if (j < K) {
        float A[4][4], Bm[4][4], Q[4][4], mp[4], AS[4][4], Sp[4][4];
        kvae_sw::Update U;   // only the density is read
        dynamics_of(dA, dB, dQ, j, A, Bm, Q);
        kvae_sw::predict(A, Bm, Q, mu, Sg, u, mp, AS, Sp);
        kvae_sw::update(Cm, Rm, mp, Sp, y0, y1, mk, U);
        const float lp = first ? lPuni : lP[reg][j];
        lc[j] = lp + (observed ? U.tl.ll : 0.0f);
        lvl = fmaxf(lvl, lp > -INFINITY ? (float)U.tl.level : 0.0f);
      }
    }
    float mx = lc[0];
#pragma unroll
    for (int j = 1; j < MAX_K; ++j) mx = fmaxf(mx, lc[j]);
    float e[MAX_K], se = 0.0f;
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) {
      e[j] = expf(lc[j] - mx);   // 0 past K and for an impossible transition
      se += e[j];
    }
    const float inc = mx + logf(se);
    // ---- the weights: ll_t = logsumexp_i (lw_i + inc_i), the new normalised weights ----
    const float a = lw + inc;
    float top[2] = {a, lvl};
    block_reduce<2, true>(top, red, wave, lane, nw);
    const float ex = expf(a - top[0]);
    float tot[1] = {ex};
    block_reduce<1, false>(tot, red, wave, lane, nw);
    const float lS = logf(tot[0]), ll = top[0] + lS;
    const float lwn = (a - top[0]) - lS, Wn = ex / tot[0];
    float rf[MAX_K + 1];
#pragma unroll
    for (int j = 0; j < MAX_K; ++j) rf[j] = Wn * (e[j] / se);
    rf[MAX_K] = Wn * Wn;
    block_reduce<MAX_K + 1, false>(rf, red, wave, lane, nw);
    const float ess = 1.0f / rf[MAX_K];
    // ---- the draw ----
    int s = -1, last = 0;
    {
      const float thr = theta * se;
      float cs = 0.0f;
#pragma unroll
      for (int j = 0; j < MAX_K; ++j) {
        cs += e[j];
        if (s < 0 && cs > thr) s = j;
        if (e[j] > 0.0f) last = j;
      }
      s = s < 0 ? last : s;
    }
    // ---- the measurement update under the drawn regime (the statements of the loop above: the same predict) ----
    float muf[4], Sf[4][4];
    {
      float A[4][4], Bm[4][4], Q[4][4], mp[4], AS[4][4], Sp[4][4];
      kvae_sw::Update U;
      dynamics_of(dA, dB, dQ, s, A, Bm, Q);
      kvae_sw::predict(A, Bm, Q, mu, Sg, u, mp, AS, Sp);
      kvae_sw::update(Cm, Rm, mp, Sp, y0, y1, mk, U);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        muf[r] = U.muf[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) Sf[r][c] = U.Sf[r][c];
      }
    }
    // ---- the step's outputs ----
    const bool lead = tid == 0;
    if (P.ll && lead) P.ll[q] = observed ? ll : 0.0f;
    if (P.ess && lead) P.ess[q] = ess;
    if (P.levels && lead) P.levels[q] = (int32_t)top[1];
    if (P.regime_filt && lead) {
#pragma unroll
      for (int j = 0; j < MAX_K; ++j)
        if (j < K) P.regime_filt[q * K + j] = rf[j];
    }
    if (P.regimes) P.regimes[q * N + tid] = s;
    if (P.mus_filt || P.Sigmas_filt) {   // the moment match of the N beliefs under the new weights
      float mm[4], d[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) mm[r] = Wn * muf[r];
      block_reduce<4, false>(mm, red, wave, lane, nw);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d[r] = muf[r] - mm[r];
        if (P.mus_filt && lead && r < n) P.mus_filt[q * n + r] = mm[r];
      }
      if (P.Sigmas_filt) {
        float V[10];
        {
          int o = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int c = r; c < 4; ++c) V[o++] = Wn * fmaf(d[r], d[c], Sf[r][c]);
          }
        }
        block_reduce<10, false>(V, red, wave, lane, nw);
        int o = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int c = r; c < 4; ++c) {
            const float v = V[o++];
            if (lead && c < n) P.Sigmas_filt[q * n * n + r * n + c] = v, P.Sigmas_filt[q * n * n + c * n + r] = v;
          }
        }
      }
    }
    // ---- systematic resampling: the same decision on every lane (ess has the same bits on all of them) ----
    const bool rs = always || (!never && ess < P.ess_threshold * (float)N);
    if (P.resampled && lead) P.resampled[q] = rs ? 1 : 0;
    int anc = tid;
    if (rs) {
      float c = Wn;   // inclusive scan: inside the wavefront, then the totals of the wavefronts before this one
#pragma unroll
      for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const float o = __shfl(c, lane >= dlt ? lane - dlt : lane, 64);
        c = lane >= dlt ? c + o : c;
      }
      if (lane == 63) red[wave][0] = c;
      __syncthreads();
      float off = 0.0f;
      for (int w = 0; w < wave; ++w) off += red[w][0];
      cum[tid] = c + off;
#pragma unroll
      for (int r = 0; r < 4; ++r) stage[r][tid] = muf[r];
      {
        int o = 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int cc = r; cc < 4; ++cc) stage[o++][tid] = Sf[r][cc];
        }
      }
      stage_r[tid] = s;
      __syncthreads();
      const float pos = (phi + (float)tid) / (float)N;
      // The first slot whose cumulative weight exceeds pos, the last slot if none: log2 N halvings.  Adjacent prefixes of the scan are
      // summed along different trees, so cum is monotone only up to rounding: where two neighbours are out of order by an ulp the
      // halvings may settle on the neighbour (a slot whose own weight is below that rounding).  Fixed order, the same bits every call.
      int lo = 0;
      for (int half = N >> 1; half >= 1; half >>= 1) lo = cum[lo + half - 1] > pos ? lo : lo + half;
      anc = lo;
#pragma unroll
      for (int r = 0; r < 4; ++r) mu[r] = stage[r][anc];
      {
        int o = 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int cc = r; cc < 4; ++cc) {
            Sg[r][cc] = stage[o++][anc];
            Sg[cc][r] = Sg[r][cc];
          }
        }
      }
      reg = stage_r[anc];
      lw = nlogN;
      __syncthreads();   // red, cum and the stage are free again
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        mu[r] = muf[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) Sg[r][c] = Sf[r][c];
      }
      reg = s, lw = lwn;
    }
    if (P.ancestors) P.ancestors[q * N + tid] = anc;
  }
  // ---- the carried state out ----
  if (P.out_log_w) P.out_log_w[part] = lw;
  if (P.out_regime) P.out_regime[part] = reg;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (P.out_mu && r < n) P.out_mu[part * n + r] = mu[r];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (P.out_Sigma && r < n && c < n) P.out_Sigma[(part * n + r) * n + c] = Sg[r][c];
  }
}

// ---- the lineages: lane = final slot n of replicate (b, g), walked back over the ancestors of every step ----
__device__ inline void paths_block(const kvae_spf_problem &P) {
  const int T = P.T, N = P.N, tid = (int)threadIdx.x;
  const int64_t bg = blockIdx.x;
  int i = tid;
  for (int t = T - 1; t >= 0; --t) {
    const int64_t base = (bg * T + t) * N;
    i = P.ancestors[base + i];
    i = i < 0 ? 0 : (i >= N ? N - 1 : i);   // the sweep wrote a slot of this replicate; an index all the same
    P.paths[(bg * N + tid) * T + t] = P.regimes[base + i];
  }
}

// ---- seq_ll[b, g] = sum_t ll[b, g, t]: the switching filter's sequence sums over B * G rows ----
inline kvae_swf_problem seq_problem(const kvae_spf_problem &P) {
  kvae_swf_problem S{};
  S.B = P.B * P.G, S.T = P.T, S.ll = P.ll, S.seq_ll = P.seq_ll;
  return S;
}

// ---- what both entry points (kvae_lgssm_spf.hip, the host simulation below) share --------------------------------------------
inline int spf_check(const kvae_spf_problem *P) {
  if (!P) return KVAE_ERR_NULL;
  if (!P->A || !P->Bm || !P->Q || !P->C || !P->R || !P->P || !P->y || !P->u || !P->pf_regime || !P->pf_resample) return KVAE_ERR_NULL;
  const bool any = P->state_log_w || P->state_regime || P->state_mu || P->state_Sigma;
  const bool all = P->state_log_w && P->state_regime && P->state_mu && P->state_Sigma;
  if (!any && (!P->mu0 || !P->Sigma0)) return KVAE_ERR_NULL;
  if (P->seq_ll && !P->ll) return KVAE_ERR_NULL;                          // the sequence sums read ll
  if (P->paths && (!P->regimes || !P->ancestors)) return KVAE_ERR_NULL;   // the lineage walk reads both
  if (P->B < 1 || P->G < 1 || P->T < 1) return KVAE_ERR_DIMS;
  if (P->K < 1 || P->K > MAX_K || P->n < 1 || P->n > MAX_N || P->m < 1 || P->m > MAX_M || P->p != 2) return KVAE_ERR_ARG;
  if (P->N != 64 && P->N != 128 && P->N != 256) return KVAE_ERR_ARG;
  if (!(P->ess_threshold >= 0.0f && P->ess_threshold <= 1.0f)) return KVAE_ERR_ARG;
  if (any && !all) return KVAE_ERR_ARG;
  if ((int64_t)P->B * P->G > (int64_t)INT32_MAX) return KVAE_ERR_ARG;   // grid limit
  return KVAE_OK;
}
inline bool spf_wants_sweep(const kvae_spf_problem &P) {
  return P.ll || P.regime_filt || P.mus_filt || P.Sigmas_filt || P.ess || P.resampled || P.regimes || P.ancestors || P.levels ||
         P.out_log_w || P.out_regime || P.out_mu || P.out_Sigma;
}

}  // namespace kvae_spf

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_switching_pf (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) ---------------
// The kernel bodies on emulated workgroups, with the grids of kvae_lgssm_spf.hip; the launches are counted per body so that tests
// can assert which one ran.  Include this header with KVAE_WAVE_EMU in ONE translation unit per binary.
namespace kvae_spf {
inline int *emu_launches() {
  static int n[3] = {0, 0, 0};   // 0 the sweep, 1 the lineages, 2 the sequence sums
  return n;
}
}  // namespace kvae_spf

extern "C" int kvae_lgssm_switching_pf(const kvae_spf_problem *prob, void *) {
  using namespace kvae_spf;
  const int rc = spf_check(prob);
  if (rc) return rc;
  const kvae_spf_problem &P = *prob;
  const wemu::Dim3 grid = {(unsigned)(P.B * P.G), 1, 1};
  if (spf_wants_sweep(P)) {
    emu_launches()[0] += 1;
    wemu::launch_wg(grid, (unsigned)P.N, 0, [&] { sweep_block(P); });
  }
  if (P.paths) {
    emu_launches()[1] += 1;
    wemu::launch_wg(grid, (unsigned)P.N, 0, [&] { paths_block(P); });
  }
  if (P.seq_ll) {
    emu_launches()[2] += 1;
    const kvae_swf_problem S = seq_problem(P);
    wemu::launch((unsigned)S.B, [&] { kvae_swf::seq_wave(S); });
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_switching_pf_launches(int which) { return which >= 0 && which <= 2 ? kvae_spf::emu_launches()[which] : -1; }

#include "lgssm_swh.h"    // likewise kvae_lgssm_switching_forecast
#endif
