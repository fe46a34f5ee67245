// regime_decode.h — exact inference over the regime chain of the switching dynamics (include/kvae_lgssm.h kvae_regime_decode,
// lgssm_ops.regime_decode, SwitchingDynamicsParameter.decode, KVAE.decode_regimes).  The variational posterior is a Markov chain,
//   q(s_0) = softmax(init_logits),   q(s_t = j | s_{t-1} = i) = Q_t[i,j],  Q_t = row-softmax(logits[t]),
// so its marginals, its most likely path and its KL against the sticky prior are one forward sweep (no sampling, no tau):
//   m_0 = softmax(init),             m_t[j] = sum_i m_{t-1}[i] Q_t[i,j]                        (probability space, never renormalised)
//   d_0 = log_softmax(init),         d_t[j] = max_i d_{t-1}[i] + log Q_t[i,j],  bp_t[j] = the LOWEST i that attains it
//   kl_0 = sum_j m_0[j] (log m_0[j] - log(1/K)),   kl_t = sum_i m_{t-1}[i] sum_j Q_t[i,j] (log Q_t[i,j] - log max(P[i,j], 1e-8))
//   path_logq = max_j d_{T-1}[j],    path: lowest argmax of d_{T-1}, then s_{t-1} = bp_t[s_t]
// (the clamp is the one of regime.h's log p_t).  One launch, one wavefront per sequence, as the sampled chain (regime_grid.h).
//
// K <= 8: registers only on the 8 x 8 lane grid of regime_grid.h, lane = 8 g + k <-> element [i = g][j = k] of the step's K x K
//   tile (the order it has in memory).  The row softmax, log Q and the KL of a row are 8-lane DPP reductions inside group g and do
//   not depend on the chain.  The chain itself: m_{t-1} and d_{t-1} sit "on the groups" (element g on every lane of group g);
//   sum_i / max_i is an all-reduce over the eight GROUPS (lanes k, k+8, .., k+56: two DPP mirrors, permlane16_swap,
//   permlane32_swap), which leaves m_t / d_t "along the lanes" (element k on lane k of every group); picking the diagonal
//   (k == g) and one more 8-lane reduction puts it back on the groups.  No LDS, no ds_bpermute in the sweep, every group and lane
//   redundant, nothing broadcast from a single lane.  The next step's logits are fetched one step ahead from a clamped address.
// 8 < K <= 16: the same sweep as phases over an LDS struct (KV_PAR / KV_SYNC / KV_LANE0 of lgssm_vm.h), which the host
//   simulation runs as it runs regime.h.
//
// Backpointers: 4 bits per target state, one word per (b, t) - 32 bits for K <= 8, 64 bits above - written to the workspace with
// ordinary vector stores by lane 0 during the sweep.  The backtrace is done by the SAME wavefront in the same launch: a fence
// after the sweep, then the words of 64 steps are read back with one coalesced load (lane l <-> step t1 - l) and walked in
// registers (K <= 8: the word of step d by a wave-uniform __shfl) or from LDS (K > 8); path is written coalesced.
#pragma once
#include "regime.h"
#include "regime_grid.h"

#if defined(KVAE_HOSTSIM)
#define KV_DECODE_FENCE() ((void)0)
#else
#define KV_DECODE_FENCE() __threadfence()
#endif

namespace kvae {
namespace rdec {

// ---- K <= 8: the lane grid ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fbits(float x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ float bitsf(uint32_t x) { return __builtin_bit_cast(float, x); }
// a product that is never contracted into the first addition of the reduction it feeds: there fma(a, b, partner's product)
// would round differently on the two partner lanes, and the copies every group keeps of one value would drift apart
#if defined(KVAE_HOSTSIM)
inline float mul(float a, float b) { return a * b; }
#else
__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
#endif
// lane ^ 8: row_mirror (l -> 15 - l) then row_half_mirror (l -> l ^ 7)
__device__ __forceinline__ float xor8(float x) { return rgrid::dpp<0x141>(rgrid::dpp<0x140>(x)); }
// all-reduce over the eight groups (lanes k, k + 8, .., k + 56), the result on every one of them.  OP: 0 sum, 1 max, 2 min
template <int OP>
__device__ __forceinline__ float op2(float a, float b) { return OP == 0 ? a + b : (OP == 1 ? fmaxf(a, b) : fminf(a, b)); }
template <int OP>
__device__ __forceinline__ float xg8(float x) {
  x = op2<OP>(x, xor8(x));
  auto a = __builtin_amdgcn_permlane16_swap(fbits(x), fbits(x), false, false);
  x = op2<OP>(bitsf(a[0]), bitsf(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(fbits(x), fbits(x), false, false);
  return op2<OP>(bitsf(b[0]), bitsf(b[1]));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t oct_or(uint32_t x) {   // over the 8 lanes of a group
  x |= dpp_u<0xB1>(x);
  x |= dpp_u<0x4E>(x);
  x |= dpp_u<0x141>(x);
  return x;
}

// log_softmax and softmax over the 8 lanes of a group (v = -inf on the lanes past K).  The log-sum-exp is log1p of the sum over
// all lanes but the (first) maximum, whose term is exactly 1: where one state dominates, log(1 + r) taken from the rounded sum
// 1 + r loses r's digits - an absolute 6e-8 on a log-probability that may itself be 1e-2 - and the restated equations in float64
// are what the outputs are held to per slice.
struct LogSoft {
  float ls, p;
};
__device__ __forceinline__ LogSoft log_soft(float v, int k, bool vk) {
  const float mx = rgrid::oct_max(v);
  const float first = rgrid::oct_min(v == mx ? (float)k : 99.0f);
  const float ex = vk ? expf(v - mx) : 0.0f;
  const float r = rgrid::oct_sum((float)k == first ? 0.0f : ex);
  LogSoft o;
  o.ls = (v - mx) - log1pf(r);
  o.p = ex / (1.0f + r);
  return o;
}

// The backtrace over the T words of one sequence (4 bits per target state), from the state st of step T - 1: 64 steps at a time, the
// words read back with one coalesced load (lane l <-> step t1 - l, step 0 has no word to follow), walked in registers by a
// wave-uniform __shfl; emit(step, state) is then called on the lane that holds the step.  Shared with the Viterbi decoder of the
// switching model (csrc/lgssm_swv.h).
template <class Emit>
__device__ __forceinline__ void walk_back(const uint32_t *bp, int T, int st, int lane, Emit &&emit) {
  for (int t1 = T - 1; t1 >= 0; t1 -= 64) {   // lane l <-> step t1 - l
    const int tl = t1 - lane, n = t1 + 1 < 64 ? t1 + 1 : 64;
    const uint32_t w = tl >= 1 ? bp[tl] : 0u;   // step 0 has no word
    int mine = 0;
    for (int d = 0; d < n; ++d) {              // wave-uniform trip count and source lane
      if (lane == d) mine = st;
      const uint32_t wd = fbits(__shfl(bitsf(w), d, 64));
      st = (int)((wd >> (4 * st)) & 15u);       // s_{t-1} = bp_t[s_t]
    }
    if (tl >= 0) emit(tl, mine);
  }
}

// bp: the sequence's T backpointer words (NULL unless path is requested)
__device__ __forceinline__ void decode_grid(const float *__restrict__ logits, const float *__restrict__ init_logits,
                                            const float *__restrict__ Pm, float *__restrict__ marginals, int32_t *__restrict__ path,
                                            float *__restrict__ path_logq, float *__restrict__ kl, uint32_t *bp, int b, int T, int K) {
  const int lane = threadIdx.x & 63, k = lane & 7, g = lane >> 3;
  const bool vk = k < K, vg = g < K, ve = vk && vg, diag = k == g;
  const bool want_m = marginals || kl, want_v = path || path_logq;
  const int KK = K * K, e = ve ? g * K + k : 0, kc = vk ? k : 0;
  const float log_uniform = logf(1.0f / (float)K);
  const float lP = logf(fmaxf(Pm[e], 1e-8f));
  const int64_t q0 = (int64_t)b * T;
  // ---- step 0 (along the lanes) ----
  const float l0 = init_logits[(int64_t)b * K + kc];
  // operands of step 1, in flight during step 0
  int64_t qn = q0 + (T > 1 ? 1 : 0);
  float Ln = logits[qn * KK + e];
  const LogSoft f0 = log_soft(vk ? l0 : -INFINITY, k, vk);
  const float ls0 = f0.ls;
  float mA = f0.p, dA = vk ? ls0 : -INFINITY;
  if (want_m) {
    const float kl0 = rgrid::oct_sum(vk ? mul(mA, ls0 - log_uniform) : 0.0f);
    if (marginals && lane < K) marginals[q0 * K + lane] = mA;
    if (kl && lane == 0) kl[q0] = kl0;
  }
  // on the groups: element g on every lane of group g (0 / -inf on the groups past K)
  float mG = rgrid::oct_sum(diag ? mA : 0.0f), dG = rgrid::oct_max(diag ? dA : -INFINITY);
  for (int t = 1; t < T; ++t) {
    const int64_t q = q0 + t;
    const float v = vk ? (vg ? Ln : 0.0f) : -INFINITY;   // a group past K works on a row of zeros, unused
    qn = q + (t + 1 < T ? 1 : 0);
    Ln = logits[qn * KK + e];
    // row g of Q_t and of log Q_t: independent of the chain
    const LogSoft f = log_soft(v, k, vk);
    const float lq = f.ls, Q = f.p;
    if (want_m) {
      const float klrow = rgrid::oct_sum(ve ? mul(Q, lq - lP) : 0.0f);
      const float klt = xg8<0>(mul(mG, klrow));                 // sum_g m_{t-1}[g] klrow[g]
      mA = xg8<0>(ve ? mul(mG, Q) : 0.0f);                      // m_t[k]
      if (marginals && lane < K) marginals[q * K + lane] = mA;
      if (kl && lane == 0) kl[q] = klt;
      mG = rgrid::oct_sum(diag ? mA : 0.0f);
    }
    if (want_v) {
      const float cand = ve ? dG + lq : -INFINITY;
      dA = xg8<1>(cand);                                     // d_t[k]
      if (bp) {
        const float arg = xg8<2>((ve && cand == dA) ? (float)g : 99.0f);   // the lowest i among the maxima
        const uint32_t word = oct_or(vk ? (uint32_t)arg << (4 * k) : 0u);
        if (lane == 0) bp[t] = word;
      }
      dG = rgrid::oct_max(diag ? dA : -INFINITY);
    }
  }
  if (!want_v) return;
  const float best = rgrid::oct_max(dA);
  if (path_logq && lane == 0) path_logq[b] = best;
  if (!path) return;
  const int st = (int)rgrid::oct_min((vk && dA == best) ? (float)k : 99.0f);
  KV_DECODE_FENCE();   // the words lane 0 stored, visible to the loads of every lane below
  walk_back(bp, T, st, lane, [&](int tl, int mine) { path[q0 + tl] = mine; });
}

// ---- 8 < K <= 16: phases over LDS --------------------------------------------------------------------------------------------
struct DecodeLds {
  float Lt[KVAE_REGIME_MAX_K * KVAE_REGIME_MAX_K], Q[KVAE_REGIME_MAX_K * KVAE_REGIME_MAX_K];
  float lq[KVAE_REGIME_MAX_K * KVAE_REGIME_MAX_K], lP[KVAE_REGIME_MAX_K * KVAE_REGIME_MAX_K];
  float l[KVAE_REGIME_MAX_K], m[KVAE_REGIME_MAX_K], mn[KVAE_REGIME_MAX_K], d[KVAE_REGIME_MAX_K], dn[KVAE_REGIME_MAX_K];
  float klr[KVAE_REGIME_MAX_K], mx[KVAE_REGIME_MAX_K], lse[KVAE_REGIME_MAX_K], rs[KVAE_REGIME_MAX_K];
  int32_t arg[KVAE_REGIME_MAX_K], pth[64];
  uint64_t bp[64];
};

// max and log1p(sum over all elements but the first maximum of exp(v - max)) of a K-vector in LDS (see log_soft)
KV_DEV void lse1p_of(const float *v, int K, float *mx_out, float *l1p_out, float *r_out) {
  float mx = v[0];
  int arg = 0;
  for (int k = 1; k < K; ++k)
    if (v[k] > mx) { mx = v[k]; arg = k; }
  float r = 0.f;
  for (int k = 0; k < K; ++k)
    if (k != arg) r += expf(v[k] - mx);
  *mx_out = mx;
  *l1p_out = log1pf(r);
  *r_out = r;
}

KV_DEV void decode_body(const float *logits, const float *init_logits, const float *Pm, float *marginals, int32_t *path,
                        float *path_logq, float *kl, uint64_t *bp, int b, int T, int K, DecodeLds &L) {
  const bool want_m = marginals || kl, want_v = path || path_logq;
  const int KK = K * K;
  const int64_t q0 = (int64_t)b * T;
  KV_PAR(e, KK) { L.lP[e] = logf(fmaxf(Pm[e], 1e-8f)); }
  KV_PAR(j, K) { L.l[j] = init_logits[(int64_t)b * K + j]; }
  Prefetch<KVAE_REGIME_MAX_K * KVAE_REGIME_MAX_K> pf_l;   // the next step's logits, one step ahead (regime.h)
  if (T > 1) pf_l.issue(logits + (q0 + 1) * KK, KK);
  KV_SYNC();
  KV_PAR(j, K) {
    float mx, lse, r;
    lse1p_of(L.l, K, &mx, &lse, &r);
    const float ls = (L.l[j] - mx) - lse;
    const float mj = expf(L.l[j] - mx) / (1.0f + r);
    L.m[j] = mj;
    L.d[j] = ls;
    L.klr[j] = mj * (ls - logf(1.0f / (float)K));
    if (marginals) marginals[q0 * K + j] = mj;
  }
  KV_SYNC();
  if (kl) {
    KV_LANE0 {
      float acc = 0.f;
      for (int j = 0; j < K; ++j) acc += L.klr[j];
      kl[q0] = acc;
    }
  }
  for (int t = 1; t < T; ++t) {
    const int64_t q = q0 + t;
    pf_l.commit(L.Lt, KK);
    KV_SYNC();   // also: the previous step's readers of klr / m / d are done
    if (t + 1 < T) pf_l.issue(logits + (q + 1) * KK, KK);
    KV_PAR(i, K) { lse1p_of(L.Lt + i * K, K, &L.mx[i], &L.lse[i], &L.rs[i]); }
    KV_SYNC();
    KV_PAR(e, KK) {
      const int i = e / K;
      L.lq[e] = (L.Lt[e] - L.mx[i]) - L.lse[i];
      L.Q[e] = expf(L.Lt[e] - L.mx[i]) / (1.0f + L.rs[i]);
    }
    KV_SYNC();
    if (want_m) {
      KV_PAR(j, K) {
        float acc = 0.f;
        for (int i = 0; i < K; ++i) acc = fmaf(L.m[i], L.Q[i * K + j], acc);
        L.mn[j] = acc;
      }
      KV_PAR(i, K) {
        float acc = 0.f;
        for (int j = 0; j < K; ++j) acc = fmaf(L.Q[i * K + j], L.lq[i * K + j] - L.lP[i * K + j], acc);
        L.klr[i] = acc;
      }
    }
    if (want_v) {
      KV_PAR(j, K) {
        float best = -INFINITY;
        int arg = 0;
        for (int i = 0; i < K; ++i) {
          const float c = L.d[i] + L.lq[i * K + j];
          if (c > best) { best = c; arg = i; }   // strict: the lowest i among the maxima
        }
        L.dn[j] = best;
        L.arg[j] = arg;
      }
    }
    KV_SYNC();
    KV_LANE0 {
      if (kl) {
        float acc = 0.f;
        for (int i = 0; i < K; ++i) acc = fmaf(L.m[i], L.klr[i], acc);
        kl[q] = acc;
      }
      if (bp) {
        uint64_t word = 0;
        for (int j = 0; j < K; ++j) word |= (uint64_t)L.arg[j] << (4 * j);
        bp[t] = word;
      }
    }
    KV_SYNC();
    KV_PAR(j, K) {
      if (want_m) {
        L.m[j] = L.mn[j];
        if (marginals) marginals[q * K + j] = L.mn[j];
      }
      if (want_v) L.d[j] = L.dn[j];
    }
    KV_SYNC();
  }
  if (!want_v) return;
  float best = -INFINITY;   // every lane, redundantly: the walk below needs the state in all of them
  int st = 0;
  for (int j = 0; j < K; ++j)
    if (L.d[j] > best) { best = L.d[j]; st = j; }
  if (path_logq) {
    KV_LANE0 { path_logq[b] = best; }
  }
  if (!path) return;
  KV_DECODE_FENCE();
  for (int t1 = T - 1; t1 >= 0; t1 -= 64) {   // slot l <-> step t1 - l
    const int n = t1 + 1 < 64 ? t1 + 1 : 64;
    KV_PAR(l, n) { L.bp[l] = t1 - l >= 1 ? bp[t1 - l] : 0; }
    KV_SYNC();
    for (int d = 0; d < n; ++d) {
      KV_LANE0 { L.pth[d] = st; }
      st = (int)((L.bp[d] >> (4 * st)) & 15ull);
    }
    KV_SYNC();
    KV_PAR(l, n) { path[q0 + t1 - l] = L.pth[l]; }
    KV_SYNC();
  }
}

// ---- what both entry points (kvae_lgssm_decode.hip, the host simulation below) share ----------------------------------------
inline int64_t decode_ws_bytes(int64_t B, int32_t T, int32_t K) {
  if (B < 1 || T < 1 || K < 1 || K > KVAE_REGIME_MAX_K) return 0;
  return B * (int64_t)T * (K <= 8 ? 4 : 8);
}
inline int decode_check(const float *logits, const float *init_logits, const float *P, const int32_t *path, const float *path_logq,
                        const void *ws, int32_t B, int32_t T, int32_t K) {
  if (!logits || !init_logits || !P) return KVAE_ERR_NULL;
  if (B < 1 || T < 1 || K > KVAE_REGIME_MAX_K) return KVAE_ERR_DIMS;
  if (K < 1) return KVAE_ERR_ARG;
  if ((path || path_logq) && !ws) return KVAE_ERR_NULL;
  return KVAE_OK;
}

}  // namespace rdec
}  // namespace kvae

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_regime_decode (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) --------------------
// The lane-grid body on emulated wavefronts, the LDS body as the host simulation runs every KV_PAR body (one sequence after the
// other, KV_PAR a serial loop); launches are counted per body so that tests can assert which one ran.  Include this header with
// KVAE_WAVE_EMU in ONE translation unit per binary (the definitions below are not inline).
#include <memory>

namespace kvae {
namespace rdec {
inline int *emu_launches() {
  static int n[2] = {0, 0};   // 0 lane grid, 1 LDS body
  return n;
}
}  // namespace rdec
}  // namespace kvae

extern "C" int64_t kvae_regime_decode_ws_bytes(int64_t B, int32_t T, int32_t K) { return kvae::rdec::decode_ws_bytes(B, T, K); }
extern "C" int kvae_regime_decode(const float *logits, const float *init_logits, const float *P, float *marginals, int32_t *path,
                                  float *path_logq, float *kl, void *ws, int32_t B, int32_t T, int32_t K, void *) {
  using namespace kvae::rdec;
  const int rc = decode_check(logits, init_logits, P, path, path_logq, ws, B, T, K);
  if (rc) return rc;
  if (K <= 8) {
    emu_launches()[0] += 1;
    wemu::launch((unsigned)B, [&] {
      const int b = (int)blockIdx.x;
      decode_grid(logits, init_logits, P, marginals, path, path_logq, kl, path ? (uint32_t *)ws + (int64_t)b * T : nullptr, b, T, K);
    });
    return KVAE_OK;
  }
  emu_launches()[1] += 1;
  auto L = std::make_unique<DecodeLds>();
  for (int b = 0; b < B; ++b) {
    memset(L.get(), 0xFF, sizeof(*L));
    decode_body(logits, init_logits, P, marginals, path, path_logq, kl, path ? (uint64_t *)ws + (int64_t)b * T : nullptr, b, T, K, *L);
  }
  return KVAE_OK;
}
extern "C" int kvae_wemu_regime_decode_launches(int which) { return which == 0 || which == 1 ? kvae::rdec::emu_launches()[which] : -1; }
#endif
