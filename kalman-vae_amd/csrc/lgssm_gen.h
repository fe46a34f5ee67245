// lgssm_gen.h — sampled futures of the learned dynamics (include/kvae_lgssm.h kvae_lgssm_generate, KVAE.generate): the whole
// closed-loop rollout (alpha-network cell -> head -> softmax | regime step -> mixing -> state update -> emission, H times) for G
// rollouts in ONE one-wavefront workgroup.
//
// Layout.  The G rollouts of a wavefront share every weight.  The LSTM cell runs unit-major: lane j < 50 owns hidden unit j of
// all G rollouts, its four gate rows (i|f|g|o, torch order) sit in LDS as one 16-byte word per input (W[k][j]), and the cell
// inputs [y | h | 1] of the G rollouts sit in LDS as xin[k][r] (read as a broadcast).  So the gates of (rollout, unit) land in
// ONE lane and the cell update needs no exchange; the new h goes back to xin.  The head, the softmax / regime step and the
// state update run item-major: lane l takes items l, l + 64, ... of (rollout, output) pairs and reads z, alpha, h from LDS.
// The mode matrices stay in global memory (read-only, cached: the same few KB for every wavefront).  Nothing is exchanged
// across lanes except through LDS and __syncthreads, so the body runs unchanged on the wavefront emulator
// (tests/hostsim/wave_emu.h: one-wavefront workgroups, __syncthreads = wave rendezvous).
//
// No per-lane arrays are indexed at run time (the G accumulators are unrolled at compile time), so nothing lives in scratch.
// Noise is read from the caller's buffers; a NULL buffer drops the term.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/kvae_lgssm.h"

namespace kvae_gen {

constexpr int HID = 50;                 // alpha-network units the cell is built for (KVAEConfig default)
constexpr int PI = 2;                   // its input: a_dim
constexpr int KI = PI + HID + 1;        // cell inputs [y | h | 1] (the bias is the weight of the constant input)
constexpr int MAXD = KVAE_MAX_DIM, MAXK = 16;

typedef float f4 __attribute__((ext_vector_type(4)));

template <int G, bool CELL>
struct Lds {
  f4 W[CELL ? KI : 1][HID];     // gate rows of unit j for input k: (i, f, g, o)
  float xin[KI][G];             // cell inputs of the G rollouts
  float hw[CELL ? MAXK : 1][HID + 1];   // head weights | bias
  float w[G][MAXK];             // alpha_h / s_h of the step
  float wn[G][MAXK];            // regime step: pi_h before the draw
  float z[2][G][MAXD];          // z_{h-1} / z_h (ping-pong)
};

__device__ __forceinline__ float gen_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// NC, MC: compile-time n, m (0 = read from the problem).  G rollouts per wavefront.
template <int G, int NC, int MC, bool SWITCH>
__device__ void generate_wave(const kvae_gen_problem &P, Lds<G, !SWITCH> &L) {
  constexpr bool CELL = !SWITCH;
  const int n = NC ? NC : P.n, m = MC ? MC : P.m, p = P.p, K = P.K, S = P.S, H = P.H;
  const int64_t R = (int64_t)P.B * S;
  const int lane = (int)(threadIdx.x & 63);
  const int64_t r0 = (int64_t)blockIdx.x * G;
  const bool cell = CELL && K > 1;
  auto seq_of = [&](int r) -> int64_t { return r0 + r < R ? (r0 + r) / S : -1; };

  // ---- hand-over from the conditioning filter ----
  if (cell) {
    for (int idx = lane; idx < KI * HID; idx += 64) {
      const int k = idx / HID, j = idx % HID;
      f4 v;
      for (int q = 0; q < 4; ++q) {
        const int row = q * HID + j;
        v[q] = k < PI ? P.w_ih[row * PI + k] : (k < PI + HID ? P.w_hh[row * HID + (k - PI)] : P.b_ih[row] + P.b_hh[row]);
      }
      L.W[CELL ? k : 0][j] = v;
    }
    for (int idx = lane; idx < K * (HID + 1); idx += 64) {
      const int k = idx / (HID + 1), j = idx % (HID + 1);
      L.hw[CELL ? k : 0][j] = j < HID ? P.head_w[k * HID + j] : P.head_b[k];
    }
    for (int idx = lane; idx < KI * G; idx += 64) {
      const int k = idx / G, r = idx % G;
      const int64_t b = seq_of(r);
      float v = 1.0f;
      if (k < PI) v = b >= 0 ? P.y0[b * PI + k] : 0.f;
      else if (k < PI + HID) v = b >= 0 ? P.h0[b * HID + (k - PI)] : 0.f;
      L.xin[k][r] = v;
    }
  }
  for (int idx = lane; idx < G * MAXK; idx += 64) {
    const int r = idx / MAXK, k = idx % MAXK;
    const int64_t b = seq_of(r);
    L.w[r][k] = (k < K) ? (SWITCH ? (b >= 0 ? P.s0[b * K + k] : 0.f) : (K == 1 ? 1.f : 0.f)) : 0.f;
  }
  for (int idx = lane; idx < G * n; idx += 64) {
    const int r = idx / n, i = idx % n;
    const int64_t b = seq_of(r);
    float v = 0.f;
    if (b >= 0) {
      v = P.mu[b * n + i];
      if (P.eps0) {
        const float *l0 = P.L0 + b * n * n + i * n, *e0 = P.eps0 + (r0 + r) * n;
        for (int j = 0; j < n; ++j) v = fmaf(l0[j], e0[j], v);
      }
    }
    L.z[0][r][i] = v;
  }
  float c[G];   // cell state of unit `lane` for the G rollouts
#pragma unroll
  for (int r = 0; r < G; ++r) {
    const int64_t b = seq_of(r);
    c[r] = (cell && lane < HID && b >= 0) ? P.c0[b * HID + lane] : 0.f;
  }
  __syncthreads();

  for (int h = 0; h < H; ++h) {
    const int cur = h & 1, nxt = cur ^ 1;
    if (cell) {
      // ---- LSTM cell: the four gates of (rollout r, unit lane) ----
      float acc[G][4];
#pragma unroll
      for (int r = 0; r < G; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[r][q] = 0.f;
      if (lane < HID) {
        for (int k = 0; k < KI; ++k) {
          const f4 wv = L.W[CELL ? k : 0][lane];
#pragma unroll
          for (int r = 0; r < G; ++r) {
            const float x = L.xin[k][r];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] = fmaf(wv[q], x, acc[r][q]);
          }
        }
      }
      __syncthreads();   // every lane has read h_{h-1}
      if (lane < HID) {
#pragma unroll
        for (int r = 0; r < G; ++r) {
          c[r] = gen_sigmoid(acc[r][1]) * c[r] + gen_sigmoid(acc[r][0]) * tanhf(acc[r][2]);
          L.xin[PI + lane][r] = gen_sigmoid(acc[r][3]) * tanhf(c[r]);
        }
      }
      __syncthreads();
      // ---- head -> logits, softmax -> alpha_h ----
      for (int it = lane; it < G * K; it += 64) {
        const int r = it / K, k = it % K;
        const float *hw = L.hw[CELL ? k : 0];
        float lg = hw[HID];
        for (int j = 0; j < HID; ++j) lg = fmaf(hw[j], L.xin[PI + j][r], lg);
        L.wn[r][k] = lg;
      }
      __syncthreads();
      if (lane < G) {
        float mx = -INFINITY, sum = 0.f;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, L.wn[lane][k]);
        for (int k = 0; k < K; ++k) sum += expf(L.wn[lane][k] - mx);
        for (int k = 0; k < K; ++k) L.w[lane][k] = expf(L.wn[lane][k] - mx) / sum;
      }
      __syncthreads();
    } else if (SWITCH) {
      // ---- regime step: pi_h = s_{h-1} P; a Gumbel draw makes it one-hot ----
      for (int it = lane; it < G * K; it += 64) {
        const int r = it / K, k = it % K;
        float v = 0.f;
        for (int i = 0; i < K; ++i) v = fmaf(L.w[r][i], P.P[i * K + k], v);
        L.wn[r][k] = v;
      }
      __syncthreads();
      if (lane < G) {
        if (P.gumbel) {
          const float *g = P.gumbel + ((r0 + lane) * H + h) * K;
          const bool ok = r0 + lane < R;
          int best = 0;
          float top = -INFINITY;
          for (int k = 0; k < K; ++k) {
            const float sc = logf(L.wn[lane][k]) + (ok ? g[k] : 0.f);
            if (sc > top) top = sc, best = k;
          }
          for (int k = 0; k < K; ++k) L.w[lane][k] = k == best ? 1.f : 0.f;
        } else {
          for (int k = 0; k < K; ++k) L.w[lane][k] = L.wn[lane][k];
        }
      }
      __syncthreads();
    }
    // ---- z_h = sum_k w_k (A_k z + B_k u) + LQ_h eps ----
    for (int it = lane; it < G * n; it += 64) {
      const int r = it / n, i = it % n;
      const int64_t b = seq_of(r);
      const float *u = (P.U && b >= 0) ? P.U + (b * H + h) * m : nullptr;
      float v = 0.f;
      for (int k = 0; k < K; ++k) {
        const float *Ak = P.A + ((int64_t)k * n + i) * n, *Bk = P.Bm + ((int64_t)k * n + i) * m;
        float s = 0.f;
        for (int j = 0; j < n; ++j) s = fmaf(Ak[j], L.z[cur][r][j], s);
        if (u)
          for (int j = 0; j < m; ++j) s = fmaf(Bk[j], u[j], s);
        v = fmaf(L.w[r][k], s, v);
      }
      if (P.eps_z && b >= 0) {
        const float *e = P.eps_z + ((r0 + r) * H + h) * n;
        if (SWITCH) {
          for (int k = 0; k < K; ++k) {
            const float *lq = P.LQ + ((int64_t)k * n + i) * n;
            float s = 0.f;
            for (int j = 0; j <= i; ++j) s = fmaf(lq[j], e[j], s);
            v = fmaf(L.w[r][k], s, v);
          }
        } else {
          const float *lq = P.LQ + (int64_t)i * n;
          for (int j = 0; j <= i; ++j) v = fmaf(lq[j], e[j], v);
        }
      }
      L.z[nxt][r][i] = v;
      if (b >= 0) P.z_out[((r0 + r) * H + h) * n + i] = v;
    }
    __syncthreads();
    // ---- a_h = C_h z_h + LR eps_a; the weights of the step go out with it ----
    for (int it = lane; it < G * p; it += 64) {
      const int r = it / p, i = it % p;
      const int64_t b = seq_of(r);
      float v = 0.f;
      for (int k = 0; k < (SWITCH ? 1 : K); ++k) {
        const float *Ck = P.C + ((int64_t)k * p + i) * n;
        float s = 0.f;
        for (int j = 0; j < n; ++j) s = fmaf(Ck[j], L.z[nxt][r][j], s);
        v = SWITCH ? s : fmaf(L.w[r][k], s, v);
      }
      if (P.eps_a && b >= 0) {
        const float *e = P.eps_a + ((r0 + r) * H + h) * p;
        for (int j = 0; j <= i; ++j) v = fmaf(P.LR[i * p + j], e[j], v);
      }
      if (cell) L.xin[i][r] = v;   // next cell input (p == PI here)
      if (b >= 0) P.a_out[((r0 + r) * H + h) * p + i] = v;
    }
    for (int it = lane; it < G * K; it += 64) {
      const int r = it / K, k = it % K;
      if (seq_of(r) >= 0) P.w_out[((r0 + r) * H + h) * K + k] = L.w[r][k];
    }
    __syncthreads();
  }
}

// argument checks of kvae_lgssm_generate (the GPU entry point and the host simulation's below)
inline int gen_check(const kvae_gen_problem *P) {
  if (!P) return KVAE_ERR_NULL;
  const auto bad = [](int v) { return v < 1 || v > KVAE_MAX_DIM; };
  if (P->B < 1 || P->S < 1 || P->H < 1 || bad(P->n) || bad(P->m) || bad(P->p) || P->K < 1 || P->K > MAXK) return KVAE_ERR_DIMS;
  if (P->kind != 0 && P->kind != 1) return KVAE_ERR_ARG;
  if (!P->A || !P->Bm || !P->C || !P->mu || !P->a_out || !P->z_out || !P->w_out) return KVAE_ERR_NULL;
  if ((P->eps_z && !P->LQ) || (P->eps_a && !P->LR) || (P->eps0 && !P->L0)) return KVAE_ERR_NULL;
  if (P->kind == 0 && P->K > 1) {
    if (P->hidden != HID || P->p != PI) return KVAE_ERR_DIMS;
    if (!P->w_ih || !P->w_hh || !P->b_ih || !P->b_hh || !P->head_w || !P->head_b || !P->h0 || !P->c0 || !P->y0)
      return KVAE_ERR_NULL;
  }
  if (P->kind == 1) {
    if (!P->P || !P->s0) return KVAE_ERR_NULL;
    if (P->eps_z && !P->gumbel) return KVAE_ERR_ARG;
  }
  return KVAE_OK;
}

// rollouts per wavefront for R rollouts: enough wavefronts to fill the chip, as few weight copies as that allows
inline int gen_rollouts_per_wave(int64_t R) { return (R + 3) / 4 <= 768 ? 4 : 8; }

}  // namespace kvae_gen

#if defined(KVAE_WAVE_EMU)
// ---- the host simulation's kvae_lgssm_generate (TEST-ONLY: tests/hostsim/wave_emu.h defines KVAE_WAVE_EMU) -------------------
// The rollout has no generic host body: the host simulation (libkvae_hostsim.so, whose wave_emu_kernels.cpp reaches this header
// through lgssm_n16_elbo.h) runs the kernel body above on emulated wavefronts, with the grid, the rollouts per wavefront and the
// instantiations kvae_lgssm_gen.hip launches, and counts the launches so that tests can assert the emulated kernel is what ran.
// Include this header with KVAE_WAVE_EMU in ONE translation unit per binary (the definitions below are not inline).
#include <memory>

namespace kvae_gen {
inline int &emu_launches() {
  static int n = 0;
  return n;
}
template <int G, int NC, int MC, bool SWITCH>
inline void generate_emu(const kvae_gen_problem &P, unsigned grid) {
  auto L = std::make_unique<Lds<G, !SWITCH>>();   // one wavefront at a time: the LDS of the workgroup in flight
  memset(L.get(), 0xFF, sizeof(*L));
  wemu::launch(grid, [&] { generate_wave<G, NC, MC, SWITCH>(P, *L); });
}
template <int G>
inline void generate_emu_dispatch(const kvae_gen_problem &P, unsigned grid) {
  if (P.kind == 1) generate_emu<G, 0, 0, true>(P, grid);
  else if (P.n == 4 && P.m == 4) generate_emu<G, 4, 4, false>(P, grid);
  else if (P.n == 16 && P.m == 16) generate_emu<G, 16, 16, false>(P, grid);
  else generate_emu<G, 0, 0, false>(P, grid);
}
}  // namespace kvae_gen

extern "C" int kvae_lgssm_generate(const kvae_gen_problem *prob, void *) {
  const int rc = kvae_gen::gen_check(prob);
  if (rc) return rc;
  const int64_t R = (int64_t)prob->B * prob->S;
  const int G = kvae_gen::gen_rollouts_per_wave(R);
  const unsigned grid = (unsigned)((R + G - 1) / G);
  kvae_gen::emu_launches() += 1;
  if (G == 4) kvae_gen::generate_emu_dispatch<4>(*prob, grid);
  else kvae_gen::generate_emu_dispatch<8>(*prob, grid);
  return KVAE_OK;
}
extern "C" int kvae_wemu_generate_launches(void) { return kvae_gen::emu_launches(); }
#endif
