// wave_emu_rnn.cpp — TEST-ONLY: the recurrent kernels that share the captured chain with the LGSSM sweeps, the very __global__
// functions of the product, on emulated workgroups (wave_emu.h) over host pointers:
//   csrc/lstm_fast.h    k_lstm_fwd_fast<50,2> / k_lstm_bwd_fast<50,2>     256 threads (four wavefronts) per sequence
//   csrc/gru_fast.h     k_gru_fwd_fast<50,2> (256) / k_gru_bwd_fast<50,2> (192 threads), grid (B, 2)
//   csrc/regime_grid.h  rgrid::regime_fwd / regime_bwd                    one wavefront per sequence, K <= 8
//   csrc/regime_tpp.h   k_regime_fwd_tpp<K> / k_regime_bwd_tpp<K>         one thread per sequence, K = 2..8
// hostsim.cpp routes kvae_lstm_*, kvae_bigru_*, kvae_regime_* here when kvae_hostsim_wave_emu(1) was called, behind the shape
// gates of the GPU dispatch (kvae_lgssm.hip, kvae_lgssm_tpp.hip), and every launch is counted per family (kvae_wemu_rnn_launches).
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/gru_fast.h"
#include "../../kalman-vae_amd/csrc/lstm_fast.h"
#include "../../kalman-vae_amd/csrc/regime_grid.h"
#include "../../kalman-vae_amd/csrc/regime_tpp.h"

using namespace kvae;

// launches so far: 0 / 1 LSTM fwd / bwd, 2 / 3 bi-GRU fwd / bwd, 4 / 5 regime lane-grid fwd / bwd, 6 / 7 regime thread-per-
// sequence fwd / bwd, 8 / 9 regime LDS bodies fwd / bwd (run by hostsim.cpp, noted here); 10 .. 32: the reduction, mixture and
// linear-head kernels, one index per instance (wave_emu_reduce.cpp); 33 .. 45: the optimizer, loss-head, column-sum, emission and
// conv-epilogue kernels, one index per instance (wave_emu_step.cpp); 46 .. 55: the encoder's convolution kernels, one index per
// instance (wave_emu_conv.cpp)
constexpr int kKinds = 56;
static int g_launches[kKinds] = {};
// the switches of the GPU dispatch: KVAE_REGIME_TPP (kvae_lgssm.hip: 1 lane grid up to the batch threshold, then thread per
// sequence; 2 thread per sequence always; 0 the LDS bodies) and the threshold itself, settable here so that the thread-per-
// sequence kernels run at a batch the emulation can afford
static int g_regime_mode = 1, g_regime_grid_max_b = KVAE_REGIME_GRID_MAX_B;

#define KVAE_REGIME_TPP_CASES(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)   // as kvae_lgssm_tpp.hip

// a kernel for the emulator itself: three wavefronts, a static and a dynamic LDS array, a block-wide barrier between a write
// and the read of ANOTHER wavefront's element, __shfl_xor inside the wavefront.  out[block * 192 + tid] = what the lane read.
// The lane threads persist over the blocks of a launch, so the kernel also reports what must NOT have come over from the block
// before: `fresh` counts lanes that enter with a parity counter set, or find an LDS element that is not the NaN fill.  Blocks
// leave both in a state the next one would notice: wavefront 1 of an odd block makes one exchange more than the others (its
// parity ends odd) and every lane overwrites its LDS elements.
static void k_selftest(float *out, int *fresh, int n_dyn) {
  KV_LDS(float, stat, [192]);
  KV_LDS_DYN(float, dyn);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const bool stale = wemu::t_par != 0 || wemu::t_rpar != 0 || stat[tid] == stat[tid] || (tid < n_dyn && dyn[tid] == dyn[tid]);
  if (stale) __atomic_fetch_add(fresh, 1, __ATOMIC_RELAXED);
  stat[tid] = (float)(tid + 1000 * blk);
  if (tid < n_dyn) dyn[tid] = (float)(2 * tid + blk);
  __syncthreads();
  const float other = stat[(tid + 64) % nt];                    // written by the next wavefront
  const float pair = __shfl_xor((float)tid, 1, 64);             // lane tid ^ 1 of this wavefront
  const float d = dyn[(tid + 1) % n_dyn];
  float extra = 0.f;
  if ((blk & 1) && (tid >> 6) == 1) extra = __shfl_xor((float)tid, 2, 64) - (float)(tid ^ 2);   // 0; one exchange more
  if ((tid >> 4) == 2) extra += (float)__builtin_amdgcn_mov_dpp(tid, 0x140, 0xf, 0xf, true) - (float)((tid & ~15) | (15 - (tid & 15)));
  __syncthreads();
  out[blk * nt + tid] = other + 0.5f * pair + 0.25f * d + extra + 4096.f * blockIdx.y + 16384.f * blockIdx.z;
}

extern "C" int kvae_wemu_conv_selftest(void);   // wave_emu_conv.cpp: the 32x32x2 MFMA map, raw buffer accesses, KV_LDS_RD

extern "C" {

// 0 if launch_wg, the block barrier, both kinds of LDS and __shfl_xor behave and no state of a block reaches the next one (a 3-D
// grid of 2 x 3 x 2 blocks on persistent lane threads) and the 32x32x2 MFMA map, the buffer accesses in and out of range and the
// three outcomes of an LDS read that may leave the allocation do too; the number of wrong elements otherwise
int kvae_wemu_selftest(void) {
  const int gx = 2, gy = 3, gz = 2, blocks = gx * gy * gz, nt = 192, n_dyn = 7;
  std::vector<float> out((size_t)blocks * nt, NAN);
  int fresh = 0;
  wemu::launch_wg({(unsigned)gx, (unsigned)gy, (unsigned)gz}, nt, n_dyn * sizeof(float), [&] { k_selftest(out.data(), &fresh, n_dyn); });
  int bad = fresh;
  for (int b = 0; b < blocks; ++b)
    for (int t = 0; t < nt; ++t) {
      const int by = b / gx % gy, bz = b / (gx * gy);
      const float want = (float)((t + 64) % nt + 1000 * b) + 0.5f * (float)(t ^ 1) + 0.25f * (float)(2 * ((t + 1) % n_dyn) + b) +
                         4096.f * by + 16384.f * bz;
      bad += out[(size_t)b * nt + t] != want;
    }
  return bad + kvae_wemu_conv_selftest();
}

int kvae_wemu_rnn_launches(int which) { return which >= 0 && which < kKinds ? g_launches[which] : -1; }
void kvae_wemu_rnn_note(int which) { g_launches[which] += 1; }
int kvae_wemu_regime_mode(int v) {   // < 0: back to the default; returns the previous mode
  const int was = g_regime_mode;
  g_regime_mode = v < 0 ? 1 : v;
  return was;
}
int kvae_wemu_regime_grid_max_b(int v) {   // < 0: back to the default; returns the previous threshold
  const int was = g_regime_grid_max_b;
  g_regime_grid_max_b = v < 0 ? KVAE_REGIME_GRID_MAX_B : v;
  return was;
}

void kvae_wemu_lstm_fwd(const float *x, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, float *h_seq,
                        float *gates, float *c_seq, int B, int T) {
  g_launches[0] += 1;
  wemu::launch_wg({(unsigned)B, 1, 1}, 256, 0, [&] { k_lstm_fwd_fast<50, 2>(x, w_ih, w_hh, b_ih, b_hh, h_seq, gates, c_seq, T); });
}
void kvae_wemu_lstm_bwd(const float *g_h, const float *gates, const float *c_seq, const float *w_ih, const float *w_hh,
                        float *d_pre, float *dx, int B, int T) {
  g_launches[1] += 1;
  wemu::launch_wg({(unsigned)B, 1, 1}, 256, 0, [&] { k_lstm_bwd_fast<50, 2>(g_h, gates, c_seq, w_ih, w_hh, d_pre, dx, T); });
}

void kvae_wemu_bigru_fwd(const float *x, const float *const w_ih[2], const float *const w_hh[2], const float *const b_ih[2],
                         const float *const b_hh[2], float *h_seq, float *gates, int B, int T) {
  const GruWeights wf{w_ih[0], w_hh[0], b_ih[0], b_hh[0]}, wb{w_ih[1], w_hh[1], b_ih[1], b_hh[1]};
  g_launches[2] += 1;
  wemu::launch_wg({(unsigned)B, 2, 1}, 256, 0, [&] { k_gru_fwd_fast<50, 2>(x, wf, wb, h_seq, gates, B, T); });
}
void kvae_wemu_bigru_bwd(const float *g_h, const float *gates, const float *h_seq, const float *const w_ih[2],
                         const float *const w_hh[2], float *d_pre_i, float *d_pre_h, float *dx, int B, int T) {
  const GruWeights wf{w_ih[0], w_hh[0], nullptr, nullptr}, wb{w_ih[1], w_hh[1], nullptr, nullptr};
  g_launches[3] += 1;
  wemu::launch_wg({(unsigned)B, 2, 1}, 192, 0, [&] { k_gru_bwd_fast<50, 2>(g_h, gates, h_seq, wf, wb, d_pre_i, d_pre_h, dx, B, T); });
}

// the regime chain, as kvae_regime_fwd / kvae_regime_bwd of kvae_lgssm.hip choose: returns the family launched (1 lane grid,
// 2 thread per sequence) or 0, in which case the caller runs the LDS bodies of regime.h
int kvae_wemu_regime_fwd(const float *logits, const float *init_logits, const float *gumbel, const float *P, float *y_seq,
                         float *log_q, float *log_p, int B, int T, int K, float tau, const float *tau_dev, int hard) {
  if (g_regime_mode == 1 && K <= 8 && B <= g_regime_grid_max_b) {   // kvae_grid_launch_regime_fwd + k_regime_fwd_grid
    g_launches[4] += 1;
    wemu::launch((unsigned)B, [&] {
      float tau_l = tau;
      if (tau_dev) tau_l = *tau_dev;
      rgrid::regime_fwd(logits, init_logits, gumbel, P, y_seq, log_q, log_p, blockIdx.x, T, K, tau_l, hard);
    });
    return 1;
  }
  if (g_regime_mode) {   // kvae_tpp_launch_regime_fwd
    const unsigned grid = (unsigned)((B + 63) / 64);
    switch (K) {
#define X(KC)                                                                                                                  \
  case KC:                                                                                                                     \
    g_launches[6] += 1;                                                                                                        \
    wemu::launch(grid, [&] { k_regime_fwd_tpp<KC>(logits, init_logits, gumbel, P, y_seq, log_q, log_p, B, T, tau, tau_dev, hard); }); \
    return 2;
      KVAE_REGIME_TPP_CASES(X)
#undef X
      default: break;
    }
  }
  return 0;
}
int kvae_wemu_regime_bwd(const float *logits, const float *init_logits, const float *gumbel, const float *P, const float *y_seq,
                         const float *g_y, const float *g_lq, const float *g_lp, float *g_logits, float *g_init, int B, int T, int K,
                         float tau, const float *tau_dev) {
  if (g_regime_mode == 1 && K <= 8 && B <= g_regime_grid_max_b) {   // kvae_grid_launch_regime_bwd + k_regime_bwd_grid
    g_launches[5] += 1;
    wemu::launch((unsigned)B, [&] {
      float tau_l = tau;
      if (tau_dev) tau_l = *tau_dev;
      rgrid::regime_bwd(logits, init_logits, gumbel, P, y_seq, g_y, g_lq, g_lp, g_logits, g_init, blockIdx.x, T, K, tau_l);
    });
    return 1;
  }
  if (g_regime_mode) {   // kvae_tpp_launch_regime_bwd
    const unsigned grid = (unsigned)((B + 63) / 64);
    switch (K) {
#define X(KC)                                                                                                                  \
  case KC:                                                                                                                     \
    g_launches[7] += 1;                                                                                                        \
    wemu::launch(grid, [&] { k_regime_bwd_tpp<KC>(logits, init_logits, gumbel, P, y_seq, g_y, g_lq, g_lp, g_logits, g_init, B, T, tau, tau_dev); }); \
    return 2;
      KVAE_REGIME_TPP_CASES(X)
#undef X
      default: break;
    }
  }
  return 0;
}
}
