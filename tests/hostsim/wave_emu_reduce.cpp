// wave_emu_reduce.cpp — TEST-ONLY: the reduction and streaming kernels that run in every training step of every preset, the
// very __global__ functions of the product, on emulated workgroups (wave_emu.h) over host pointers:
//   csrc/rnn_wgrad.h     k_rnn_wgrad_partial<RT> (RT = 1, 4, 10, 13, 16; 16x16x4 MFMA, LDS staging) / k_rnn_wgrad_final
//   csrc/mix_wave.h      mixw::k_mix_fwd_wave<KMAX, EJ> / k_mix_bwd_wave<KMAX, EJ> / k_mix_bwd_fold
//   csrc/small_linear.h  k_linear_fwd / k_linear_softmax_fwd / k_linear_bwd_input / k_linear_softmax_bwd_input (dynamic LDS)
// The grids, chunks, slabs and LDS sizes come from the geometry functions of those headers - the ones kvae_lgssm_rnn.hip and
// kvae_lgssm.hip call - with caps that a test may lower (kvae_wemu_wgrad_max_chunks, ...), so that the multi-stage chunks, the
// capped slabs and the 32 / 64 rows per block of the large presets run at a few hundred rows.  hostsim.cpp routes kvae_rnn_wgrad,
// kvae_mix_fwd/bwd and kvae_linear_fwd/bwd_input here when kvae_hostsim_wave_emu(1) was called; every launch is counted per
// kernel instance (kvae_wemu_rnn_launches, indices below).
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../include/kvae_lgssm.h"
#include "../../kalman-vae_amd/csrc/mix_wave.h"
#include "../../kalman-vae_amd/csrc/rnn_wgrad.h"
#include "../../kalman-vae_amd/csrc/small_linear.h"

using namespace kvae;

static_assert(sizeof(kvae_wgrad_problem) == sizeof(WgradProblem), "C-ABI struct and kernel struct must agree");

extern "C" void kvae_wemu_rnn_note(int which);   // wave_emu_rnn.cpp: the launch counters

// indices of kvae_wemu_rnn_launches (0 .. 9: wave_emu_rnn.cpp)
enum {
  kWgPartial = 10,   // + 0 .. 4: k_rnn_wgrad_partial<1 | 4 | 10 | 13 | 16>
  kWgFinal = 15,
  kMixFwd = 16,      // + 0 .. 5: k_mix_fwd_wave<4,1 | 4,2 | 4,3 | 8,1 | 8,2 | 8,3>
  kMixBwd = 22,      // + 0 .. 5: k_mix_bwd_wave, the same instances
  kMixFold = 28,
  kLinFwd = 29, kLinSoftmaxFwd = 30, kLinBwd = 31, kLinSoftmaxBwd = 32,
};
static int rt_slot(int rt) { return rt == 1 ? 0 : (rt == 4 ? 1 : (rt == 10 ? 2 : (rt == 13 ? 3 : 4))); }
static int mix_slot(int km, int ej) { return (km == 4 ? 0 : 3) + ej - 1; }

// the arguments the product passes as its constants, settable here
static int g_wg_max_chunks = WG_MAX_CHUNKS, g_wg_fill = WG_FILL;
static int g_mix_fwd_max_slabs = mixw::FWD_MAX_SLABS, g_mix_bwd_max_slabs = mixw::MAX_SLABS;
static int g_sl_min_blocks = SL_MIN_BLOCKS;

static int swap_setting(int &slot, int v, int dflt) {   // v < 0: back to the product's constant; returns the previous value
  const int was = slot;
  slot = v < 0 ? dflt : v;
  return was;
}

extern "C" {

int kvae_wemu_wgrad_max_chunks(int v) { return swap_setting(g_wg_max_chunks, v, WG_MAX_CHUNKS); }
int kvae_wemu_wgrad_fill(int v) { return swap_setting(g_wg_fill, v, WG_FILL); }
int kvae_wemu_mix_fwd_max_slabs(int v) { return swap_setting(g_mix_fwd_max_slabs, v, mixw::FWD_MAX_SLABS); }
int kvae_wemu_mix_bwd_max_slabs(int v) { return swap_setting(g_mix_bwd_max_slabs, v, mixw::MAX_SLABS); }
int kvae_wemu_linear_min_blocks(int v) { return swap_setting(g_sl_min_blocks, v, SL_MIN_BLOCKS); }

int64_t kvae_wemu_wgrad_ws_floats(const kvae_wgrad_problem *probs, int32_t n) { return wg_ws_floats(probs, n, g_wg_max_chunks); }

// kvae_rnn_launch_wgrad of kvae_lgssm_rnn.hip
int kvae_wemu_wgrad(const kvae_wgrad_problem *probs, int32_t n, float *ws) {
  WgradBatch batch;
  batch.n = n;
  for (int i = 0; i < n; ++i) {
    const int bad = wg_check(probs[i]);
    if (bad) return bad == 1 ? KVAE_ERR_NULL : KVAE_ERR_ARG;
    memcpy(&batch.p[i], &probs[i], sizeof(WgradProblem));
  }
  const WgGeom g = wg_geometry(probs, n, g_wg_max_chunks, g_wg_fill);
  const wemu::Dim3 grid = {(unsigned)g.chunks, (unsigned)g.groups, (unsigned)n};
  kvae_wemu_rnn_note(kWgPartial + rt_slot(g.rt));
#define KVAE_WGRAD_PARTIAL(RT) wemu::launch_wg(grid, 256, 0, [&] { k_rnn_wgrad_partial<RT>(batch, ws, g.stride, g.chunks); })
  KVAE_WGRAD_DISPATCH(g.rt, KVAE_WGRAD_PARTIAL);
#undef KVAE_WGRAD_PARTIAL
  kvae_wemu_rnn_note(kWgFinal);
  wemu::launch_wg({(unsigned)g.final_blocks, (unsigned)n, 1}, 256, 0, [&] { k_rnn_wgrad_final(batch, ws, g.stride, g.chunks); });
  return KVAE_OK;
}

// kvae_mix_fwd / kvae_mix_bwd of kvae_lgssm.hip: 1 when the streaming kernels ran, 0 when the gate sends the call to the
// element-wise kernels (the caller's plain-loop twins)
int kvae_wemu_mix_fwd(const float *alpha, const float *base, float *out, int64_t rows, int32_t K, int32_t E) {
  if (!mixw::mix_wave_ok(alpha, base, out, K, E)) return 0;
  const mixw::MixGeom geo = mixw::mix_fwd_geometry(rows, g_mix_fwd_max_slabs);
#define KVAE_MIXW_FWD(KM, EJ)                  \
  kvae_wemu_rnn_note(kMixFwd + mix_slot(KM, EJ)), \
      wemu::launch_wg({geo.blocks, 1, 1}, 256, 0, [&] { mixw::k_mix_fwd_wave<KM, EJ>(alpha, base, out, rows, K, E, geo.per); })
  KVAE_MIXW_DISPATCH(KVAE_MIXW_FWD);
#undef KVAE_MIXW_FWD
  return 1;
}
int kvae_wemu_mix_bwd(const float *alpha, const float *base, const float *g_out, float *g_alpha, float *g_base, float *partials,
                      int64_t rows, int32_t K, int32_t E, int32_t accumulate_alpha, int64_t partials_cap) {
  if (!mixw::mix_wave_ok(alpha, base, g_out, K, E) || !mixw::aligned16(partials)) return 0;
  const mixw::MixGeom geo = mixw::mix_bwd_geometry(rows, g_mix_bwd_max_slabs, partials_cap);   // cap: kvae_mix_bwd_partials(rows)
#define KVAE_MIXW_BWD(KM, EJ)                                                                                             \
  kvae_wemu_rnn_note(kMixBwd + mix_slot(KM, EJ)), wemu::launch_wg({geo.blocks, 1, 1}, 256, 0, [&] {                          \
    mixw::k_mix_bwd_wave<KM, EJ>(alpha, base, g_out, g_alpha, partials, rows, K, E, geo.per, geo.nslab, accumulate_alpha); \
  })
  KVAE_MIXW_DISPATCH(KVAE_MIXW_BWD);
#undef KVAE_MIXW_BWD
  kvae_wemu_rnn_note(kMixFold);
  wemu::launch_wg({mixw::mix_fold_blocks(K, E), 1, 1}, 256, 0, [&] { mixw::k_mix_bwd_fold(partials, g_base, geo.nslab, K * E); });
  return 1;
}

// kvae_rnn_launch_linear_fwd / kvae_rnn_launch_linear_bwd_input of kvae_lgssm_rnn.hip
void kvae_wemu_linear_fwd(const float *x, int64_t xs, int64_t N, int F, const float *W, const float *b, int O, int softmax,
                          float *y) {
  const int rows = sl_rows_per_block(F, O, N, g_sl_min_blocks);
  const size_t lds = sizeof(float) * sl_fwd_lds_floats(F, O, rows);
  const wemu::Dim3 grid = {(unsigned)sl_fwd_blocks(N, rows), 1, 1};
  kvae_wemu_rnn_note(softmax ? kLinSoftmaxFwd : kLinFwd);
  if (softmax)
    wemu::launch_wg(grid, 256, lds, [&] { k_linear_softmax_fwd(x, xs, N, F, W, b, O, y, rows); });
  else
    wemu::launch_wg(grid, 256, lds, [&] { k_linear_fwd(x, xs, N, F, W, b, O, y, rows); });
}
void kvae_wemu_linear_bwd_input(const float *g, const float *y, int64_t N, int F, const float *W, int O, float *g_logit, float *dx,
                                int64_t dxs) {
  const size_t lds = sizeof(float) * sl_bwd_lds_floats(F, O);
  const wemu::Dim3 grid = {(unsigned)sl_bwd_blocks(N, F), 1, 1};
  kvae_wemu_rnn_note(y ? kLinSoftmaxBwd : kLinBwd);
  if (y)
    wemu::launch_wg(grid, 256, lds, [&] { k_linear_softmax_bwd_input(g, y, N, F, W, O, g_logit, dx, dxs); });
  else
    wemu::launch_wg(grid, 256, lds, [&] { k_linear_bwd_input(g, N, F, W, O, dx, dxs); });
}
// rows per block the forward takes at the current setting (what a case asserts next to the counter)
int kvae_wemu_linear_rows_per_block(int F, int O, int64_t N) { return sl_rows_per_block(F, O, N, g_sl_min_blocks); }
}
