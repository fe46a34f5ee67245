// wave_emu_kernels.cpp — TEST-ONLY: the wavefront-level LGSSM kernels of the product ((4,4,2): csrc/lgssm_m4.h over lgssm_q4.h;
// (16,16,2): csrc/lgssm_n16.h and the ELBO kernels of csrc/lgssm_n16_elbo.h), the same bodies the __global__ functions of
// kvae_lgssm_n16.hip / kvae_lgssm_elbo16.hip wrap, run on emulated wavefronts (wave_emu.h) over host pointers.  hostsim.cpp routes
// its smoother and ELBO entry points here when kvae_hostsim_wave_emu(1) was called.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_m4.h"
#include "../../kalman-vae_amd/csrc/lgssm_n16.h"
#include "../../kalman-vae_amd/csrc/lgssm_n16_elbo.h"

using namespace kvae;

// emulated launches so far (tests assert they happened): fwd n4, bwd n4, fwd n16, bwd n16, ELBO probe n16, ELBO main n16
constexpr int kLaunchKinds = 6;
static int g_launches[kLaunchKinds] = {0, 0, 0, 0, 0, 0};

template <bool HAS_FP, bool HAS_GQ>
static void bwd_n4(const kvae_lgssm_problem *p, const kvae_lgssm_states *saved, const kvae_lgssm_states *up,
                   const kvae_lgssm_input_grads *out, float *ws) {   // as launch_bwd_m4 of kvae_lgssm_n16.hip
  const unsigned grid = (unsigned)((p->B + 15) / 16);
  if (m4::kv_m4_split_bwd(*p)) {
    wemu::launch(grid, [&] { m4::smooth_bwd_wave<HAS_FP, HAS_GQ>(*p, *saved, *up, *out, ws, KV_M4_BWD_CHAIN); });
    wemu::launch(m4::kv_m4_gain_grid(*p), [&] { m4::rts_bwd_items<HAS_FP>(*p, *saved, *up, *out, ws); });
    wemu::launch(grid, [&] { m4::smooth_bwd_wave<HAS_FP, HAS_GQ>(*p, *saved, *up, *out, ws, KV_M4_BWD_FCHAIN); });
    wemu::launch(m4::kv_m4_item_grid(*p), [&] { m4::filter_bwd_items(*p, *saved, *out, ws); });
    return;
  }
  wemu::launch(grid, [&] { m4::smooth_bwd_wave<HAS_FP, HAS_GQ>(*p, *saved, *up, *out, ws, KV_M4_BWD_ALL); });
}
extern "C" {

int kvae_wemu_m4_split_max_b(int v) {   // < 0: back to the default; returns the previous override
  const int was = m4::kv_m4_split_override();
  m4::kv_m4_split_override() = v;
  return was;
}
int kvae_wemu_launches(int which) { return which >= 0 && which < kLaunchKinds ? g_launches[which] : -1; }

void kvae_wemu_fwd_n4(const kvae_lgssm_problem *p, const kvae_lgssm_states *st, int do_filter, int do_rts) {
  const unsigned grid = (unsigned)((p->B + 15) / 16);
  g_launches[0] += 1;
  if (m4::kv_m4_split(*p, do_filter, do_rts)) {   // as launch_fwd_m4 of kvae_lgssm_n16.hip: filter | all gains at once | smoother
    const unsigned gg = m4::kv_m4_gain_grid(*p);
    if (st->aux) {
      wemu::launch(grid, [&] { m4::smooth_fwd_wave<true>(*p, *st, 1, 0); });
      wemu::launch(gg, [&] { m4::gains_wave<true>(*p, *st); });
      wemu::launch(grid, [&] { m4::smooth_fwd_wave<true>(*p, *st, 0, KV_M4_RTS_WITH_GAINS); });
    } else {
      wemu::launch(grid, [&] { m4::smooth_fwd_wave<false>(*p, *st, 1, 0); });
      wemu::launch(gg, [&] { m4::gains_wave<false>(*p, *st); });
      wemu::launch(grid, [&] { m4::smooth_fwd_wave<false>(*p, *st, 0, KV_M4_RTS_WITH_GAINS); });
    }
    return;
  }
  if (st->aux) wemu::launch(grid, [&] { m4::smooth_fwd_wave<true>(*p, *st, do_filter, do_rts); });
  else wemu::launch(grid, [&] { m4::smooth_fwd_wave<false>(*p, *st, do_filter, do_rts); });
}
void kvae_wemu_bwd_n4(const kvae_lgssm_problem *p, const kvae_lgssm_states *saved, const kvae_lgssm_states *up,
                      const kvae_lgssm_input_grads *out, float *ws, int has_fp) {
  const bool gq = out->gQ.ptr != nullptr;
  g_launches[1] += 1;
  if (has_fp && gq) bwd_n4<true, true>(p, saved, up, out, ws);
  else if (has_fp) bwd_n4<true, false>(p, saved, up, out, ws);
  else if (gq) bwd_n4<false, true>(p, saved, up, out, ws);
  else bwd_n4<false, false>(p, saved, up, out, ws);
}

void kvae_wemu_fwd_n16(const kvae_lgssm_problem *p, const kvae_lgssm_states *st, int do_filter, int do_rts) {
  n16::Lds L;   // one wavefront at a time: the tile of the workgroup in flight
  memset(&L, 0xFF, sizeof(L));
  g_launches[2] += 1;
  if (st->aux) wemu::launch((unsigned)p->B, [&] { n16::smooth_fwd_wave<true>(*p, *st, do_filter, do_rts, L); });
  else wemu::launch((unsigned)p->B, [&] { n16::smooth_fwd_wave<false>(*p, *st, do_filter, do_rts, L); });
}
void kvae_wemu_bwd_n16(const kvae_lgssm_problem *p, const kvae_lgssm_states *saved, const kvae_lgssm_states *up,
                       const kvae_lgssm_input_grads *out, float *ws, int has_fp) {
  n16::Lds L;
  memset(&L, 0xFF, sizeof(L));
  const bool gq = out->gQ.ptr != nullptr;
  g_launches[3] += 1;
  if (has_fp && gq) wemu::launch((unsigned)p->B, [&] { n16::smooth_bwd_wave<true, true>(*p, *saved, *up, *out, ws, L); });
  else if (has_fp) wemu::launch((unsigned)p->B, [&] { n16::smooth_bwd_wave<true, false>(*p, *saved, *up, *out, ws, L); });
  else if (gq) wemu::launch((unsigned)p->B, [&] { n16::smooth_bwd_wave<false, true>(*p, *saved, *up, *out, ws, L); });
  else wemu::launch((unsigned)p->B, [&] { n16::smooth_bwd_wave<false, false>(*p, *saved, *up, *out, ws, L); });
}

// the ELBO of (16,16,2), as kvae_n16_launch_elbo_probe + kvae_n16_launch_elbo of kvae_lgssm_elbo16.hip: the same grids, the same
// choice between the per-step and the four-steps-per-wavefront kernels, the same instantiations.  The caller (hostsim.cpp) zeroes
// levels[0..2] first, as kvae_lgssm_elbo does.  g_mus / g_Sigs are filled with NaN before the launches (test-only): a (b,t) that
// no wavefront writes then shows up as NaN, not as whatever the buffer held.
void kvae_wemu_elbo_n16(const kvae_lgssm_problem *p, const float *mus, const float *Sigs, const float *eps, float *terms,
                        int32_t *levels, float *zst, float *g_mus, float *g_Sigs, const kvae_lgssm_input_grads *g, int have_g) {
  const int64_t steps = (int64_t)p->B * p->T;
  if (have_g) {
    for (int64_t e = 0; e < steps * n16::N; ++e) g_mus[e] = NAN;
    for (int64_t e = 0; e < steps * n16::NN; ++e) g_Sigs[e] = NAN;
  }
  const unsigned grid = (unsigned)steps, grid4 = (unsigned)((int64_t)p->B * ((p->T + 3) / 4));
  const bool shared_q = p->Q.sb == 0 && p->Q.st == 0;   // elbo_shared_q
  g_launches[4] += 1;
  if (shared_q) wemu::launch(grid4, [&] { n16::elbo_probe4_wave(*p, Sigs, mus, eps, zst, levels); });
  else wemu::launch(grid, [&] { n16::elbo_probe_wave(*p, Sigs, mus, eps, zst, levels); });
  wemu::launch(grid4, [&] { n16::elbo_zfix_wave(*p, Sigs, mus, eps, zst, levels); });
  g_launches[5] += 1;
  const kvae_lgssm_input_grads &G = *g;
  if (shared_q && !(have_g && g->gQ.ptr)) {
    n16::ELds4 L4;   // one wavefront at a time: the tile of the workgroup in flight
    memset(&L4, 0xFF, sizeof(L4));
    if (have_g) wemu::launch(grid4, [&] { n16::elbo4_wave<true>(*p, mus, Sigs, eps, terms, levels, zst, g_mus, g_Sigs, G, L4); });
    else wemu::launch(grid4, [&] { n16::elbo4_wave<false>(*p, mus, Sigs, eps, terms, levels, zst, g_mus, g_Sigs, G, L4); });
    return;
  }
  n16::ELds L;
  memset(&L, 0xFF, sizeof(L));
  if (!have_g) wemu::launch(grid, [&] { n16::elbo_wave<false, false>(*p, mus, Sigs, eps, terms, levels, zst, g_mus, g_Sigs, G, L); });
  else if (g->gQ.ptr) wemu::launch(grid, [&] { n16::elbo_wave<true, true>(*p, mus, Sigs, eps, terms, levels, zst, g_mus, g_Sigs, G, L); });
  else wemu::launch(grid, [&] { n16::elbo_wave<true, false>(*p, mus, Sigs, eps, terms, levels, zst, g_mus, g_Sigs, G, L); });
}
// 1 if the workgroup -> work-unit remap of the ELBO launches (n16::xcd_contiguous) is a permutation of 0..nwg-1
int kvae_wemu_xcd_contiguous_is_permutation(unsigned nwg) {
  std::vector<unsigned char> hit(nwg, 0);
  for (unsigned wg = 0; wg < nwg; ++wg) {
    const unsigned w = n16::xcd_contiguous(wg, nwg);
    if (w >= nwg || hit[w]) return 0;
    hit[w] = 1;
  }
  return 1;
}
}
