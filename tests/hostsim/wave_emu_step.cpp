// wave_emu_step.cpp — TEST-ONLY: the small kernels BETWEEN the compute kernels of every training step, the very __global__
// functions of the product, on emulated workgroups (wave_emu.h) over host pointers:
//   csrc/clip_adam.h       k_grad_sumsq / k_clip_adam (LDS trees, per-segment LDS tables, grid-stride tails)
//   csrc/vae_heads.h       k_loss_head_fwd (ONE workgroup of 1024 threads, float4 / scalar gate inside) / k_loss_head_bwd
//   csrc/colsum.h          k_colsum_v4 / k_colsum_v4_pair (512 threads, four rows in flight) / k_colsum
//   csrc/emission_means.h  k_emission_means
//   csrc/vae_epilogue.h    k_vae_epilogue_fwd_v4<1 | 2> / k_vae_epilogue_fwd / k_vae_epilogue_bwd_bias (dynamic LDS bins, LDS and
//                          global atomicAdd, blockIdx.y = chunk of samples) / k_vae_epilogue_bwd
// The path gates, grids and LDS sizes come from the geometry functions of those headers - the ones kvae_vae.hip and kvae_lgssm.hip
// call - with caps that a test may lower (kvae_wemu_epi_max_blocks, ...), so that the grid-stride rounds of the element-wise
// kernels and the chunk edges of the bias kernel run at a few thousand elements.  hostsim.cpp routes its entry points here, after
// their argument checks, when kvae_hostsim_wave_emu(1) was called; every launch is counted per kernel instance
// (kvae_wemu_rnn_launches, indices below).
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../include/kvae_lgssm.h"
#include "../../kalman-vae_amd/csrc/clip_adam.h"
#include "../../kalman-vae_amd/csrc/colsum.h"
#include "../../kalman-vae_amd/csrc/emission_means.h"
#include "../../kalman-vae_amd/csrc/vae_epilogue.h"
#include "../../kalman-vae_amd/csrc/vae_heads.h"

using namespace kvae;

extern "C" void kvae_wemu_rnn_note(int which);   // wave_emu_rnn.cpp: the launch counters

// indices of kvae_wemu_rnn_launches (0 .. 9: wave_emu_rnn.cpp, 10 .. 32: wave_emu_reduce.cpp)
enum {
  kSumsq = 33, kClipAdam = 34,
  kHeadFwd = 35, kHeadBwd = 36,
  kColsumV4 = 37, kColsumV4Pair = 38, kColsum = 39,
  kEmission = 40,
  kEpiFwdV4 = 41,   // + 0 / 1: k_vae_epilogue_fwd_v4<1 | 2>
  kEpiFwd = 43, kEpiBwdBias = 44, kEpiBwd = 45,
};

// the arguments the product passes as its constants, settable here
static int g_epi_max_blocks = (int)EPI_MAX_BLOCKS, g_epi_per_chunk = EPI_SAMPLES_PER_CHUNK;
static int g_ca_parts_cap = CA_BLOCKS, g_ca_blocks_cap = CA_MAX_BLOCKS;

static int swap_setting(int &slot, int v, int dflt) {   // v < 0: back to the product's constant; returns the previous value
  const int was = slot;
  slot = v < 0 ? dflt : v;
  return was;
}

extern "C" {

int kvae_wemu_epi_max_blocks(int v) { return swap_setting(g_epi_max_blocks, v, (int)EPI_MAX_BLOCKS); }
int kvae_wemu_epi_samples_per_chunk(int v) { return swap_setting(g_epi_per_chunk, v, EPI_SAMPLES_PER_CHUNK); }
int kvae_wemu_clip_adam_parts(int v) { return swap_setting(g_ca_parts_cap, v, CA_BLOCKS); }
int kvae_wemu_clip_adam_max_blocks(int v) { return swap_setting(g_ca_blocks_cap, v, CA_MAX_BLOCKS); }

// kvae_clip_adam of kvae_vae.hip: both launches see the same `parts`
void kvae_wemu_clip_adam(float *p, const float *g, float *m, float *v, int64_t n, const int32_t *seg_of, int32_t n_seg,
                         const float *seg_active, float *seg_steps, const float *lr_dev, float lr, float beta1, float beta2, float eps,
                         float wd, float clip, const float *div_dev, float *norm_out, float *ws) {
  const unsigned parts = ca_parts(n, g_ca_parts_cap);
  kvae_wemu_rnn_note(kSumsq);
  wemu::launch_wg({parts, 1, 1}, 256, 0, [&] { k_grad_sumsq(g, n, seg_of, n_seg, seg_active, div_dev, seg_steps, ws); });
  kvae_wemu_rnn_note(kClipAdam);
  wemu::launch_wg({ca_blocks(n, g_ca_blocks_cap), 1, 1}, 256, 0, [&] {
    k_clip_adam(p, g, m, v, n, seg_of, n_seg, seg_active, seg_steps, lr_dev, lr, beta1, beta2, eps, wd, clip, div_dev, norm_out, ws,
                (int)parts);
  });
}

// kvae_loss_head_fwd / kvae_loss_head_bwd of kvae_vae.hip
void kvae_wemu_loss_head_fwd(const float *lpx, const float *regf, const float *mask, const float *elbo_kf, const float *beta,
                             float scale, float vae_w, float kf_w, const float *w_dev, float *out, float *coef, int64_t n) {
  kvae_wemu_rnn_note(kHeadFwd);
  wemu::launch_wg({1, 1, 1}, LOSS_HEAD_FWD_THREADS, 0,
                  [&] { k_loss_head_fwd(lpx, regf, mask, elbo_kf, beta, scale, vae_w, kf_w, w_dev, out, coef, n); });
}
void kvae_wemu_loss_head_bwd(const float *g, const float *coef, const float *mask, float *g_lpx, float *g_regf, float *g_kf,
                             int64_t n) {
  kvae_wemu_rnn_note(kHeadBwd);
  wemu::launch_wg({loss_head_bwd_grid(n, g_epi_max_blocks), 1, 1}, 256, 0,
                  [&] { k_loss_head_bwd(g, coef, mask, g_lpx, g_regf, g_kf, n); });
}

// kvae_colsum / kvae_colsum2 of kvae_vae.hip
void kvae_wemu_colsum(const float *partials, float *out, int64_t rows, int64_t cols) {
  if (colsum_v4_ok(partials, out, cols)) {
    kvae_wemu_rnn_note(kColsumV4);
    wemu::launch_wg({colsum_v4_blocks(cols), 1, 1}, COLSUM_V4_THREADS, 0, [&] { k_colsum_v4(partials, out, rows, cols); });
  } else {
    kvae_wemu_rnn_note(kColsum);
    wemu::launch_wg({colsum_blocks(cols), 1, 1}, COLSUM_THREADS, 0, [&] { k_colsum(partials, out, rows, cols); });
  }
}
void kvae_wemu_colsum2(const float *pa, float *oa, int64_t rows_a, int64_t cols_a, const float *pb, float *ob, int64_t rows_b,
                       int64_t cols_b) {
  if (colsum_v4_ok(pa, oa, cols_a) && colsum_v4_ok(pb, ob, cols_b)) {
    const unsigned nb_a = colsum_v4_blocks(cols_a), nb_b = colsum_v4_blocks(cols_b);
    kvae_wemu_rnn_note(kColsumV4Pair);
    wemu::launch_wg({nb_a + nb_b, 1, 1}, COLSUM_V4_THREADS, 0,
                    [&] { k_colsum_v4_pair(pa, oa, rows_a, cols_a, nb_a, pb, ob, rows_b, cols_b); });
    return;
  }
  kvae_wemu_colsum(pa, oa, rows_a, cols_a);
  kvae_wemu_colsum(pb, ob, rows_b, cols_b);
}

// kvae_lgssm_emission_means of kvae_lgssm.hip
void kvae_wemu_emission_means(const kvae_lgssm_problem *prob, const float *ms, const float *mf, float *a_s, float *a_f) {
  const int64_t BT = (int64_t)prob->B * prob->T;
  kvae_wemu_rnn_note(kEmission);
  wemu::launch_wg({emission_blocks(BT, prob->p), 1, 1}, 256, 0,
                  [&] { k_emission_means(prob->C, ms, mf, a_s, a_f, BT, prob->T, prob->n, prob->p); });
}

// kvae_bias_shuffle_act_fwd / bwd and kvae_bias_partial_rows of kvae_vae.hip
int64_t kvae_wemu_bias_partial_rows(int64_t N) { return epi_bias_partial_rows(N, g_epi_per_chunk); }
void kvae_wemu_epilogue_fwd(const float *in, const float *bias, float *out, int64_t N, int32_t C, int32_t H, int32_t W, int32_t r,
                            int32_t relu) {
  const EpiShape s{N, C, H, W, r};
  const int64_t total = N * C * H * W * r * r;
  const int path = epi_fwd_path(in, out, W, r);
  if (path == 1) {
    kvae_wemu_rnn_note(kEpiFwdV4);
    wemu::launch_wg({epi_grid(total / 4, g_epi_max_blocks), 1, 1}, 256, 0,
                    [&] { k_vae_epilogue_fwd_v4<1>(in, bias, out, C, H, W, total / 4, relu); });
  } else if (path == 2) {
    kvae_wemu_rnn_note(kEpiFwdV4 + 1);
    wemu::launch_wg({epi_grid(total / 4, g_epi_max_blocks), 1, 1}, 256, 0,
                    [&] { k_vae_epilogue_fwd_v4<2>(in, bias, out, C, H, W, total / 4, relu); });
  } else {
    kvae_wemu_rnn_note(kEpiFwd);
    wemu::launch_wg({epi_grid(total, g_epi_max_blocks), 1, 1}, 256, 0, [&] { k_vae_epilogue_fwd(in, bias, out, s, total, relu); });
  }
}
void kvae_wemu_epilogue_bwd(const float *g_out, const float *out, float *g_in, float *bias_partials, int64_t N, int32_t C, int32_t H,
                            int32_t W, int32_t r, int32_t relu) {
  const EpiShape s{N, C, H, W, r};
  const int64_t total = N * C * H * W * r * r;
  if (bias_partials) {
    const int Cin = C * r * r;
    const int64_t chunks = epi_bias_partial_rows(N, g_epi_per_chunk);
    memset(bias_partials, 0, sizeof(float) * chunks * Cin);   // hipMemsetAsync of the entry point
    const int64_t vol = (int64_t)C * H * W * r * r;
    kvae_wemu_rnn_note(kEpiBwdBias);
    wemu::launch_wg({epi_bias_blocks_x(vol), (unsigned)chunks, 1}, 256, epi_bias_lds_bytes(Cin),
                    [&] { k_vae_epilogue_bwd_bias(g_out, out, g_in, bias_partials, s, g_epi_per_chunk, relu); });
    return;
  }
  kvae_wemu_rnn_note(kEpiBwd);
  wemu::launch_wg({epi_grid(total, g_epi_max_blocks), 1, 1}, 256, 0, [&] { k_vae_epilogue_bwd(g_out, out, g_in, s, total, relu); });
}
}
