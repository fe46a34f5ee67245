// kvae_vae.hip — the frame VAE's hand-written kernels and the optimizer step (the callers either side of the
// section-8 path): conv epilogues and column sums (vae_epilogue.h), the fused clip + Adam step, the Bernoulli frame term
// (vae_loss.h), the direct / f32-MFMA / Winograd convolutions (vae_conv_edge.h, vae_conv_mid.h, vae_conv_up_wino.h) and the heads
// (vae_heads.h), with their C-ABI entry points.  A unit of its own since round 3: half of what used to be one 1300-line unit,
// compiled side by side with the LGSSM units (which carry per-unit scheduler flags, __graft_entry__.UNIT_FLAGS; these
// kernels - hand-placed sched_barrier pipelines at full occupancy - keep the compiler's default strategy).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/kvae_lgssm.h"

namespace kvae {}
using namespace kvae;

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH (+ kvae_last_error)
static int launch_status(const char *what) { return kvae_launch_status(what); }

// ---------------------------------------------------------------------------------------------
// column sums (colsum.h) and the fused conv epilogues of the frame VAE (vae_epilogue.h): kernels and launch geometry
// ---------------------------------------------------------------------------------------------
#include "colsum.h"
#include "vae_epilogue.h"

extern "C" int64_t kvae_bias_partial_rows(int64_t N);

extern "C" {
int kvae_bias_shuffle_act_fwd(const float *in, const float *bias, float *out, int64_t N, int32_t C, int32_t H, int32_t W,
                              int32_t r, int32_t relu, void *stream) {
  if (!in || !bias || !out) return KVAE_ERR_NULL;
  if (N < 1 || C < 1 || H < 1 || W < 1 || r < 1) return KVAE_ERR_ARG;
  const EpiShape s{N, C, H, W, r};
  const int64_t total = N * C * H * W * r * r;
  const int path = epi_fwd_path(in, out, W, r);
  if (path == 1)
    k_vae_epilogue_fwd_v4<1><<<dim3(epi_grid(total / 4)), dim3(256), 0, (hipStream_t)stream>>>(in, bias, out, C, H, W, total / 4, relu);
  else if (path == 2)
    k_vae_epilogue_fwd_v4<2><<<dim3(epi_grid(total / 4)), dim3(256), 0, (hipStream_t)stream>>>(in, bias, out, C, H, W, total / 4, relu);
  else
    k_vae_epilogue_fwd<<<dim3(epi_grid(total)), dim3(256), 0, (hipStream_t)stream>>>(in, bias, out, s, total, relu);
  return launch_status("k_vae_epilogue_fwd");
}
int kvae_bias_shuffle_act_bwd(const float *g_out, const float *out, float *g_in, float *bias_partials, int64_t N, int32_t C,
                              int32_t H, int32_t W, int32_t r, int32_t relu, void *stream) {
  if (!g_out || !g_in || (relu && !out)) return KVAE_ERR_NULL;
  if (N < 1 || C < 1 || H < 1 || W < 1 || r < 1) return KVAE_ERR_ARG;
  const EpiShape s{N, C, H, W, r};
  const int64_t total = N * C * H * W * r * r;
  hipStream_t st = (hipStream_t)stream;
  if (bias_partials) {
    const int Cin = C * r * r;
    const int64_t chunks = kvae_bias_partial_rows(N);
    if (hipMemsetAsync(bias_partials, 0, sizeof(float) * chunks * Cin, st) != hipSuccess) return launch_status("memset bias_partials");
    const int64_t vol = (int64_t)C * H * W * r * r;
    k_vae_epilogue_bwd_bias<<<dim3(epi_bias_blocks_x(vol), (unsigned)chunks), dim3(256), epi_bias_lds_bytes(Cin), st>>>(
        g_out, out, g_in, bias_partials, s, EPI_SAMPLES_PER_CHUNK, relu);
    return launch_status("k_vae_epilogue_bwd_bias");
  }
  k_vae_epilogue_bwd<<<dim3(epi_grid(total)), dim3(256), 0, st>>>(g_out, out, g_in, s, total, relu);
  return launch_status("k_vae_epilogue_bwd");
}
int kvae_colsum(const float *partials, float *out, int64_t rows, int64_t cols, void *stream) {
  if (!partials || !out) return KVAE_ERR_NULL;
  if (rows < 1 || cols < 1) return KVAE_ERR_ARG;
  if (colsum_v4_ok(partials, out, cols))
    k_colsum_v4<<<dim3(colsum_v4_blocks(cols)), dim3(COLSUM_V4_THREADS), 0, (hipStream_t)stream>>>(partials, out, rows, cols);
  else
    k_colsum<<<dim3(colsum_blocks(cols)), dim3(COLSUM_THREADS), 0, (hipStream_t)stream>>>(partials, out, rows, cols);
  return launch_status("k_colsum");
}
int kvae_colsum2(const float *pa, float *oa, int64_t rows_a, int64_t cols_a, const float *pb, float *ob, int64_t rows_b,
                 int64_t cols_b, void *stream) {
  if (!pa || !oa || !pb || !ob) return KVAE_ERR_NULL;
  if (rows_a < 1 || cols_a < 1 || rows_b < 1 || cols_b < 1) return KVAE_ERR_ARG;
  if (colsum_v4_ok(pa, oa, cols_a) && colsum_v4_ok(pb, ob, cols_b)) {
    const unsigned nb_a = colsum_v4_blocks(cols_a), nb_b = colsum_v4_blocks(cols_b);
    k_colsum_v4_pair<<<dim3(nb_a + nb_b), dim3(COLSUM_V4_THREADS), 0, (hipStream_t)stream>>>(pa, oa, rows_a, cols_a, nb_a, pb, ob, rows_b, cols_b);
    return launch_status("k_colsum_v4_pair");
  }
  const int rc = kvae_colsum(pa, oa, rows_a, cols_a, stream);
  return rc ? rc : kvae_colsum(pb, ob, rows_b, cols_b, stream);
}
int64_t kvae_bias_partial_rows(int64_t N) { return epi_bias_partial_rows(N); }
}  // extern "C"

// ---------------------------------------------------------------------------------------------
// clip_grad_norm_ + Adam on flat buffers: two launches instead of ~12 (norm, clamp, reciprocal, scale, three foreach kernels)
// ---------------------------------------------------------------------------------------------
#include "clip_adam.h"

extern "C" int kvae_clip_adam(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                              const int32_t *seg_of, int32_t n_seg, const float *seg_active, float *seg_steps, const float *lr_dev,
                              float lr, float beta1, float beta2, float eps, float weight_decay, float clip, const float *div_dev,
                              float *norm_out, float *ws, void *stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !seg_steps || !ws) return KVAE_ERR_NULL;
  if (n < 1 || n_seg < 1 || n_seg > CA_MAX_SEG || (!seg_of && n_seg != 1)) return KVAE_ERR_ARG;
  const unsigned parts = ca_parts(n);   // k_clip_adam folds the partials k_grad_sumsq leaves
  k_grad_sumsq<<<dim3(parts), dim3(256), 0, (hipStream_t)stream>>>(grads, n, seg_of, n_seg, seg_active, div_dev, seg_steps, ws);
  int rc = launch_status("k_grad_sumsq");
  if (rc) return rc;
  k_clip_adam<<<dim3(ca_blocks(n)), dim3(256), 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, seg_of, n_seg, seg_active,
                                                                   seg_steps, lr_dev, lr, beta1, beta2, eps, weight_decay, clip,
                                                                   div_dev, norm_out, ws, (int)parts);
  return launch_status("k_clip_adam");
}

// ---------------------------------------------------------------------------------------------
// fused Bernoulli reconstruction term (vae_loss.h): one wavefront per frame
// ---------------------------------------------------------------------------------------------
#include "vae_loss.h"

__global__ __launch_bounds__(256) void k_vae_bce_fwd(const float *__restrict__ logits, const float *__restrict__ x,
                                                     float *__restrict__ frame_ll, int64_t frames, int pixels) {
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= frames) return;
  const float *l = logits + f * pixels, *t = x + f * pixels;
  float acc = 0.f;
  if ((pixels & 3) == 0 && (((uintptr_t)l | (uintptr_t)t) & 15) == 0) {
    for (int i = lane * 4; i < pixels; i += 256) {
      const float4 a = *reinterpret_cast<const float4 *>(l + i), b = *reinterpret_cast<const float4 *>(t + i);
      acc += bce_logit(a.x, b.x) + bce_logit(a.y, b.y) + bce_logit(a.z, b.z) + bce_logit(a.w, b.w);
    }
  } else {
    for (int i = lane; i < pixels; i += 64) acc += bce_logit(l[i], t[i]);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) frame_ll[f] = -acc;
}

__global__ __launch_bounds__(256) void k_vae_bce_bwd(const float *__restrict__ logits, const float *__restrict__ x,
                                                     const float *__restrict__ g_frame, float *__restrict__ g_logits,
                                                     int64_t total, int pixels) {
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * 1024) {
    const float g = -g_frame[i / pixels];   // pixels % 4 == 0 on this path: the 4 elements share a frame
    const float4 a = *reinterpret_cast<const float4 *>(logits + i), b = *reinterpret_cast<const float4 *>(x + i);
    *reinterpret_cast<float4 *>(g_logits + i) = make_float4(g * (sigmoid_stable(a.x) - b.x), g * (sigmoid_stable(a.y) - b.y),
                                                            g * (sigmoid_stable(a.z) - b.z), g * (sigmoid_stable(a.w) - b.w));
  }
}
__global__ __launch_bounds__(256) void k_vae_bce_bwd_scalar(const float *logits, const float *x, const float *g_frame,
                                                            float *g_logits, int64_t total, int pixels) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    g_logits[i] = -g_frame[i / pixels] * (sigmoid_stable(logits[i]) - x[i]);
}

extern "C" {
int kvae_bce_frames_fwd(const float *logits, const float *x, float *frame_ll, int64_t frames, int32_t pixels, void *stream) {
  if (!logits || !x || !frame_ll) return KVAE_ERR_NULL;
  if (frames < 1 || pixels < 1) return KVAE_ERR_ARG;
  k_vae_bce_fwd<<<dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(logits, x, frame_ll, frames, pixels);
  return launch_status("k_vae_bce_fwd");
}
int kvae_bce_frames_bwd(const float *logits, const float *x, const float *g_frame, float *g_logits, int64_t frames,
                        int32_t pixels, void *stream) {
  if (!logits || !x || !g_frame || !g_logits) return KVAE_ERR_NULL;
  if (frames < 1 || pixels < 1) return KVAE_ERR_ARG;
  const int64_t total = frames * pixels;
  const bool v4 = (pixels & 3) == 0 && ((((uintptr_t)logits | (uintptr_t)x | (uintptr_t)g_logits) & 15) == 0);
  if (v4)
    k_vae_bce_bwd<<<dim3(epi_grid(total / 4)), dim3(256), 0, (hipStream_t)stream>>>(logits, x, g_frame, g_logits, total, pixels);
  else
    k_vae_bce_bwd_scalar<<<dim3(epi_grid(total)), dim3(256), 0, (hipStream_t)stream>>>(logits, x, g_frame, g_logits, total, pixels);
  return launch_status("k_vae_bce_bwd");
}
}  // extern "C"

#include "vae_conv_edge.h"
extern "C" {
int64_t kvae_conv_edge_partial_rows(int64_t N) { return conv_edge_partial_rows(N); }

int kvae_dec_head_fwd(const float *in, const float *W, const float *bias, float *logits, float *w_scratch, int64_t N,
                      int32_t Cin, int32_t side, void *stream) {
  if (!in || !W || !bias || !logits || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != DH_CI || side != DH_S) return KVAE_ERR_DIMS;
  k_dec_head_prep<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(W, w_scratch);
  k_dec_head_fwd<false><<<dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream>>>(in, w_scratch, bias, logits, nullptr, nullptr, nullptr);
  return launch_status("k_dec_head_fwd");
}
int kvae_dec_head_loss_fwd(const float *in, const float *W, const float *bias, const float *x, float *logits, float *x_recon,
                           float *frame_ll, float *w_scratch, int64_t N, int32_t Cin, int32_t side, void *stream) {
  if (!in || !W || !bias || !x || !logits || !frame_ll || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != DH_CI || side != DH_S) return KVAE_ERR_DIMS;
  k_dec_head_prep<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(W, w_scratch);
  k_dec_head_fwd<true><<<dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream>>>(in, w_scratch, bias, logits, x, x_recon, frame_ll);
  return launch_status("k_dec_head_loss_fwd");
}
}  // extern "C"
// one persistent launch for both gradients of the head; the gradient of the logits is read (LOSS = false) or formed from the
// Bernoulli term (LOSS = true)
template <bool LOSS>
static int dec_head_bwd_launch(const float *in, const float *W, const float *g_logits, const float *logits, const float *x,
                               const float *g_frame, float *g_in, float *w_partials, float *b_partials, float *w_scratch,
                               int64_t N, bool mask, hipStream_t st) {
  const dim3 grid((unsigned)kvae_conv_edge_partial_rows(N));
  if (g_in) {
    k_dec_head_prep<<<dim3(1), dim3(256), 0, st>>>(W, w_scratch);
    if (mask)
      k_dec_head_bwd<LOSS, true, true><<<grid, dim3(256), 0, st>>>(in, g_logits, logits, x, g_frame, w_scratch, g_in, w_partials, b_partials, N);
    else
      k_dec_head_bwd<LOSS, true><<<grid, dim3(256), 0, st>>>(in, g_logits, logits, x, g_frame, w_scratch, g_in, w_partials, b_partials, N);
  } else {
    k_dec_head_bwd<LOSS, false><<<grid, dim3(256), 0, st>>>(in, g_logits, logits, x, g_frame, w_scratch, g_in, w_partials, b_partials, N);
  }
  return launch_status("k_dec_head_bwd");
}
extern "C" {
int kvae_dec_head_bwd(const float *in, const float *W, const float *g_logits, float *g_in, float *w_partials,
                      float *b_partials, float *w_scratch, int64_t N, int32_t Cin, int32_t side, void *stream) {
  if (!in || !W || !g_logits || !w_partials || !b_partials || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != DH_CI || side != DH_S) return KVAE_ERR_DIMS;
  return dec_head_bwd_launch<false>(in, W, g_logits, nullptr, nullptr, nullptr, g_in, w_partials, b_partials, w_scratch, N, false,
                                    (hipStream_t)stream);
}
int kvae_dec_head_loss_bwd(const float *in, const float *W, const float *logits, const float *x, const float *g_frame, float *g_in,
                           float *w_partials, float *b_partials, float *w_scratch, int64_t N, int32_t Cin, int32_t side,
                           void *stream) {
  if (!in || !W || !logits || !x || !g_frame || !w_partials || !b_partials || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != DH_CI || side != DH_S) return KVAE_ERR_DIMS;
  return dec_head_bwd_launch<true>(in, W, nullptr, logits, x, g_frame, g_in, w_partials, b_partials, w_scratch, N, false,
                                   (hipStream_t)stream);
}
// the same two with g_in = in > 0 ? g_in : 0 (k_dec_head_bwd<., true, true>)
int kvae_dec_head_bwd_masked(const float *in, const float *W, const float *g_logits, float *g_in, float *w_partials,
                             float *b_partials, float *w_scratch, int64_t N, int32_t Cin, int32_t side, void *stream) {
  if (!in || !W || !g_logits || !w_partials || !b_partials || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != DH_CI || side != DH_S) return KVAE_ERR_DIMS;
  return dec_head_bwd_launch<false>(in, W, g_logits, nullptr, nullptr, nullptr, g_in, w_partials, b_partials, w_scratch, N, true,
                                    (hipStream_t)stream);
}
int kvae_dec_head_loss_bwd_masked(const float *in, const float *W, const float *logits, const float *x, const float *g_frame,
                                  float *g_in, float *w_partials, float *b_partials, float *w_scratch, int64_t N, int32_t Cin,
                                  int32_t side, void *stream) {
  if (!in || !W || !logits || !x || !g_frame || !w_partials || !b_partials || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != DH_CI || side != DH_S) return KVAE_ERR_DIMS;
  return dec_head_bwd_launch<true>(in, W, nullptr, logits, x, g_frame, g_in, w_partials, b_partials, w_scratch, N, true,
                                   (hipStream_t)stream);
}
int kvae_enc_stem_fwd(const float *x, const float *W, const float *bias, float *out, uint32_t *relu_bits, int64_t N, int32_t Cout,
                      int32_t side, void *stream) {
  if (!x || !W || !bias || !out) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cout != ES_CO || side != ES_IN) return KVAE_ERR_DIMS;
  k_enc_stem_fwd<<<dim3(es_fwd_grid(N)), dim3(256), 0, (hipStream_t)stream>>>(x, W, bias, out, relu_bits);
  return launch_status("k_enc_stem_fwd");
}
int kvae_enc_stem_bwd(const float *x, const float *out, const uint32_t *relu_bits, const float *g_out, float *w_partials,
                      float *b_partials, int64_t N, int32_t Cout, int32_t side, void *stream) {
  if (!x || (!out && !relu_bits) || !g_out || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cout != ES_CO || side != ES_IN) return KVAE_ERR_DIMS;
  static const int mfma = getenv("KVAE_STEM_MFMA") ? atoi(getenv("KVAE_STEM_MFMA")) : 1;   // 0: VALU version, 2: mask from out (A/B runs)
  const dim3 grid((unsigned)conv_edge_partial_rows(N));
  const int kernel = es_wrw_kernel(mfma, relu_bits != nullptr, out != nullptr);
  if (kernel == ES_WRW_REFUSED) return KVAE_ERR_NULL;
  if (kernel == ES_WRW_MFMA_BITS) k_enc_stem_wrw_mfma<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, out, relu_bits, g_out, w_partials, b_partials, N);
  else if (kernel == ES_WRW_MFMA_OUT) k_enc_stem_wrw_mfma<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, out, relu_bits, g_out, w_partials, b_partials, N);
  else k_enc_stem_wrw<<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, out, g_out, w_partials, b_partials, N);
  return launch_status("k_enc_stem_wrw");
}
}  // extern "C"

#include "vae_conv_mid.h"
extern "C" {
int64_t kvae_enc_mid_partial_rows(int64_t N, int32_t side) { return em_grid(N, side); }

int kvae_enc_mid_fwd(const float *in, const float *W, const float *bias, float *out, int64_t N, int32_t C, int32_t side,
                     void *stream) {
  if (!in || !W || !bias || !out) return KVAE_ERR_NULL;
  if (!em_launch_ok(N, side)) return KVAE_ERR_ARG;   // 32-bit byte offsets
  if (C != EM_C || (side != 16 && side != 8)) return KVAE_ERR_DIMS;
  const dim3 grid((unsigned)em_grid(N, side));
  if (side == 16) k_enc_mid_fwd<16><<<grid, dim3(256), 0, (hipStream_t)stream>>>(in, W, bias, out, N);
  else k_enc_mid_fwd<8><<<grid, dim3(256), 0, (hipStream_t)stream>>>(in, W, bias, out, N);
  return launch_status("k_enc_mid_fwd");
}
int kvae_enc_mid_bwd(const float *in, const float *W, const float *out, const float *g_out, float *g_in,
                     float *w_partials, float *b_partials, int64_t N, int32_t C, int32_t side, void *stream) {
  if (!in || !W || !out || !g_out || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (!em_launch_ok(N, side)) return KVAE_ERR_ARG;
  if (C != EM_C || (side != 16 && side != 8)) return KVAE_ERR_DIMS;
  const dim3 grid((unsigned)em_grid(N, side));
  if (g_in) {
    if (side == 16) k_enc_mid_bwd_data<16><<<grid, dim3(256), 0, (hipStream_t)stream>>>(W, out, g_out, g_in, N);
    else k_enc_mid_bwd_data<8><<<grid, dim3(256), 0, (hipStream_t)stream>>>(W, out, g_out, g_in, N);
    const int rc = launch_status("k_enc_mid_bwd_data");
    if (rc) return rc;
  }
  if (side == 16) k_enc_mid_wrw<16><<<grid, dim3(256), 0, (hipStream_t)stream>>>(in, out, g_out, w_partials, b_partials, N);
  else k_enc_mid_wrw<8><<<grid, dim3(256), 0, (hipStream_t)stream>>>(in, out, g_out, w_partials, b_partials, N);
  return launch_status("k_enc_mid_wrw");
}
}  // extern "C"

#include "vae_conv_up_wino.h"
static bool dec_up_wino() {
  static const int env = getenv("KVAE_WINO") ? atoi(getenv("KVAE_WINO")) : 1;   // 0: direct convolution (A/B runs)
  return env != 0;
}
// Persistent decoder-block workgroups: one per CU, or fewer (KVAE_UP_WGS) so that a second stream's kernels that do not fit
// beside them (anything above 32 registers per lane) find free CUs while they run.
static int g_dec_up_wgs = 0;   // 0: not set through kvae_dec_up_set_workgroups
static inline int64_t dec_up_cap() {
  static const int env = getenv("KVAE_UP_WGS") ? atoi(getenv("KVAE_UP_WGS")) : 0;   // the environment wins over the setter (A/B runs)
  const int v = env >= 1 && env <= 256 ? env : __atomic_load_n(&g_dec_up_wgs, __ATOMIC_RELAXED);
  return v >= 1 && v <= 256 ? v : 256;
}
static inline int64_t dec_up_grid(int64_t N, int32_t side) {
  const int64_t fpi = side == 8 ? 2 : 8, iters = (N + fpi - 1) / fpi, cap = dec_up_cap();
  return iters < cap ? (iters < 1 ? 1 : iters) : cap;
}
extern "C" {
int64_t kvae_dec_up_partial_rows(int64_t N, int32_t side) { return dec_up_grid(N, side); }
int32_t kvae_dec_up_set_workgroups(int32_t n) {
  const int32_t prev = (int32_t)dec_up_cap();
  __atomic_store_n(&g_dec_up_wgs, n >= 1 && n <= 256 ? n : 0, __ATOMIC_RELAXED);
  return prev;
}

int kvae_dec_up_fwd(const float *x, const float *W, const float *bias, float *out, int64_t N, int32_t Cin, int32_t side,
                    void *stream) {
  if (!x || !W || !bias || !out) return KVAE_ERR_NULL;
  if (N < 1 || (N + 256 * 8) * UP_CO * side * side * 4 >= EM_MAX_BYTES) return KVAE_ERR_ARG;   // 32-bit byte offsets
  if (Cin != UP_CI || (side != 8 && side != 4)) return KVAE_ERR_DIMS;
  const dim3 grid((unsigned)dec_up_grid(N, side));
  if (dec_up_wino()) {   // pairs of workgroups (one per half of the output channels) walk the column sets together
    const int64_t sets = side == 8 ? N : (N + 3) / 4;
    const dim3 wgrid((unsigned)(sets < dec_up_cap() ? sets : dec_up_cap()));
    if (side == 8) k_dec_up_fwd_wino<8><<<wgrid, dim3(512), 0, (hipStream_t)stream>>>(x, W, bias, out, N);
    else k_dec_up_fwd_wino<4><<<wgrid, dim3(512), 0, (hipStream_t)stream>>>(x, W, bias, out, N);
    return launch_status("k_dec_up_fwd_wino");
  }
  if (side == 8) k_dec_up_fwd<8><<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, W, bias, out, N);
  else k_dec_up_fwd<4><<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, W, bias, out, N);
  return launch_status("k_dec_up_fwd");
}
}  // extern "C"
// g[i] = act[i] > 0 ? g[i] : 0 in place, 16 bytes per thread: KVAE_UP_MASK_GX wherever the Winograd 8x8 data gradient does not
// apply it itself (the direct kernels of KVAE_WINO=0, the 4x4 block, a gradient that is not pre-masked) - A/B and test routes
__global__ __launch_bounds__(256) void k_relu_mask_inplace(float *__restrict__ g, const float *__restrict__ act, int64_t quads) {
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const float4 a = reinterpret_cast<const float4 *>(act)[q];
    float4 v = reinterpret_cast<float4 *>(g)[q];
    v = make_float4(a.x > 0.f ? v.x : 0.f, a.y > 0.f ? v.y : 0.f, a.z > 0.f ? v.z : 0.f, a.w > 0.f ? v.w : 0.f);
    reinterpret_cast<float4 *>(g)[q] = v;
  }
}
static int dec_up_bwd_launch(const float *x, const float *W, const float *out, const float *g_out, float *g_x, float *w_partials,
                             float *b_partials, int64_t N, int32_t side, int32_t flags, hipStream_t st) {
  const dim3 grid((unsigned)dec_up_grid(N, side));
  const bool pre = (flags & KVAE_UP_G_PREMASKED) != 0, wino = dec_up_wino();
  if (g_x) {
    const int64_t sets = side == 8 ? N : (N + 3) / 4;
    const dim3 wgrid((unsigned)(sets < dec_up_cap() ? sets : dec_up_cap()));
    bool mask_gx = (flags & KVAE_UP_MASK_GX) != 0;
    if (wino && side == 8 && pre && mask_gx) {
      k_dec_up_bwd_data_wino<8, true, true><<<wgrid, dim3(512), 0, st>>>(W, x, out, g_out, g_x, N);
      mask_gx = false;                                // done by the kernel
    } else if (wino && side == 8 && pre) k_dec_up_bwd_data_wino<8, true><<<wgrid, dim3(512), 0, st>>>(W, x, out, g_out, g_x, N);
    else if (wino && side == 8) k_dec_up_bwd_data_wino<8><<<wgrid, dim3(512), 0, st>>>(W, x, out, g_out, g_x, N);
    else if (wino && pre) k_dec_up_bwd_data_wino<4, true><<<wgrid, dim3(512), 0, st>>>(W, x, out, g_out, g_x, N);
    else if (wino) k_dec_up_bwd_data_wino<4><<<wgrid, dim3(512), 0, st>>>(W, x, out, g_out, g_x, N);
    else if (side == 8) k_dec_up_bwd_data<8><<<grid, dim3(256), 0, st>>>(W, out, g_out, g_x, N);   // the direct kernels mask again:
    else k_dec_up_bwd_data<4><<<grid, dim3(256), 0, st>>>(W, out, g_out, g_x, N);                   // the select is idempotent
    int rc = launch_status("k_dec_up_bwd_data");
    if (rc) return rc;
    if (mask_gx) {
      const int64_t quads = N * UP_CI * side * side / 4;
      k_relu_mask_inplace<<<dim3(epi_grid(quads)), dim3(256), 0, st>>>(g_x, x, quads);
      rc = launch_status("k_relu_mask_inplace");
      if (rc) return rc;
    }
  }
  if (wino) {
    if (side == 8 && pre) k_dec_up_wrw_wino<8, true><<<grid, dim3(512), 0, st>>>(x, out, g_out, w_partials, b_partials, N);
    else if (side == 8) k_dec_up_wrw_wino<8><<<grid, dim3(512), 0, st>>>(x, out, g_out, w_partials, b_partials, N);
    else if (pre) k_dec_up_wrw_wino<4, true><<<grid, dim3(512), 0, st>>>(x, out, g_out, w_partials, b_partials, N);
    else k_dec_up_wrw_wino<4><<<grid, dim3(512), 0, st>>>(x, out, g_out, w_partials, b_partials, N);
    return launch_status("k_dec_up_wrw_wino");
  }
  if (side == 8) k_dec_up_wrw<8><<<grid, dim3(256), 0, st>>>(x, out, g_out, w_partials, b_partials, N);
  else k_dec_up_wrw<4><<<grid, dim3(256), 0, st>>>(x, out, g_out, w_partials, b_partials, N);
  return launch_status("k_dec_up_wrw");
}
extern "C" {
int kvae_dec_up_bwd(const float *x, const float *W, const float *out, const float *g_out, float *g_x, float *w_partials,
                    float *b_partials, int64_t N, int32_t Cin, int32_t side, void *stream) {
  if (!x || !W || !out || !g_out || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (N < 1 || (N + 256 * 8) * UP_CO * side * side * 4 >= EM_MAX_BYTES) return KVAE_ERR_ARG;
  if (Cin != UP_CI || (side != 8 && side != 4)) return KVAE_ERR_DIMS;
  return dec_up_bwd_launch(x, W, out, g_out, g_x, w_partials, b_partials, N, side, 0, (hipStream_t)stream);
}
int kvae_dec_up_bwd_flags(const float *x, const float *W, const float *out, const float *g_out, float *g_x, float *w_partials,
                          float *b_partials, int64_t N, int32_t Cin, int32_t side, int32_t flags, void *stream) {
  if (!x || !W || !out || !g_out || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (N < 1 || (N + 256 * 8) * UP_CO * side * side * 4 >= EM_MAX_BYTES) return KVAE_ERR_ARG;
  if (flags & ~(KVAE_UP_G_PREMASKED | KVAE_UP_MASK_GX)) return KVAE_ERR_ARG;
  if (Cin != UP_CI || (side != 8 && side != 4)) return KVAE_ERR_DIMS;
  return dec_up_bwd_launch(x, W, out, g_out, g_x, w_partials, b_partials, N, side, flags, (hipStream_t)stream);
}
}  // extern "C"

#include "vae_heads.h"
extern "C" {
int64_t kvae_head_partial_rows(void) { return HD_WAVES; }

int kvae_enc_head_fwd(const float *feat, const float *Wmu, const float *bmu, const float *Wvar, const float *bvar,
                      const float *eps, float *mu, float *var, float *a, int64_t N, int32_t F, int32_t A,
                      float noise_emission, void *stream) {
  if (!feat || !Wmu || !bmu || !Wvar || !bvar || !mu || !var || !a) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (F != HD_F || A != HD_A) return KVAE_ERR_DIMS;
  const unsigned grid = (unsigned)(N < 4 * 512 ? (N + 3) / 4 : 512);
  k_enc_head_fwd<<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>(feat, Wmu, bmu, Wvar, bvar, eps, noise_emission, mu, var, a, N);
  return launch_status("k_enc_head_fwd");
}
int kvae_enc_head_bwd(const float *feat, const float *Wmu, const float *Wvar, const float *var, const float *eps,
                      const float *g_a, const float *g_mu, const float *g_var, float *g_feat, float *w_partials,
                      float *b_partials, int64_t N, int32_t F, int32_t A, float noise_emission, void *stream) {
  if (!feat || !Wmu || !Wvar || !var || !g_feat || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (F != HD_F || A != HD_A) return KVAE_ERR_DIMS;
  k_enc_head_bwd<<<dim3(HD_WAVES / 4), dim3(256), 0, (hipStream_t)stream>>>(feat, Wmu, Wvar, var, eps, g_a, g_mu, g_var,
                                                                             noise_emission, g_feat, w_partials, b_partials, N);
  return launch_status("k_enc_head_bwd");
}
int kvae_dec_fc_fwd(const float *a, const float *W, const float *b, float *h, int64_t N, int32_t F, int32_t A, void *stream) {
  if (!a || !W || !b || !h) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (F != HD_F || A != HD_A) return KVAE_ERR_DIMS;
  k_dec_fc_fwd<<<dim3(epi_grid(N * (HD_F / 4))), dim3(256), 0, (hipStream_t)stream>>>(a, W, b, h, N * (HD_F / 4));
  return launch_status("k_dec_fc_fwd");
}
int kvae_dec_fc_bwd(const float *g_h, const float *a, const float *W, float *g_a, float *w_partials, float *b_partials,
                    int64_t N, int32_t F, int32_t A, void *stream) {
  if (!g_h || !a || !W || !g_a || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (F != HD_F || A != HD_A) return KVAE_ERR_DIMS;
  k_dec_fc_bwd<<<dim3(HD_WAVES / 4), dim3(256), 0, (hipStream_t)stream>>>(g_h, a, W, g_a, w_partials, b_partials, N);
  return launch_status("k_dec_fc_bwd");
}
int kvae_latent_reg_fwd(const float *a, const float *mu, const float *var, float *reg, int64_t N, int32_t A, void *stream) {
  if (!a || !mu || !var || !reg) return KVAE_ERR_NULL;
  if (N < 1 || A < 1) return KVAE_ERR_ARG;
  k_latent_reg_fwd<<<dim3(epi_grid(N)), dim3(256), 0, (hipStream_t)stream>>>(a, mu, var, reg, N, A);
  return launch_status("k_latent_reg_fwd");
}
int kvae_latent_reg_bwd(const float *a, const float *mu, const float *var, const float *g, float *g_a, float *g_mu,
                        float *g_var, int64_t N, int32_t A, void *stream) {
  if (!a || !mu || !var || !g || !g_a || !g_mu || !g_var) return KVAE_ERR_NULL;
  if (N < 1 || A < 1) return KVAE_ERR_ARG;
  k_latent_reg_bwd<<<dim3(epi_grid(N * A)), dim3(256), 0, (hipStream_t)stream>>>(a, mu, var, g, g_a, g_mu, g_var, N, A);
  return launch_status("k_latent_reg_bwd");
}
int kvae_loss_head_fwd(const float *lpx, const float *regf, const float *mask, const float *elbo_kf, const float *beta,
                       float scale_reconstruction, float vae_weight, float kf_weight, const float *weights_dev, float *out6,
                       float *coef3, int64_t n, void *stream) {
  if (!lpx || !regf || !elbo_kf || !beta || !out6 || !coef3) return KVAE_ERR_NULL;
  if (n < 1) return KVAE_ERR_ARG;
  k_loss_head_fwd<<<dim3(1), dim3(LOSS_HEAD_FWD_THREADS), 0, (hipStream_t)stream>>>(lpx, regf, mask, elbo_kf, beta, scale_reconstruction, vae_weight,
                                                                  kf_weight, weights_dev, out6, coef3, n);
  return launch_status("k_loss_head_fwd");
}
int kvae_loss_head_bwd(const float *g_loss, const float *coef3, const float *mask, float *g_lpx, float *g_regf,
                       float *g_elbo_kf, int64_t n, void *stream) {
  if (!g_loss || !coef3 || !g_lpx || !g_regf || !g_elbo_kf) return KVAE_ERR_NULL;
  if (n < 1) return KVAE_ERR_ARG;
  k_loss_head_bwd<<<dim3(loss_head_bwd_grid(n)), dim3(256), 0, (hipStream_t)stream>>>(g_loss, coef3, mask, g_lpx, g_regf,
                                                                            g_elbo_kf, n);
  return launch_status("k_loss_head_bwd");
}
}  // extern "C"
