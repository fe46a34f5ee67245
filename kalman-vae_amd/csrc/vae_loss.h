// vae_loss.h — Bernoulli reconstruction term of the frame VAE, fused:
//   frame_ll[f] = - sum_pixels BCEWithLogits(logit, x)        (reference losses.py:85-87: F.binary_cross_entropy_with_logits
//                                                               (reduction='none').sum(dim=(2,3,4)), negated)
// One wavefront per frame: 16-byte loads, in-register accumulation, one shuffle reduction, one float out.  The reference
// materialises the per-pixel loss tensor (52 MB at configs[1]) and reduces it in a second pass; its autograd adds three
// more element-wise passes.  Backward here: g_logit = -g_frame[f] * (sigmoid(logit) - x), one pass.
#pragma once
#include "lgssm_vm.h"

namespace kvae {

// numerically stable, same formula torch uses: max(l,0) - l*x + log1p(exp(-|l|))
KV_DEV float bce_logit(float l, float x) { return fmaxf(l, 0.f) - l * x + log1pf(expf(-fabsf(l))); }
KV_DEV float sigmoid_stable(float l) {
  const float e = expf(-fabsf(l));
  return l >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

}  // namespace kvae

#ifdef KVAE_HOSTSIM
// Host twins of the decoder head with the Bernoulli term folded in (vae_conv_edge.h: k_dec_head_fwd<true>, k_dec_head_bwd<true, .>)
// for the CPU test tier: plain loops over the host twins of the unfused entry points, which the public header declares.
#include <stdlib.h>
extern "C" {
int kvae_dec_head_loss_fwd(const float *in, const float *W, const float *bias, const float *x, float *logits, float *x_recon,
                           float *frame_ll, float *w_scratch, int64_t N, int32_t Cin, int32_t side, void *) {
  if (!in || !W || !bias || !x || !logits || !frame_ll || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != 32 || side != 16) return KVAE_ERR_DIMS;
  const int rc = kvae_dec_head_fwd(in, W, bias, logits, w_scratch, N, Cin, side, nullptr);
  if (rc) return rc;
  for (int64_t n = 0; n < N; ++n) {
    const float *l = logits + n * 1024, *t = x + n * 1024;
    // the kernel's order: thread (h, w) sums its 2 x 2 pixels, 64 threads fold in a shuffle tree, the four waves in a fixed order
    float wave[4];
    for (int wv = 0; wv < 4; ++wv) {
      float lane[64];
      for (int j = 0; j < 64; ++j) {
        const int tid = wv * 64 + j, p = (2 * (tid >> 4)) * 32 + 2 * (tid & 15);
        lane[j] = (kvae::bce_logit(l[p], t[p]) + kvae::bce_logit(l[p + 1], t[p + 1])) +
                  (kvae::bce_logit(l[p + 32], t[p + 32]) + kvae::bce_logit(l[p + 33], t[p + 33]));
      }
      for (int off = 32; off > 0; off >>= 1)
        for (int j = 0; j < off; ++j) lane[j] += lane[j + off];
      wave[wv] = lane[0];
    }
    frame_ll[n] = -((wave[0] + wave[1]) + (wave[2] + wave[3]));
    if (x_recon)
      for (int p = 0; p < 1024; ++p) x_recon[n * 1024 + p] = kvae::sigmoid_stable(l[p]);
  }
  return KVAE_OK;
}
int kvae_dec_head_loss_bwd(const float *in, const float *W, const float *logits, const float *x, const float *g_frame,
                           float *g_in, float *w_partials, float *b_partials, float *w_scratch, int64_t N, int32_t Cin,
                           int32_t side, void *) {
  if (!in || !W || !logits || !x || !g_frame || !w_partials || !b_partials || !w_scratch) return KVAE_ERR_NULL;
  if (N < 1) return KVAE_ERR_ARG;
  if (Cin != 32 || side != 16) return KVAE_ERR_DIMS;
  float *g = static_cast<float *>(malloc(sizeof(float) * N * 1024));   // the gradient the kernel never stores
  if (!g) return KVAE_ERR_ARG;
  int rc = kvae_bce_frames_bwd(logits, x, g_frame, g, N, 1024, nullptr);
  if (!rc) rc = kvae_dec_head_bwd(in, W, g, g_in, w_partials, b_partials, w_scratch, N, Cin, side, nullptr);
  free(g);
  return rc;
}
// Host twins of the entries that apply a ReLU mask where the gradient is made (k_dec_head_bwd<., true, true>, vae_conv_up_wino.h
// PREMASKED / MASK_GX): the existing twins plus the select.  A pre-masked gradient needs nothing here: the twin of
// kvae_dec_up_bwd masks by `out` again, which changes no bit of it.
static void kv_relu_mask_host(float *g, const float *act, int64_t n) {
  for (int64_t i = 0; i < n; ++i) g[i] = act[i] > 0.f ? g[i] : 0.f;
}
int kvae_dec_head_bwd_masked(const float *in, const float *W, const float *g_logits, float *g_in, float *w_partials,
                             float *b_partials, float *w_scratch, int64_t N, int32_t Cin, int32_t side, void *) {
  const int rc = kvae_dec_head_bwd(in, W, g_logits, g_in, w_partials, b_partials, w_scratch, N, Cin, side, nullptr);
  if (!rc && g_in) kv_relu_mask_host(g_in, in, N * Cin * side * side);
  return rc;
}
int kvae_dec_head_loss_bwd_masked(const float *in, const float *W, const float *logits, const float *x, const float *g_frame,
                                  float *g_in, float *w_partials, float *b_partials, float *w_scratch, int64_t N, int32_t Cin,
                                  int32_t side, void *) {
  const int rc = kvae_dec_head_loss_bwd(in, W, logits, x, g_frame, g_in, w_partials, b_partials, w_scratch, N, Cin, side, nullptr);
  if (!rc && g_in) kv_relu_mask_host(g_in, in, N * Cin * side * side);
  return rc;
}
int kvae_dec_up_bwd_flags(const float *x, const float *W, const float *out, const float *g_out, float *g_x, float *w_partials,
                          float *b_partials, int64_t N, int32_t Cin, int32_t side, int32_t flags, void *) {
  if (!x || !W || !out || !g_out || !w_partials || !b_partials) return KVAE_ERR_NULL;
  if (N < 1 || (flags & ~(KVAE_UP_G_PREMASKED | KVAE_UP_MASK_GX))) return KVAE_ERR_ARG;
  const int rc = kvae_dec_up_bwd(x, W, out, g_out, g_x, w_partials, b_partials, N, Cin, side, nullptr);
  if (!rc && g_x && (flags & KVAE_UP_MASK_GX)) kv_relu_mask_host(g_x, x, N * Cin * side * side);
  return rc;
}
}  // extern "C"
#endif
