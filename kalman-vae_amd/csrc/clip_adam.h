// clip_adam.h — clip_grad_norm_ + Adam on flat buffers: two launches instead of ~12 (norm, clamp, reciprocal, scale, three foreach
// kernels).  k_grad_sumsq leaves one partial sum of squares per workgroup in ws[0 .. parts) and counts the step of every active
// segment; k_clip_adam folds the same partials in every workgroup, in the same order, and applies the clipped Adam update.
// The launch geometry (ca_parts, ca_blocks) sits beside the kernels: kvae_vae.hip calls it with the product's constants, the
// test-only emulated workgroups (tests/hostsim/wave_emu_step.cpp) with caps a test may lower.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds_decl.h"

namespace kvae {

constexpr int CA_BLOCKS = 512;       // partial sums of squares (ws[0..CA_BLOCKS))
constexpr int CA_MAX_SEG = 1024;     // parameter tensors ("segments") of one flat buffer
constexpr int CA_MAX_BLOCKS = 2048;  // workgroups of k_clip_adam; the elements beyond them are taken grid-stride

// ---- launch geometry (host side) ------------------------------------------------------------------------------------------------
// workgroups of k_grad_sumsq = partials k_clip_adam folds (`nparts`): one per 1024 elements, at most `cap`
inline unsigned ca_parts(int64_t n, int cap = CA_BLOCKS) {
  const int64_t want = (n + 1023) / 1024;
  return (unsigned)(want < cap ? want : cap);
}
inline unsigned ca_blocks(int64_t n, int cap = CA_MAX_BLOCKS) { return (unsigned)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }

}  // namespace kvae

// (the kernels keep the names they had in kvae_vae.hip: outside the namespace)

// Segments: seg_of[i] names the parameter tensor element i belongs to; a segment with seg_active[s] == 0 is a FROZEN parameter
// (requires_grad False: the reference's training phases, train.py:142-207) - torch's clip_grad_norm_ and Adam skip it because its
// .grad is None: it adds nothing to the norm, its moments and its step count stay as they are.  Every segment counts its own steps
// (torch keeps `step` per parameter, so a parameter thawed at epoch 6 starts its bias correction at step 1).
__global__ __launch_bounds__(256) void k_grad_sumsq(const float *__restrict__ g, int64_t n, const int32_t *__restrict__ seg_of,
                                                    int n_seg, const float *__restrict__ seg_active,
                                                    const float *__restrict__ div_dev, float *__restrict__ seg_steps,
                                                    float *__restrict__ ws) {
  KV_LDS(float, red, [256]);
  const float inv = div_dev ? 1.0f / fmaxf(*div_dev, 1.0f) : 1.0f;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = g[i] * inv;
    if (seg_active && seg_active[seg_of ? seg_of[i] : 0] == 0.f) v = 0.f;   // the same predicate as k_clip_adam's freeze
    s = fmaf(v, v, s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = red[0];
  if (blockIdx.x == 0)                                  // the next launch reads the incremented step counts
    for (int sg = threadIdx.x; sg < n_seg; sg += 256)
      if (!seg_active || seg_active[sg] != 0.f) seg_steps[sg] += 1.0f;
}
__global__ __launch_bounds__(256) void k_clip_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ v, int64_t n, const int32_t *__restrict__ seg_of, int n_seg,
                                                   const float *__restrict__ seg_active, const float *__restrict__ seg_steps,
                                                   const float *__restrict__ lr_dev, float lr, float beta1, float beta2, float eps,
                                                   float wd, float clip, const float *__restrict__ div_dev,
                                                   float *__restrict__ norm_out, const float *__restrict__ ws, int nparts) {
  KV_LDS(float, red, [256]);
  KV_LDS(float, s_step_size, [kvae::CA_MAX_SEG]);           // step_size < 0 marks a frozen segment
  KV_LDS(float, s_bc2s, [kvae::CA_MAX_SEG]);
  float s = 0.f;                                      // every block folds the same partials in the same order
  for (int i = threadIdx.x; i < nparts; i += 256) s += ws[i];
  red[threadIdx.x] = s;
  const float lrv = lr_dev ? *lr_dev : lr;
  for (int sg = threadIdx.x; sg < n_seg; sg += 256) {
    const float step = seg_steps[sg];
    const bool on = !seg_active || seg_active[sg] != 0.f;
    s_step_size[sg] = on ? lrv / (1.0f - powf(beta1, step)) : -1.0f;
    s_bc2s[sg] = on ? sqrtf(1.0f - powf(beta2, step)) : 1.0f;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float total = sqrtf(red[0]);
  if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total;
  const float inv = div_dev ? 1.0f / fmaxf(*div_dev, 1.0f) : 1.0f;
  const float scale = inv * (clip > 0.f ? fminf(clip / (total + 1e-6f), 1.0f) : 1.0f);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int sg = seg_of ? seg_of[i] : 0;
    const float step_size = s_step_size[sg], bc2s = s_bc2s[sg];
    if (step_size < 0.f) continue;
    float gi = g[i] * scale;
    const float pi = p[i];
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    const float mi = m[i] + (gi - m[i]) * (1.0f - beta1);          // lerp
    const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
    m[i] = mi, v[i] = vi;
    p[i] = pi - step_size * mi / (sqrtf(vi) / bc2s + eps);
  }
}
