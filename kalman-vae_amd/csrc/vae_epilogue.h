// vae_epilogue.h — fused conv epilogues of the frame VAE (SURVEY §8f row 3 territory): the convolutions stay on
// MIOpen, but everything PyTorch appends to them as separate full-tensor passes —
//     + bias  ->  PixelShuffle(r)  ->  ReLU            (decoder, reference vae.py:92-101; r = 1 for the encoder, :20-31)
// — is ONE pass here (read the conv output once, write the activation once), and its backward
//     g_conv = pixel_unshuffle(g_out * [out > 0])
// is one pass as well.  At configs[1] the decoder's second layer alone moves 419 MB per tensor, so every avoided
// pass is ~0.1 ms.  Pure HBM streaming: coalesced along W, no LDS, grid-stride over elements.
//
//   in  : [N, C*r*r, H, W]   (conv output, no bias)      bias : [C*r*r]
//   out : [N, C, H*r, W*r]
// The per-element bodies (epi_fwd_elem / epi_bwd_elem) also serve the plain-loop host simulation; the kernels and their launch
// geometry (path gates, grids, LDS bytes) follow, for kvae_vae.hip and for the test-only emulated workgroups
// (tests/hostsim/wave_emu_step.cpp), which call the same geometry functions with caps a test may lower.
#pragma once
#include <stdint.h>

#include "lds_decl.h"
#include "lgssm_vm.h"

namespace kvae {

struct EpiShape { int64_t N; int C, H, W, r; };

// flat index in `in` that feeds flat index `o` of `out`, and its channel
KV_DEV int64_t epi_src(const EpiShape &s, int64_t o, int *ch) {
  const int OW = s.W * s.r, OH = s.H * s.r;
  const int ow = (int)(o % OW);
  const int64_t t1 = o / OW;
  const int oh = (int)(t1 % OH);
  const int64_t t2 = t1 / OH;
  const int c = (int)(t2 % s.C);
  const int64_t n = t2 / s.C;
  const int cc = c * s.r * s.r + (oh % s.r) * s.r + (ow % s.r);
  *ch = cc;
  return ((n * (s.C * s.r * s.r) + cc) * s.H + oh / s.r) * s.W + ow / s.r;
}

KV_DEV void epi_fwd_elem(const EpiShape &s, const float *in, const float *bias, float *out, int64_t o, int relu) {
  int ch;
  const int64_t i = epi_src(s, o, &ch);
  float v = in[i] + bias[ch];
  if (relu) v = v > 0.f ? v : 0.f;
  out[o] = v;
}

KV_DEV void epi_bwd_elem(const EpiShape &s, const float *g_out, const float *out, float *g_in, int64_t o, int relu) {
  int ch;
  const int64_t i = epi_src(s, o, &ch);
  float g = g_out[o];
  if (relu && !(out[o] > 0.f)) g = 0.f;
  g_in[i] = g;
}

// ---- launch geometry (host side) ------------------------------------------------------------------------------------------------
constexpr int64_t EPI_MAX_BLOCKS = 256 * 32;     // <= 32 blocks per CU, grid-stride the rest
constexpr int EPI_SAMPLES_PER_CHUNK = 32;        // samples a workgroup of k_vae_epilogue_bwd_bias walks = one row of bias_partials
inline unsigned epi_grid(int64_t total, int64_t cap = EPI_MAX_BLOCKS) {
  const int64_t blocks = (total + 255) / 256;
  return (unsigned)(blocks < cap ? blocks : cap);
}
// forward path: 1 / 2 = k_vae_epilogue_fwd_v4<1 | 2> (16-byte accesses: both pointers aligned, whole quads along W), 0 = scalar
inline int epi_fwd_path(const float *in, const float *out, int W, int r) {
  const bool aligned = ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0);
  if (aligned && r == 1 && W % 4 == 0) return 1;
  if (aligned && r == 2 && W % 2 == 0) return 2;
  return 0;
}
inline int64_t epi_bias_partial_rows(int64_t N, int per_chunk = EPI_SAMPLES_PER_CHUNK) { return (N + per_chunk - 1) / per_chunk; }
inline unsigned epi_bias_blocks_x(int64_t vol) { return (unsigned)((vol + 255) / 256); }   // 256 positions of one sample's volume
inline size_t epi_bias_lds_bytes(int Cin) { return sizeof(float) * (size_t)Cin; }          // one bin per input channel

}  // namespace kvae

#if !defined(KVAE_HOSTSIM) || defined(KVAE_WAVE_EMU)
// (the kernels keep the names they had in kvae_vae.hip: outside the namespace)
// Forward, R = 1 or 2: each thread produces 4 consecutive outputs along W (one 16-byte store) from one 16-byte
// (R = 1) or two 8-byte (R = 2: the two sub-pixel channels dx = 0,1 of this output row) loads; 32-bit index math.
template <int R>
__global__ __launch_bounds__(256) void k_vae_epilogue_fwd_v4(const float *__restrict__ in, const float *__restrict__ bias,
                                                             float *__restrict__ out, int C, int H, int W, int64_t quads,
                                                             int relu) {
  const int OW = W * R, OH = H * R, QW = OW / 4;
  for (int64_t qd = (int64_t)blockIdx.x * 256 + threadIdx.x; qd < quads; qd += (int64_t)gridDim.x * 256) {
    const int qw = (int)(qd % QW);
    const int64_t t1 = qd / QW;
    const int oh = (int)(t1 % OH);
    const int64_t t2 = t1 / OH;
    const int c = (int)(t2 % C);
    const int64_t n = t2 / C;
    float4 v;
    if (R == 1) {
      const float b = bias[c];
      const float4 x = *reinterpret_cast<const float4 *>(in + ((n * C + c) * H + oh) * W + 4 * qw);
      v = make_float4(x.x + b, x.y + b, x.z + b, x.w + b);
    } else {
      const int ch0 = c * 4 + (oh & 1) * 2;
      const int64_t base = ((n * (C * 4) + ch0) * H + (oh >> 1)) * W + 2 * qw;
      const float2 a = *reinterpret_cast<const float2 *>(in + base);                    // dx = 0, w = 2qw, 2qw+1
      const float2 d = *reinterpret_cast<const float2 *>(in + base + (int64_t)H * W);  // dx = 1
      const float b0 = bias[ch0], b1 = bias[ch0 + 1];
      v = make_float4(a.x + b0, d.x + b1, a.y + b0, d.y + b1);
    }
    if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    *reinterpret_cast<float4 *>(out + qd * 4) = v;
  }
}

__global__ __launch_bounds__(256) void k_vae_epilogue_fwd(const float *in, const float *bias, float *out, kvae::EpiShape s,
                                                          int64_t total, int relu) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256)
    kvae::epi_fwd_elem(s, in, bias, out, o, relu);
}

// Backward with the bias gradient folded in: a block owns 256 consecutive output positions of the per-sample volume
// [C, H*r, W*r] and walks a chunk of samples; per-thread sums go to per-channel LDS bins (ds_add_f32), one partial row
// per (chunk, channel) leaves the block -> bias_partials[chunk, C*r*r] (summed by the caller; fixed order per bin is not
// guaranteed inside a block: float LDS atomics, differences are at rounding level).
__global__ __launch_bounds__(256) void k_vae_epilogue_bwd_bias(const float *__restrict__ g_out, const float *__restrict__ out,
                                                               float *__restrict__ g_in, float *__restrict__ bias_partials,
                                                               kvae::EpiShape s, int n_per_chunk, int relu) {
  KV_LDS_DYN(float, bins);   // C*r*r floats
  const int Cin = s.C * s.r * s.r;
  const int OW = s.W * s.r, OH = s.H * s.r;
  const int64_t vol = (int64_t)s.C * OH * OW;
  for (int i = threadIdx.x; i < Cin; i += 256) bins[i] = 0.f;
  __syncthreads();
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;   // position inside one sample's output volume
  if (pos < vol) {
    const int ow = (int)(pos % OW);
    const int oh = (int)((pos / OW) % OH);
    const int c = (int)(pos / ((int64_t)OW * OH));
    const int ch = c * s.r * s.r + (oh % s.r) * s.r + (ow % s.r);
    const int64_t in_off = ((int64_t)ch * s.H + oh / s.r) * s.W + ow / s.r;
    const int64_t in_vol = (int64_t)Cin * s.H * s.W;
    const int64_t n0 = (int64_t)blockIdx.y * n_per_chunk;
    const int64_t n1 = n0 + n_per_chunk < s.N ? n0 + n_per_chunk : s.N;
    float acc = 0.f;
    for (int64_t n = n0; n < n1; ++n) {
      float g = g_out[n * vol + pos];
      if (relu && !(out[n * vol + pos] > 0.f)) g = 0.f;
      g_in[n * in_vol + in_off] = g;
      acc += g;
    }
    atomicAdd(&bins[ch], acc);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Cin; i += 256) {
    // only the channels this block touched are non-zero; every block writes its own disjoint partial row slice
    if (bins[i] != 0.f) atomicAdd(&bias_partials[(int64_t)blockIdx.y * Cin + i], bins[i]);
  }
}

__global__ __launch_bounds__(256) void k_vae_epilogue_bwd(const float *g_out, const float *out, float *g_in, kvae::EpiShape s,
                                                          int64_t total, int relu) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256)
    kvae::epi_bwd_elem(s, g_out, out, g_in, o, relu);
}
#endif
