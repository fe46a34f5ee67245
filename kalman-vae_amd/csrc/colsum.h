// colsum.h — out[c] = sum_r partials[r, c]: second stage of every deterministic two-stage reduction (bias / weight gradient
// partial rows).  HBM-bound (the 32->128 layers hand over 256 x 36864 floats = 38 MB): a lane owns four columns (dwordx4, 1 KiB
// per wave and row), the eight waves of a block take every eighth row, four rows in flight per wave, fold through LDS.
// The path gate and the grids (colsum_v4_ok, colsum_v4_blocks, colsum_blocks) sit beside the kernels: kvae_vae.hip and the
// test-only emulated workgroups (tests/hostsim/wave_emu_step.cpp) call the same functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds_decl.h"

namespace kvae {

// ---- launch geometry (host side) ------------------------------------------------------------------------------------------------
constexpr int COLSUM_V4_THREADS = 512, COLSUM_THREADS = 256;
// the dwordx4 kernel: whole quads of columns, input and output on 16-byte boundaries (then every row is, cols % 4 == 0)
inline bool colsum_v4_ok(const float *partials, const float *out, int64_t cols) {
  return (cols & 3) == 0 && ((((uintptr_t)partials | (uintptr_t)out) & 15) == 0);
}
inline unsigned colsum_v4_blocks(int64_t cols) { return (unsigned)((cols + 255) / 256); }   // 64 lanes x 4 columns per block
inline unsigned colsum_blocks(int64_t cols) { return (unsigned)((cols + 63) / 64); }        // 64 columns x 4 row lanes per block

}  // namespace kvae

// (the kernels keep the names they had in kvae_vae.hip: outside the namespace)
__device__ __forceinline__ void colsum_v4_body(const float *__restrict__ partials, float *__restrict__ out, int64_t rows, int64_t cols,
                                               unsigned block) {
  KV_LDS(float4, red, [8][64]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = ((int64_t)block * 64 + lane) * 4;
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
  if (c < cols) {
    const float *p = partials + c;
    int64_t r = wv;
    for (; r + 24 < rows; r += 32) {
      const float4 a = *reinterpret_cast<const float4 *>(p + r * cols), b = *reinterpret_cast<const float4 *>(p + (r + 8) * cols),
                   d = *reinterpret_cast<const float4 *>(p + (r + 16) * cols), e = *reinterpret_cast<const float4 *>(p + (r + 24) * cols);
      s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
      s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
      s2.x += d.x; s2.y += d.y; s2.z += d.z; s2.w += d.w;
      s3.x += e.x; s3.y += e.y; s3.z += e.z; s3.w += e.w;
    }
    for (; r < rows; r += 8) {
      const float4 a = *reinterpret_cast<const float4 *>(p + r * cols);
      s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
    }
  }
  red[wv][lane] = make_float4((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y), (s0.z + s1.z) + (s2.z + s3.z),
                              (s0.w + s1.w) + (s2.w + s3.w));
  __syncthreads();
  if (wv == 0 && c < cols) {
    float4 t = red[0][lane];
#pragma unroll
    for (int w = 1; w < 8; ++w) { const float4 u = red[w][lane]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
    *reinterpret_cast<float4 *>(out + c) = t;
  }
}
__global__ __launch_bounds__(512) void k_colsum_v4(const float *__restrict__ partials, float *__restrict__ out, int64_t rows,
                                                   int64_t cols) {
  colsum_v4_body(partials, out, rows, cols, blockIdx.x);
}
// two jobs in one launch: the first nb_a workgroups take job a, the rest job b
__global__ __launch_bounds__(512) void k_colsum_v4_pair(const float *__restrict__ pa, float *__restrict__ oa, int64_t rows_a, int64_t cols_a,
                                                        unsigned nb_a, const float *__restrict__ pb, float *__restrict__ ob,
                                                        int64_t rows_b, int64_t cols_b) {
  if (blockIdx.x < nb_a) colsum_v4_body(pa, oa, rows_a, cols_a, blockIdx.x);
  else colsum_v4_body(pb, ob, rows_b, cols_b, blockIdx.x - nb_a);
}
// any column count (scalar): 64 columns x 4 row lanes per block
__global__ __launch_bounds__(256) void k_colsum(const float *__restrict__ partials, float *__restrict__ out, int64_t rows,
                                                int64_t cols) {
  KV_LDS(float, red, [256]);
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cx;
  float s0 = 0.f, s1 = 0.f;
  if (c < cols) {
    int64_t r = ry;
    for (; r + 4 < rows; r += 8) {
      s0 += partials[r * cols + c];
      s1 += partials[(r + 4) * cols + c];
    }
    if (r < rows) s0 += partials[r * cols + c];
  }
  red[threadIdx.x] = s0 + s1;
  __syncthreads();
  if (ry == 0 && c < cols) out[c] = (red[cx] + red[64 + cx]) + (red[128 + cx] + red[192 + cx]);
}
