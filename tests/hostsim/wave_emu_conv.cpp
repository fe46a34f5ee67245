// wave_emu_conv.cpp — TEST-ONLY: the encoder's convolution kernels, the very __global__ functions of the product, on emulated
// workgroups (wave_emu.h) over host pointers:
//   csrc/vae_conv_mid.h   k_enc_mid_fwd<16 | 8> / k_enc_mid_bwd_data<16 | 8> / k_enc_mid_wrw<16 | 8>  (32x32x2 f32 MFMA, raw buffer
//                         loads and stores, zero padding through LDS reads out of range, persistent grid, chunk rotation)
//   csrc/vae_conv_edge.h  k_enc_stem_fwd / k_enc_stem_wrw / k_enc_stem_wrw_mfma<true | false>          (16x16x4 f32 MFMA)
// The grids, the 32-bit-offset gate and the choice of the stem's weight-gradient kernel come from the host functions of those
// headers - the ones kvae_vae.hip calls - with the caps and the KVAE_STEM_MFMA mode as arguments a test may set
// (kvae_wemu_enc_mid_max_wgs, kvae_wemu_stem_max_rows, kvae_wemu_stem_mode), so that the persistent rounds run at a few frames.
// hostsim.cpp routes kvae_enc_mid_fwd / bwd and kvae_enc_stem_fwd / bwd here, after their argument checks, when
// kvae_hostsim_wave_emu(1) was called; every launch is counted per kernel instance (kvae_wemu_rnn_launches, indices below), and
// the buffer accesses that fell outside their resource - loads answered with zeros, stores dropped - are kept per instance for
// its last launch (kvae_wemu_conv_oob).
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../include/kvae_lgssm.h"
#include "../../kalman-vae_amd/csrc/vae_conv_edge.h"
#include "../../kalman-vae_amd/csrc/vae_conv_mid.h"

using namespace kvae;

static_assert(EM_OOB == wemu::kLdsOob, "the out-of-range base of the kernels is the emulator's");

extern "C" void kvae_wemu_rnn_note(int which);   // wave_emu_rnn.cpp: the launch counters

// indices of kvae_wemu_rnn_launches (0 .. 9: wave_emu_rnn.cpp, 10 .. 32: wave_emu_reduce.cpp, 33 .. 45: wave_emu_step.cpp)
enum {
  kMidFwd = 46,    // + 0 / 1: k_enc_mid_fwd<16 | 8>
  kMidData = 48,   // + 0 / 1: k_enc_mid_bwd_data<16 | 8>
  kMidWrw = 50,    // + 0 / 1: k_enc_mid_wrw<16 | 8>
  kStemFwd = 52, kStemWrw = 53,
  kStemWrwMfma = 54,   // + 0 / 1: k_enc_stem_wrw_mfma<true | false>
  kConvFirst = kMidFwd, kConvKinds = 10,
};

// the arguments the product passes as its constants (or reads once from the environment), settable here
static int g_em_max_wgs = EM_MAX_WGS, g_ce_max_rows = CE_MAX_ROWS, g_stem_mode = 1;
static long g_oob[kConvKinds][2];   // [instance][0 loads answered with zeros | 1 stores dropped] of the instance's last launch

static int swap_setting(int &slot, int v, int dflt) {   // v < 0: back to the product's constant; returns the previous value
  const int was = slot;
  slot = v < 0 ? dflt : v;
  return was;
}

// one launch: counted, named for the emulator's abort messages, its out-of-range buffer accesses kept
template <class Body>
static void conv_launch(int which, const char *name, unsigned grid, Body body) {
  kvae_wemu_rnn_note(which);
  wemu::oob_loads.store(0), wemu::oob_stores.store(0);
  wemu::launch_wg({grid, 1, 1}, 256, 0, [&] {
    wemu::t_kernel = name;
    body();
  });
  g_oob[which - kConvFirst][0] = wemu::oob_loads.load(), g_oob[which - kConvFirst][1] = wemu::oob_stores.load();
}

extern "C" {

int kvae_wemu_enc_mid_max_wgs(int v) { return swap_setting(g_em_max_wgs, v, EM_MAX_WGS); }
int kvae_wemu_stem_max_rows(int v) { return swap_setting(g_ce_max_rows, v, CE_MAX_ROWS); }
int kvae_wemu_stem_mode(int v) { return swap_setting(g_stem_mode, v, 1); }   // KVAE_STEM_MFMA = 0 | 1 | 2
long kvae_wemu_conv_oob(int which, int stores) {
  return which >= kConvFirst && which < kConvFirst + kConvKinds ? g_oob[which - kConvFirst][stores ? 1 : 0] : -1;
}

// kvae_enc_mid_partial_rows / kvae_conv_edge_partial_rows and the gate of kvae_enc_mid_fwd / bwd (kvae_vae.hip)
int64_t kvae_wemu_enc_mid_rows(int64_t N, int32_t side) { return em_grid(N, side, g_em_max_wgs); }
int64_t kvae_wemu_conv_edge_rows(int64_t N) { return conv_edge_partial_rows(N, g_ce_max_rows); }
int kvae_wemu_enc_mid_gate(int64_t N, int32_t side) { return em_launch_ok(N, side) ? KVAE_OK : KVAE_ERR_ARG; }   // the product's cap

void kvae_wemu_enc_mid_fwd(const float *in, const float *W, const float *bias, float *out, int64_t N, int32_t side) {
  const unsigned grid = (unsigned)em_grid(N, side, g_em_max_wgs);
  if (side == 16) conv_launch(kMidFwd, "k_enc_mid_fwd<16>", grid, [&] { k_enc_mid_fwd<16>(in, W, bias, out, N); });
  else conv_launch(kMidFwd + 1, "k_enc_mid_fwd<8>", grid, [&] { k_enc_mid_fwd<8>(in, W, bias, out, N); });
}
void kvae_wemu_enc_mid_bwd(const float *in, const float *W, const float *out, const float *g_out, float *g_in, float *w_partials,
                           float *b_partials, int64_t N, int32_t side) {
  const unsigned grid = (unsigned)em_grid(N, side, g_em_max_wgs);
  if (g_in) {
    if (side == 16) conv_launch(kMidData, "k_enc_mid_bwd_data<16>", grid, [&] { k_enc_mid_bwd_data<16>(W, out, g_out, g_in, N); });
    else conv_launch(kMidData + 1, "k_enc_mid_bwd_data<8>", grid, [&] { k_enc_mid_bwd_data<8>(W, out, g_out, g_in, N); });
  }
  if (side == 16) conv_launch(kMidWrw, "k_enc_mid_wrw<16>", grid, [&] { k_enc_mid_wrw<16>(in, out, g_out, w_partials, b_partials, N); });
  else conv_launch(kMidWrw + 1, "k_enc_mid_wrw<8>", grid, [&] { k_enc_mid_wrw<8>(in, out, g_out, w_partials, b_partials, N); });
}

void kvae_wemu_enc_stem_fwd(const float *x, const float *W, const float *bias, float *out, uint32_t *relu_bits, int64_t N) {
  conv_launch(kStemFwd, "k_enc_stem_fwd", es_fwd_grid(N), [&] { k_enc_stem_fwd(x, W, bias, out, relu_bits); });
}
// KVAE_OK, or KVAE_ERR_NULL where the mode needs `out` and the caller has none
int kvae_wemu_enc_stem_bwd(const float *x, const float *out, const uint32_t *relu_bits, const float *g_out, float *w_partials,
                           float *b_partials, int64_t N) {
  const unsigned grid = (unsigned)conv_edge_partial_rows(N, g_ce_max_rows);
  const int kernel = es_wrw_kernel(g_stem_mode, relu_bits != nullptr, out != nullptr);
  if (kernel == ES_WRW_REFUSED) return KVAE_ERR_NULL;
  if (kernel == ES_WRW_MFMA_BITS)
    conv_launch(kStemWrwMfma, "k_enc_stem_wrw_mfma<true>", grid,
                [&] { k_enc_stem_wrw_mfma<true>(x, out, relu_bits, g_out, w_partials, b_partials, N); });
  else if (kernel == ES_WRW_MFMA_OUT)
    conv_launch(kStemWrwMfma + 1, "k_enc_stem_wrw_mfma<false>", grid,
                [&] { k_enc_stem_wrw_mfma<false>(x, out, relu_bits, g_out, w_partials, b_partials, N); });
  else
    conv_launch(kStemWrw, "k_enc_stem_wrw", grid, [&] { k_enc_stem_wrw(x, out, g_out, w_partials, b_partials, N); });
  return KVAE_OK;
}

// the emulator's own cases for what this unit added to it (kvae_wemu_selftest of wave_emu_rnn.cpp calls it): the number of wrong
// results.  The aborting outcomes (a straddling buffer access, an LDS read between the object and the out-of-range base) are
// classified without being run: buffer_range / lds_read end the process.
static void k_conv_selftest(const float *A, const float *B, float *D, char *buf, int *bad) {
  KV_LDS(float, arr, [96]);
  const int l = threadIdx.x, j = l & 31, h = l >> 5;
  // D = A[32 x 2] B[2 x 32] + 1 on the 32x32x2 map
  em_f16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 1.f;
  acc = KV_MFMA_F32(A[j * 2 + h], B[h * 32 + j], acc);
  for (int r = 0; r < 16; ++r) D[KV_ACC_ROW(r, h) * 32 + j] = acc[r];
  // a resource of 64 x 16 - 16 bytes over a block of 64 x 16: lane 63's access is wholly outside
  const __amdgpu_buffer_rsrc_t rs = em_rsrc(buf, 63 * 16);
  const float4 v = em_ld4(rs, (uint32_t)l * 16u);
  if (l < 63 ? (v.x != (float)l || v.w != (float)l + 0.75f) : (v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f))
    __atomic_fetch_add(bad, 1, __ATOMIC_RELAXED);
  em_st4(rs, (uint32_t)l * 16u, make_float4(-1.f, -2.f, -3.f, (float)l));
  em_st1(rs, (uint32_t)l * 16u + (l < 63 ? 4u : 0u), 7.f);
  // LDS: inside the object (from a pointer into its middle, a negative index included), unwritten -> NaN, out of range -> 0
  float *mid = arr + 32;
  arr[l] = (float)(l + 1);
  __syncthreads();
  const float in0 = KV_LDS_RD(mid, l - 32), nan = KV_LDS_RD(mid, 32 + (l & 31)), z0 = KV_LDS_RD(mid, EM_OOB),
              z1 = KV_LDS_RD(mid, EM_OOB + 5 * l);
  if (in0 != (float)(l + 1) || nan == nan || z0 != 0.f || z1 != 0.f) __atomic_fetch_add(bad, 1, __ATOMIC_RELAXED);
}
int kvae_wemu_conv_selftest(void) {
  std::vector<float> A(64), B(64), D(1024, NAN);
  for (int i = 0; i < 64; ++i) A[i] = 0.25f * (float)(i % 7) - 0.5f, B[i] = 1.f + 0.125f * (float)(i % 5);
  float *buf = static_cast<float *>(malloc(64 * 16));   // ends with its last element
  for (int i = 0; i < 256; ++i) buf[i] = (float)(i / 4) + 0.25f * (float)(i % 4);
  int bad = 0;
  wemu::oob_loads.store(0), wemu::oob_stores.store(0);
  wemu::launch_wg({1, 1, 1}, 64, 0, [&] {
    wemu::t_kernel = "k_conv_selftest";
    k_conv_selftest(A.data(), B.data(), D.data(), reinterpret_cast<char *>(buf), &bad);
  });
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      float want = 1.f;
      for (int k = 0; k < 2; ++k) want = fmaf(A[i * 2 + k], B[k * 32 + j], want);
      bad += D[i * 32 + j] != want;
    }
  for (int l = 0; l < 64; ++l) {   // lanes 0 .. 62 stored, lane 63's two stores were dropped
    const float *q = buf + 4 * l;
    bad += l < 63 ? !(q[0] == -1.f && q[1] == 7.f && q[2] == -3.f && q[3] == (float)l)
                  : !(q[0] == 63.f && q[1] == 63.25f && q[2] == 63.5f && q[3] == 63.75f);
  }
  bad += wemu::oob_loads.load() != 1 || wemu::oob_stores.load() != 2;
  // the classification behind the aborts, without running one
  const wemu::Rsrc rs = wemu::make_rsrc(buf, 0, 63 * 16, 0);
  bad += wemu::buffer_class(rs, 62 * 16, 16) != 1 || wemu::buffer_class(rs, 63 * 16, 16) != 0 || wemu::buffer_class(rs, 63 * 16 - 4, 16) != -1;
  bad += wemu::lds_class(32, 64, 0) != 1 || wemu::lds_class(32, 64, -32) != 1 || wemu::lds_class(32, 64, 63) != 1 ||
         wemu::lds_class(32, 64, 64) != -1 || wemu::lds_class(32, 64, -33) != -1 || wemu::lds_class(32, 64, EM_OOB - 1) != -1 ||
         wemu::lds_class(32, 64, EM_OOB) != 0;
  free(buf);
  return bad;
}
}
