// gen_asan_driver.cpp — TEST-ONLY: the rollout kernel body of kvae_lgssm_generate (csrc/lgssm_gen.h) on emulated wavefronts
// (wave_emu.h), as a standalone program that tests/test_generate.py builds with -fsanitize=address,undefined and runs as a child
// process, through the host simulation's entry point defined there.  Every buffer is allocated at its exact size, so a read or
// write past the layouts of include/kvae_lgssm.h is a sanitizer report.  One small lstm case (K = 3, ragged: 7 rollouts, 4 per wavefront) and one small switching case.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include <memory>
#include <random>
#include <vector>

#include "../../kalman-vae_amd/csrc/lgssm_gen.h"

using V = std::vector<float>;

static V rnd(size_t n, std::mt19937 &g, float sc) {
  std::normal_distribution<float> d(0.f, sc);
  V v(n);
  for (auto &x : v) x = d(g);
  return v;
}
static V lower(int count, int n, float diag) {   // `count` lower-triangular [n,n] factors
  V v((size_t)count * n * n, 0.f);
  for (int c = 0; c < count; ++c)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) v[((size_t)c * n + i) * n + j] = i == j ? diag : 0.01f;
  return v;
}

template <bool SWITCH>
static int run(int B, int S, int H, int n, int m, int p, int K) {
  std::mt19937 g(B * 100 + K);
  const int R = B * S, HID = kvae_gen::HID;
  V A = rnd((size_t)K * n * n, g, 0.2f), Bm = rnd((size_t)K * n * m, g, 0.3f), C = rnd((size_t)K * p * n, g, 0.5f);
  V LQ = lower(SWITCH ? K : 1, n, 0.1f), LR = lower(1, p, 0.05f), mu = rnd((size_t)B * n, g, 1.f), L0 = lower(B, n, 0.3f);
  V U = rnd((size_t)B * H * m, g, 0.5f);
  V w_ih = rnd(4 * HID * p, g, 0.3f), w_hh = rnd(4 * HID * HID, g, 0.1f), b_ih = rnd(4 * HID, g, 0.1f), b_hh = rnd(4 * HID, g, 0.1f);
  V head_w = rnd((size_t)K * HID, g, 1.f), head_b = rnd(K, g, 0.5f);
  V h0 = rnd((size_t)B * HID, g, 0.5f), c0 = rnd((size_t)B * HID, g, 0.5f), y0 = rnd((size_t)B * p, g, 0.5f);
  V P((size_t)K * K, 0.1f / (K > 1 ? K - 1 : 1)), s0((size_t)B * K, 0.f);
  for (int k = 0; k < K; ++k) P[(size_t)k * K + k] = K > 1 ? 0.9f : 1.f;
  for (int b = 0; b < B; ++b) s0[(size_t)b * K + b % K] = 1.f;
  V eps0 = rnd((size_t)R * n, g, 1.f), eps_z = rnd((size_t)R * H * n, g, 1.f), eps_a = rnd((size_t)R * H * p, g, 1.f);
  V gum = rnd((size_t)R * H * K, g, 1.f);
  V a((size_t)R * H * p, NAN), z((size_t)R * H * n, NAN), w((size_t)R * H * K, NAN);
  kvae_gen_problem pr{};
  pr.B = B, pr.S = S, pr.H = H, pr.n = n, pr.m = m, pr.p = p, pr.K = K, pr.kind = SWITCH ? 1 : 0, pr.hidden = HID;
  pr.A = A.data(), pr.Bm = Bm.data(), pr.C = C.data(), pr.LQ = LQ.data(), pr.LR = LR.data(), pr.mu = mu.data(), pr.L0 = L0.data();
  pr.U = U.data();
  if (SWITCH) {
    pr.P = P.data(), pr.s0 = s0.data(), pr.gumbel = gum.data();
  } else {
    pr.w_ih = w_ih.data(), pr.w_hh = w_hh.data(), pr.b_ih = b_ih.data(), pr.b_hh = b_hh.data();
    pr.head_w = head_w.data(), pr.head_b = head_b.data(), pr.h0 = h0.data(), pr.c0 = c0.data(), pr.y0 = y0.data();
  }
  pr.eps0 = eps0.data(), pr.eps_z = eps_z.data(), pr.eps_a = eps_a.data();
  pr.a_out = a.data(), pr.z_out = z.data(), pr.w_out = w.data();
  if (kvae_lgssm_generate(&pr, nullptr) != KVAE_OK) return 1;   // the emulated entry point of csrc/lgssm_gen.h
  for (const V *v : {&a, &z, &w})
    for (float x : *v)
      if (!std::isfinite(x)) return 2;   // every output element written, nothing past them
  return 0;
}

int main() {
  const int rc1 = run<false>(1, 7, 3, 4, 3, 2, 3);
  const int rc2 = run<true>(3, 2, 4, 5, 2, 3, 4);
  printf("lstm %d switching %d\n", rc1, rc2);
  if (rc1 || rc2) return 1;
  printf("GEN-ASAN-OK\n");
  return 0;
}
