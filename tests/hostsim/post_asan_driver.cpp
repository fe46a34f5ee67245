// post_asan_driver.cpp — TEST-ONLY: both kernel bodies of kvae_lgssm_posterior_sample (csrc/lgssm_post.h: the gains of every
// (b, t) item, the backward-sampled paths) on emulated wavefronts (wave_emu.h), as a standalone program that
// tests/test_posterior_sample.py builds with -fsanitize=address,undefined and runs as a child process, through the host
// simulation's entry point defined there.  Every buffer is allocated at its exact size, so a read or write past the layouts of
// include/kvae_lgssm.h is a sanitizer report.  Cases: n = 4, n = 16 and a run-time n, ragged B*T and B*S, T = 1, a misaligned
// draw buffer (the scalar-load paths kernel).
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include <memory>
#include <random>
#include <vector>

#include "../../kalman-vae_amd/csrc/lgssm_post.h"

using V = std::vector<float>;

static V rnd(size_t n, std::mt19937 &g, float sc) {
  std::normal_distribution<float> d(0.f, sc);
  V v(n);
  for (auto &x : v) x = d(g);
  return v;
}
static V spd(int count, int n, std::mt19937 &g, float diag) {   // `count` symmetric, diagonally dominant [n,n]
  V v((size_t)count * n * n, 0.f);
  std::uniform_real_distribution<float> d(-0.02f, 0.02f);
  for (int c = 0; c < count; ++c)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) {
        const float x = i == j ? diag + d(g) : d(g);
        v[((size_t)c * n + i) * n + j] = v[((size_t)c * n + j) * n + i] = x;
      }
  return v;
}

static int run(int B, int S, int T, int n, int p, bool per_step, bool misalign) {
  std::mt19937 g(B * 1000 + T * 10 + n);
  const size_t BT = (size_t)B * T, R = (size_t)B * S;
  V mf = rnd(BT * n, g, 1.f), mp = rnd(BT * n, g, 1.f), Sf = spd((int)BT, n, g, 0.5f), Sp = spd((int)BT, n, g, 0.8f);
  V A = rnd((per_step ? BT : 1) * n * n, g, 0.2f), C = rnd((per_step ? BT : 1) * p * n, g, 0.5f);
  V Q = spd(per_step ? (int)BT : 1, n, g, 0.1f), LR((size_t)p * p, 0.f);
  for (int i = 0; i < p; ++i) LR[(size_t)i * p + i] = 0.1f;
  V epsbuf = rnd(R * T * n + 4, g, 1.f), eta = rnd(R * T * p, g, 1.f);
  const size_t skew = (4 - (reinterpret_cast<uintptr_t>(epsbuf.data()) / 4) % 4) % 4 + (misalign ? 1 : 0);
  V z(R * T * n, NAN), a(R * T * p, NAN);
  std::vector<int32_t> lv(BT, -7);
  kvae_psample_problem pr{};
  pr.B = B, pr.S = S, pr.T = T, pr.n = n, pr.p = p;
  pr.mus_filt = mf.data(), pr.Sigmas_filt = Sf.data(), pr.mus_pred = mp.data(), pr.Sigmas_pred = Sp.data();
  const int64_t on = per_step ? 1 : 0;
  pr.A = {A.data(), on * T * n * n, on * n * n}, pr.C = {C.data(), on * T * p * n, on * p * n}, pr.Q = {Q.data(), on * T * n * n, on * n * n};
  pr.LR = LR.data(), pr.eta = eta.data();
  // the draws end exactly at the end of their buffer when misaligned by one float less than the slack: keep the exact size
  V eps_exact(epsbuf.begin() + skew, epsbuf.begin() + skew + R * T * n);
  pr.eps = misalign ? epsbuf.data() + skew : eps_exact.data();
  V ws((size_t)kvae_lgssm_posterior_sample_ws_floats(&pr), NAN);
  pr.z_out = z.data(), pr.a_out = a.data(), pr.levels_out = lv.data(), pr.ws = ws.data();
  if (kvae_lgssm_posterior_sample(&pr, nullptr) != KVAE_OK) return 1;   // the emulated entry point of csrc/lgssm_post.h
  for (const V *v : {&z, &a, &ws})
    for (float x : *v)
      if (!std::isfinite(x)) return 2;   // every output element written, nothing past them
  for (int32_t l : lv)
    if (l != 0) return 3;
  return 0;
}

int main() {
  const int rc[] = {run(3, 5, 7, 4, 2, true, false),    // 21 items: a ragged last wavefront of the n = 4 gains; 15 paths
                    run(2, 70, 3, 4, 2, false, false),  // 140 paths: three wavefronts, the last ragged; broadcast A, C, Q
                    run(2, 3, 5, 16, 2, true, false),   // n = 16
                    run(3, 2, 1, 4, 2, true, false),    // T = 1
                    run(2, 2, 1, 16, 3, true, false),
                    run(2, 3, 4, 5, 3, true, false),    // run-time n
                    run(2, 3, 4, 4, 2, true, true),     // misaligned draws: the scalar-load paths kernel
                    run(1, 3, 4, 16, 2, true, true)};
  int bad = 0;
  for (size_t i = 0; i < sizeof(rc) / sizeof(rc[0]); ++i) {
    printf("case %zu: %d\n", i, rc[i]);
    bad |= rc[i];
  }
  if (bad) return 1;
  printf("POST-ASAN-OK\n");
  return 0;
}
