// pred_bwd_asan_driver.cpp — TEST-ONLY: the three adjoint bodies of kvae_lgssm_predictive_bwd (csrc/lgssm_pred.h) on emulated
// wavefronts (wave_emu.h), as a standalone program that tests/test_predictive_grad.py builds with -fsanitize=address,undefined
// and runs as a child process, through the host simulation's entry point defined there.  Every buffer is allocated at its exact
// size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.
// Shapes: one item (T = 1), ragged last wavefronts (111 items at n = 4 and a run-time n, 65 at n = 16), more sequences than a
// wavefront has lanes; C shared with gC in a [B,T,p,n] buffer, and C per step out of a record with gC in the same slot of a
// gradient record that ends with the last item's slot (nothing after it to write into); a subset of the outputs; outputs one
// float off a 16-byte boundary (the run-time body).
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include <random>
#include <vector>

#include "../../kalman-vae_amd/csrc/lgssm_pred.h"

static int run(int B, int T, int n, bool packed, bool masked) {
  const int p = 2;
  std::mt19937 g(B * 1000 + T * 10 + n);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t items = (size_t)B * T;
  const int E = packed ? 4 + p * n + 4 : 0;   // record row: 4 floats | C_t | 4 floats
  std::vector<float> mp(items * n), Sp(items * n * n), C(packed ? items * E : (size_t)p * n), R = {9e-4f, 0.f, 0.f, 9e-4f}, y(items * p),
      mask(masked ? items : 0), g_ll(items), g_seq(B);
  for (auto *v : {&mp, &C, &y, &g_ll, &g_seq})
    for (auto &x : *v) x = nd(g);
  for (size_t it = 0; it < items; ++it) {   // Sigma = M M^T / n + 0.5 I
    std::vector<float> M((size_t)n * n);
    for (auto &x : M) x = nd(g);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        float s = i == j ? 0.5f : 0.f;
        for (int k = 0; k < n; ++k) s += M[(size_t)i * n + k] * M[(size_t)j * n + k] / n;
        Sp[it * n * n + (size_t)i * n + j] = s;
      }
  }
  for (size_t it = 0; it < mask.size(); ++it) mask[it] = it % 3 == 1 ? 0.f : 1.f;
  kvae_pred_problem P{};
  P.B = B, P.T = T, P.n = n, P.p = p;
  P.mus_pred = mp.data(), P.Sigmas_pred = Sp.data(), P.R = R.data(), P.y = y.data(), P.mask = masked ? mask.data() : nullptr;
  P.C = packed ? kvae_stack{C.data() + 4, (int64_t)T * E, E} : kvae_stack{C.data(), 0, 0};
  // gC: per item, or the slot of a gradient record cut right behind the last item's slot
  const size_t gc_floats = packed ? (items - 1) * E + 4 + (size_t)p * n : items * p * n;
  std::vector<float> g_mu(items * n, NAN), g_Sig(items * n * n, NAN), gY(items * p, NAN), gC(gc_floats, NAN);
  kvae_pred_grads G{};
  G.g_ll = g_ll.data(), G.g_seq = g_seq.data();
  G.g_mus_pred = g_mu.data(), G.g_Sigmas_pred = g_Sig.data(), G.gY = gY.data();
  G.gC = packed ? kvae_gstack{gC.data() + 4, (int64_t)T * E, E} : kvae_gstack{gC.data(), (int64_t)T * p * n, p * n};
  const int kind = kvae_pred::pred_bwd_kind(P, G);
  if (kind != (n == 4 ? 0 : (n == 16 ? 1 : 2))) return 1;   // heap vectors of floats are 16-byte aligned here
  const int before = kvae_wemu_predictive_bwd_launches(kind);
  if (kvae_lgssm_predictive_bwd(&P, &G, nullptr)) return 2;
  if (kvae_wemu_predictive_bwd_launches(kind) != before + 1) return 3;
  for (const auto *v : {&g_mu, &g_Sig, &gY})
    for (float x : *v)
      if (!std::isfinite(x)) return 4;   // every output element written
  for (size_t it = 0; it < items; ++it)
    for (int e = 0; e < (packed ? E : p * n); ++e) {
      if (packed && it == items - 1 && e >= 4 + p * n) break;   // the record ends with the last slot
      const float x = gC[packed ? it * E + e : it * p * n + e];
      const bool slot = !packed || (e >= 4 && e < 4 + p * n);
      if (slot ? !std::isfinite(x) : !std::isnan(x)) return 5;  // the slot written, nothing outside it
    }
  for (size_t it = 0; it < mask.size(); ++it)
    if (mask[it] == 0.f) {
      for (int j = 0; j < n; ++j)
        if (g_mu[it * n + j] != 0.f) return 6;
      for (int j = 0; j < n * n; ++j)
        if (g_Sig[it * n * n + j] != 0.f) return 6;
      if (gY[it * 2] != 0.f || gY[it * 2 + 1] != 0.f) return 6;
    }
  // a subset of the outputs, one upstream: nothing else touched, g_Sigma of the g_seq-only call finite
  std::vector<float> g_Sig2(items * n * n, NAN);
  G.g_ll = nullptr, G.g_mus_pred = nullptr, G.gY = nullptr, G.gC = kvae_gstack{nullptr, 0, 0}, G.g_Sigmas_pred = g_Sig2.data();
  if (kvae_lgssm_predictive_bwd(&P, &G, nullptr)) return 7;
  for (float x : g_Sig2)
    if (!std::isfinite(x)) return 8;
  // the full call again: the same bits
  std::vector<float> g_mu3(items * n, NAN), g_Sig3(items * n * n, NAN);
  G.g_ll = g_ll.data(), G.g_mus_pred = g_mu3.data(), G.g_Sigmas_pred = g_Sig3.data();
  if (kvae_lgssm_predictive_bwd(&P, &G, nullptr)) return 9;
  if (memcmp(g_mu3.data(), g_mu.data(), g_mu.size() * 4) || memcmp(g_Sig3.data(), g_Sig.data(), g_Sig.size() * 4)) return 10;
  // outputs one float off a 16-byte boundary: the run-time body, the same values as the aligned call up to the summation order
  std::vector<float> g_Sig4(items * n * n + 1, NAN), gC4(items * p * n + 1, NAN);
  G.g_mus_pred = nullptr, G.g_Sigmas_pred = g_Sig4.data() + 1, G.gC = kvae_gstack{gC4.data() + 1, (int64_t)T * p * n, p * n};
  if (kvae_pred::pred_bwd_kind(P, G) != 2) return 11;
  if (kvae_lgssm_predictive_bwd(&P, &G, nullptr)) return 12;
  for (size_t e = 1; e < g_Sig4.size(); ++e)
    if (!std::isfinite(g_Sig4[e])) return 13;
  for (size_t e = 1; e < gC4.size(); ++e)
    if (!std::isfinite(gC4[e])) return 14;
  if (!std::isnan(g_Sig4[0]) || !std::isnan(gC4[0])) return 15;
  return 0;
}

int main() {
  const int shapes[8][3] = {{1, 1, 4}, {3, 37, 4}, {65, 2, 4}, {2, 65, 4}, {1, 1, 16}, {5, 13, 16}, {3, 37, 3}, {2, 5, 7}};
  int bad = 0;
  for (const auto &s : shapes)
    for (int variant = 0; variant < 2; ++variant) {
      const int rc = run(s[0], s[1], s[2], variant == 1, variant == 1);
      printf("(%d,%d,%d) %s %d\n", s[0], s[1], s[2], variant ? "packed, masked" : "shared", rc);
      bad += rc != 0;
    }
  if (bad) return 1;
  printf("PRED-BWD-ASAN-OK\n");
  return 0;
}
