// pred_asan_driver.cpp — TEST-ONLY: the three item bodies and the sequence sums of kvae_lgssm_predictive (csrc/lgssm_pred.h) on
// emulated wavefronts (wave_emu.h), as a standalone program that tests/test_predictive.py builds with
// -fsanitize=address,undefined and runs as a child process, through the host simulation's entry point defined there.  Every
// buffer is allocated at its exact size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.
// Shapes: one item (T = 1), ragged last wavefronts (111 items at n = 4 and a run-time n, 65 at n = 16), more sequences than a
// wavefront has lanes, T one past the stride of the sequence sums; C shared and per step out of a record with a row stride;
// a subset of the outputs.
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
      mask(masked ? items : 0);
  for (auto &x : mp) x = nd(g);
  for (auto &x : C) x = nd(g);
  for (auto &x : y) x = nd(g);
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
  std::vector<float> ll(items, NAN), nis(items, NAN), a_pred(items * p, NAN), S(items * p * p, NAN), seq(B, NAN);
  std::vector<int32_t> levels(items, -1);
  kvae_pred_problem P{};
  P.B = B, P.T = T, P.n = n, P.p = p;
  P.mus_pred = mp.data(), P.Sigmas_pred = Sp.data(), P.R = R.data(), P.y = y.data(), P.mask = masked ? mask.data() : nullptr;
  P.C = packed ? kvae_stack{C.data() + 4, (int64_t)T * E, E} : kvae_stack{C.data(), 0, 0};
  P.ll = ll.data(), P.nis = nis.data(), P.a_pred = a_pred.data(), P.S_out = S.data(), P.levels = levels.data(), P.seq_ll = seq.data();
  const int kind = kvae_pred::pred_kind(P);
  if (kind != (n == 4 ? 0 : (n == 16 ? 1 : 2))) return 1;   // heap vectors of floats are 16-byte aligned here
  const int before = kvae_wemu_predictive_launches(kind), before_seq = kvae_wemu_predictive_launches(3);
  if (kvae_lgssm_predictive(&P, nullptr)) return 2;
  if (kvae_wemu_predictive_launches(kind) != before + 1 || kvae_wemu_predictive_launches(3) != before_seq + 1) return 3;
  for (const auto *v : {&ll, &nis, &a_pred, &S, &seq})
    for (float x : *v)
      if (!std::isfinite(x)) return 4;   // every output element written
  for (int32_t l : levels)
    if (l != 0) return 5;
  for (size_t it = 0; it < mask.size(); ++it)
    if (mask[it] == 0.f && (ll[it] != 0.f || nis[it] != 0.f)) return 6;
  // a subset of the outputs: the same bits, nothing else touched
  std::vector<float> ll2(items, NAN), seq2(B, NAN);
  P.ll = ll2.data(), P.seq_ll = seq2.data(), P.nis = nullptr, P.a_pred = nullptr, P.S_out = nullptr, P.levels = nullptr;
  if (kvae_lgssm_predictive(&P, nullptr)) return 7;
  for (size_t e = 0; e < items; ++e)
    if (ll[e] != ll2[e]) return 8;
  for (int b = 0; b < B; ++b)
    if (seq[b] != seq2[b]) return 9;
  // operands one float off a 16-byte boundary: the run-time body
  std::vector<float> Sp2(Sp.size() + 1), a2(items * p, NAN);
  std::copy(Sp.begin(), Sp.end(), Sp2.begin() + 1);
  P.Sigmas_pred = Sp2.data() + 1, P.ll = nullptr, P.seq_ll = nullptr, P.a_pred = a2.data();
  if (kvae_pred::pred_kind(P) != 2) return 10;
  if (kvae_lgssm_predictive(&P, nullptr)) return 11;
  for (float x : a2)
    if (!std::isfinite(x)) return 12;
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
  printf("PRED-ASAN-OK\n");
  return 0;
}
