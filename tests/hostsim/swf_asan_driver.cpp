// swf_asan_driver.cpp — TEST-ONLY: the sweep and the sequence sums of kvae_lgssm_switching_filter (csrc/lgssm_swf.h) on emulated
// wavefronts (wave_emu.h), as a standalone program that tests/test_switching_filter.py builds with
// -fsanitize=address,undefined and runs as a child process, through the host simulation's entry point defined there.  Every
// buffer is allocated at its exact size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.
// Shapes: T = 1, K = 5 and K = 7 (padding lanes), a full grid of 8, run-time n and m below the padded 4, a mask, a subset of the
// outputs, a carried state (then without mu0 / Sigma0), T past the stride of the sequence sums.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include <random>
#include <vector>

#include "../../kalman-vae_amd/csrc/lgssm_swf.h"

static bool finite_all(const std::vector<float> &v) {
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

static int run(int B, int T, int K, int n, int m, bool masked) {
  const int p = 2;
  std::mt19937 g(B * 1000 + T * 10 + K);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t items = (size_t)B * T;
  std::vector<float> A((size_t)K * n * n, 0.f), Bm((size_t)K * n * m), Q((size_t)K * n * n, 0.f), C((size_t)p * n), R = {0.05f, 0.f, 0.f, 0.05f},
      Pm((size_t)K * K), mu0(n), Sigma0((size_t)n * n, 0.f), y(items * p), u(items * m), mask(masked ? items : 0);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n; ++i) {
      A[((size_t)k * n + i) * n + i] = 0.9f - 0.05f * k;
      if (i + 1 < n) A[((size_t)k * n + i) * n + i + 1] = 0.1f * (k % 2 ? 1.f : -1.f);
      Q[((size_t)k * n + i) * n + i] = 0.02f + 0.01f * k;
    }
  for (int i = 0; i < n; ++i) Sigma0[(size_t)i * n + i] = 0.5f;
  for (auto *v : {&Bm, &C, &mu0, &y, &u})
    for (auto &x : *v) x = 0.5f * nd(g);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) Pm[(size_t)i * K + j] = K == 1 ? 1.f : (i == j ? 0.8f : 0.2f / (K - 1));
  for (size_t it = 0; it < mask.size(); ++it) mask[it] = it % 3 == 1 ? 0.f : 1.f;
  std::vector<float> rf(items * K, NAN), rp(items * K, NAN), ll(items, NAN), seq(B, NAN), ap(items * p, NAN), S(items * p * p, NAN),
      mf(items * n, NAN), Sf(items * n * n, NAN), olw((size_t)B * K, NAN), omu((size_t)B * K * n, NAN), oS((size_t)B * K * n * n, NAN);
  std::vector<int32_t> levels(items, -1);
  kvae_swf_problem P{};
  P.B = B, P.T = T, P.K = K, P.n = n, P.m = m, P.p = p;
  P.A = A.data(), P.Bm = Bm.data(), P.Q = Q.data(), P.C = C.data(), P.R = R.data(), P.P = Pm.data(), P.mu0 = mu0.data();
  P.Sigma0 = Sigma0.data(), P.y = y.data(), P.u = u.data(), P.mask = masked ? mask.data() : nullptr;
  P.regime_filt = rf.data(), P.regime_pred = rp.data(), P.ll = ll.data(), P.seq_ll = seq.data(), P.a_pred = ap.data(), P.S_out = S.data();
  P.mus_filt = mf.data(), P.Sigmas_filt = Sf.data(), P.levels = levels.data(), P.out_log_w = olw.data(), P.out_mu = omu.data();
  P.out_Sigma = oS.data();
  const int b0 = kvae_wemu_switching_filter_launches(0), b1 = kvae_wemu_switching_filter_launches(1);
  if (kvae_lgssm_switching_filter(&P, nullptr)) return 1;
  if (kvae_wemu_switching_filter_launches(0) != b0 + 1 || kvae_wemu_switching_filter_launches(1) != b1 + 1) return 2;
  for (const auto *v : {&rf, &rp, &ll, &seq, &ap, &S, &mf, &Sf, &olw, &omu, &oS})
    if (!finite_all(*v)) return 3;   // every output element written
  for (int32_t l : levels)
    if (l != 0) return 4;
  for (size_t it = 0; it < items; ++it) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += rf[it * K + k];
    if (fabsf(s - 1.f) > 1e-5f) return 5;
    if (masked && mask[it] == 0.f && ll[it] != 0.f) return 6;
  }
  if (T > 8) return 0;   // the long shape is there for the prefetch and the strided sums only
  // a subset of the outputs: the same bits
  std::vector<float> rf2(items * K, NAN), seq2(B, NAN), ll2(items, NAN);
  kvae_swf_problem P2 = P;
  P2.regime_pred = nullptr, P2.a_pred = nullptr, P2.S_out = nullptr, P2.mus_filt = nullptr, P2.Sigmas_filt = nullptr, P2.levels = nullptr;
  P2.out_log_w = nullptr, P2.out_mu = nullptr, P2.out_Sigma = nullptr;
  P2.regime_filt = rf2.data(), P2.ll = ll2.data(), P2.seq_ll = seq2.data();
  if (kvae_lgssm_switching_filter(&P2, nullptr)) return 7;
  if (rf != rf2 || ll != ll2 || seq != seq2) return 8;
  // the second half from the carried state of the first: the bits of the whole
  if (T >= 2) {
    const int T1 = T / 2, T2 = T - T1;
    std::vector<float> y1((size_t)B * T1 * p), u1((size_t)B * T1 * m), k1(masked ? (size_t)B * T1 : 0), y2((size_t)B * T2 * p),
        u2((size_t)B * T2 * m), k2(masked ? (size_t)B * T2 : 0), rfa((size_t)B * T1 * K, NAN), rfb((size_t)B * T2 * K, NAN),
        lw1((size_t)B * K, NAN), mu1((size_t)B * K * n, NAN), S1((size_t)B * K * n * n, NAN), lw2((size_t)B * K, NAN);
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < T; ++t) {
        const size_t src = (size_t)b * T + t, dst = t < T1 ? (size_t)b * T1 + t : (size_t)b * T2 + (t - T1);
        for (int c = 0; c < p; ++c) (t < T1 ? y1 : y2)[dst * p + c] = y[src * p + c];
        for (int c = 0; c < m; ++c) (t < T1 ? u1 : u2)[dst * m + c] = u[src * m + c];
        if (masked) (t < T1 ? k1 : k2)[dst] = mask[src];
      }
    kvae_swf_problem Pa{};
    Pa.B = B, Pa.T = T1, Pa.K = K, Pa.n = n, Pa.m = m, Pa.p = p;
    Pa.A = A.data(), Pa.Bm = Bm.data(), Pa.Q = Q.data(), Pa.C = C.data(), Pa.R = R.data(), Pa.P = Pm.data(), Pa.mu0 = mu0.data();
    Pa.Sigma0 = Sigma0.data(), Pa.y = y1.data(), Pa.u = u1.data(), Pa.mask = masked ? k1.data() : nullptr;
    Pa.regime_filt = rfa.data(), Pa.out_log_w = lw1.data(), Pa.out_mu = mu1.data(), Pa.out_Sigma = S1.data();
    if (kvae_lgssm_switching_filter(&Pa, nullptr)) return 9;
    kvae_swf_problem Pb = Pa;
    Pb.T = T2, Pb.mu0 = nullptr, Pb.Sigma0 = nullptr, Pb.y = y2.data(), Pb.u = u2.data(), Pb.mask = masked ? k2.data() : nullptr;
    Pb.state_log_w = lw1.data(), Pb.state_mu = mu1.data(), Pb.state_Sigma = S1.data();
    Pb.regime_filt = rfb.data(), Pb.out_log_w = lw2.data(), Pb.out_mu = nullptr, Pb.out_Sigma = nullptr;
    if (kvae_lgssm_switching_filter(&Pb, nullptr)) return 10;
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < T; ++t)
        for (int k = 0; k < K; ++k) {
          const float w = rf[((size_t)b * T + t) * K + k];
          const float c = t < T1 ? rfa[((size_t)b * T1 + t) * K + k] : rfb[((size_t)b * T2 + (t - T1)) * K + k];
          if (w != c) return 11;
        }
    if (lw2 != olw) return 12;
  }
  // error paths write nothing
  kvae_swf_problem Pe = P;
  Pe.K = 9;
  if (kvae_lgssm_switching_filter(&Pe, nullptr) != KVAE_ERR_ARG) return 13;
  Pe = P, Pe.A = nullptr;
  if (kvae_lgssm_switching_filter(&Pe, nullptr) != KVAE_ERR_NULL) return 14;
  return 0;
}

int main() {
  const int shapes[7][5] = {{1, 1, 1, 4, 2}, {2, 1, 5, 4, 2}, {3, 4, 5, 3, 1}, {2, 5, 7, 4, 4}, {2, 3, 8, 2, 3}, {3, 2, 3, 1, 1}, {1, 66, 2, 4, 2}};
  int bad = 0;
  for (const auto &s : shapes)
    for (int variant = s[1] > 8 ? 1 : 0; variant < 2; ++variant) {   // the long one once
      const int rc = run(s[0], s[1], s[2], s[3], s[4], variant == 1);
      printf("(%d,%d,%d,%d,%d) %s %d\n", s[0], s[1], s[2], s[3], s[4], variant ? "masked" : "observed", rc);
      bad += rc != 0;
    }
  if (bad) return 1;
  printf("SWF-ASAN-OK\n");
  return 0;
}
