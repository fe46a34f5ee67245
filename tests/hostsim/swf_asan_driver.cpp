// swf_asan_driver.cpp — TEST-ONLY: the sweep and the sequence sums of kvae_lgssm_switching_filter (csrc/lgssm_swf.h) on emulated
// wavefronts (wave_emu.h), as a standalone program that tests/test_switching_filter.py builds with
// -fsanitize=address,undefined and runs as a child process, through the host simulation's entry point defined there.  Every
// buffer is allocated at its exact size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.
// Shapes: T = 1, K = 5 and K = 7 (padding lanes), a full grid of 8, run-time n and m below the padded 4, a mask, a subset of the
// outputs, a carried state (then without mu0 / Sigma0), T past the stride of the sequence sums.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_swf.h"
#include "switching_fixture.h"

static int run(int B, int T, int K, int n, int m, bool masked) {
  const int p = 2;
  SwitchingModel sw(B * 1000 + T * 10 + K, B, T, K, n, m, masked);
  const vec &mask = sw.mask;
  const size_t items = (size_t)B * T;
  std::vector<float> rf(items * K, NAN), rp(items * K, NAN), ll(items, NAN), seq(B, NAN), ap(items * p, NAN), S(items * p * p, NAN),
      mf(items * n, NAN), Sf(items * n * n, NAN), olw((size_t)B * K, NAN), omu((size_t)B * K * n, NAN), oS((size_t)B * K * n * n, NAN);
  std::vector<int32_t> levels(items, -1);
  kvae_swf_problem P{};
  sw.bind(P);
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
    std::vector<float> y1 = chunk(sw.y, T, p, 0, T1), u1 = chunk(sw.u, T, m, 0, T1), k1 = chunk(mask, T, 1, 0, T1), y2 = chunk(sw.y, T, p, T1, T),
        u2 = chunk(sw.u, T, m, T1, T), k2 = chunk(mask, T, 1, T1, T), rfa((size_t)B * T1 * K, NAN), rfb((size_t)B * T2 * K, NAN),
        lw1((size_t)B * K, NAN), mu1((size_t)B * K * n, NAN), S1((size_t)B * K * n * n, NAN), lw2((size_t)B * K, NAN);
    kvae_swf_problem Pa{};
    sw.bind(Pa);
    Pa.T = T1, Pa.y = y1.data(), Pa.u = u1.data(), Pa.mask = masked ? k1.data() : nullptr;
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
  const Shape shapes[] = {{1, 1, 1, 4, 2}, {2, 1, 5, 4, 2}, {3, 4, 5, 3, 1}, {2, 5, 7, 4, 4}, {2, 3, 8, 2, 3}, {3, 2, 3, 1, 1}, {1, 66, 2, 4, 2}};
  return run_shapes(shapes, "SWF-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.T, s.K, s.n, s.m, masked); });
}
