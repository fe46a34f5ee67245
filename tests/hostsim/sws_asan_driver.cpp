// sws_asan_driver.cpp — TEST-ONLY: the forward (csrc/lgssm_swf.h, history kept) and the backward (csrc/lgssm_sws.h) of
// kvae_lgssm_switching_smoother on emulated wavefronts (wave_emu.h), as a standalone program that tests/test_switching_smoother.py
// builds with -fsanitize=address,undefined and runs as a child process, through the host simulation's entry point defined there.
// Every buffer is allocated at its exact size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.
// Shapes: T = 1 and T = 2, K = 5 and K = 7 (padding lanes), a full grid of 8, run-time n = 3 and m = 1, a mask, NULL outputs in
// several combinations, a carried state (then without mu0 / Sigma0), T = 66, the error codes.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_sws.h"
#include "switching_fixture.h"

static int run(int B, int T, int K, int n, int m, bool masked) {
  SwitchingModel sw(B * 1000 + T * 10 + K, B, T, K, n, m, masked);
  const size_t items = (size_t)B * T, pitems = (size_t)B * (T > 1 ? T - 1 : 1);
  std::vector<float> rf(items * K, NAN), ll(items, NAN), seq(B, NAN), mf(items * n, NAN), olw((size_t)B * K, NAN), omu((size_t)B * K * n, NAN),
      oS((size_t)B * K * n * n, NAN);
  std::vector<float> hmu(items * K * n, NAN), hS(items * K * n * n, NAN), hW(items * K * K, NAN), hw((size_t)B * K, NAN);
  std::vector<float> rs(items * K, NAN), rp(pitems * K * K, NAN), ms(items * n, NAN), Ss(items * n * n, NAN);
  kvae_sws_problem S{};
  kvae_swf_problem &P = S.filt;
  sw.bind(P);
  P.regime_filt = rf.data(), P.ll = ll.data(), P.seq_ll = seq.data(), P.mus_filt = mf.data();
  P.out_log_w = olw.data(), P.out_mu = omu.data(), P.out_Sigma = oS.data();
  S.hist_mu = hmu.data(), S.hist_Sigma = hS.data(), S.hist_W = hW.data(), S.hist_w = hw.data();
  S.regime_smooth = rs.data(), S.regime_pairs = rp.data(), S.mus_smooth = ms.data(), S.Sigmas_smooth = Ss.data();
  const int b0 = kvae_wemu_switching_smoother_launches(0), b1 = kvae_wemu_switching_smoother_launches(1),
            b2 = kvae_wemu_switching_smoother_launches(2);
  if (kvae_lgssm_switching_smoother(&S, nullptr)) return 1;
  if (kvae_wemu_switching_smoother_launches(0) != b0 + 1 || kvae_wemu_switching_smoother_launches(1) != b1 + 1 ||
      kvae_wemu_switching_smoother_launches(2) != b2 + 1)
    return 2;
  for (const auto *v : {&rf, &ll, &seq, &mf, &olw, &omu, &oS, &hmu, &hS, &hW, &hw, &rs, &ms, &Ss})
    if (!finite_all(*v)) return 3;   // every element written
  if (T > 1 && !finite_all(rp)) return 3;
  if (T == 1) {   // nothing written to regime_pairs; the smoother is the filter
    for (float x : rp)
      if (!std::isnan(x)) return 4;
    if (rs != rf || ms != mf) return 5;
  }
  for (size_t it = 0; it < items; ++it) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += rs[it * K + k];
    if (fabsf(s - 1.f) > 1e-4f) return 6;
  }
  // the filter keys are the filter's own bits
  {
    std::vector<float> rf2(items * K, NAN), mf2(items * n, NAN), olw2((size_t)B * K, NAN);
    kvae_swf_problem F = P;
    F.regime_filt = rf2.data(), F.mus_filt = mf2.data(), F.out_log_w = olw2.data();
    F.ll = nullptr, F.seq_ll = nullptr, F.out_mu = nullptr, F.out_Sigma = nullptr;
    if (kvae_lgssm_switching_filter(&F, nullptr)) return 7;
    if (rf2 != rf || mf2 != mf || olw2 != olw) return 8;
  }
  if (T > 8) return 0;   // the long shape is there for the prefetch only
  // subsets of the outputs: the same bits
  {
    std::vector<float> rs2(items * K, NAN), ms2(items * n, NAN), rp2(pitems * K * K, NAN), Ss2(items * n * n, NAN);
    kvae_sws_problem S2 = S;
    S2.filt.regime_filt = nullptr, S2.filt.ll = nullptr, S2.filt.seq_ll = nullptr, S2.filt.mus_filt = nullptr;
    S2.filt.out_log_w = nullptr, S2.filt.out_mu = nullptr, S2.filt.out_Sigma = nullptr;
    S2.regime_smooth = rs2.data(), S2.mus_smooth = ms2.data(), S2.regime_pairs = nullptr, S2.Sigmas_smooth = nullptr;
    if (kvae_lgssm_switching_smoother(&S2, nullptr)) return 9;
    if (rs2 != rs || ms2 != ms) return 10;
    S2.regime_smooth = nullptr, S2.mus_smooth = nullptr, S2.regime_pairs = rp2.data(), S2.Sigmas_smooth = Ss2.data();
    if (kvae_lgssm_switching_smoother(&S2, nullptr)) return 11;
    if (Ss2 != Ss) return 12;
    if (T > 1 && rp2 != rp) return 12;
    // no smoother output at all: the forward alone
    const int f0 = kvae_wemu_switching_smoother_launches(0), f1 = kvae_wemu_switching_smoother_launches(1);
    kvae_sws_problem S3 = S;
    S3.regime_smooth = nullptr, S3.regime_pairs = nullptr, S3.mus_smooth = nullptr, S3.Sigmas_smooth = nullptr;
    if (kvae_lgssm_switching_smoother(&S3, nullptr)) return 13;
    if (kvae_wemu_switching_smoother_launches(0) != f0 + 1 || kvae_wemu_switching_smoother_launches(1) != f1) return 14;
  }
  // a carried state (without mu0 / Sigma0): the state the first call left
  {
    std::vector<float> rs2(items * K, NAN), ms2(items * n, NAN);
    kvae_sws_problem S4 = S;
    S4.filt.mu0 = nullptr, S4.filt.Sigma0 = nullptr;
    S4.filt.state_log_w = olw.data(), S4.filt.state_mu = omu.data(), S4.filt.state_Sigma = oS.data();
    S4.filt.out_log_w = nullptr, S4.filt.out_mu = nullptr, S4.filt.out_Sigma = nullptr;
    S4.regime_smooth = rs2.data(), S4.mus_smooth = ms2.data();
    if (kvae_lgssm_switching_smoother(&S4, nullptr)) return 15;
    if (!finite_all(rs2) || !finite_all(ms2)) return 16;
  }
  // error paths write nothing
  kvae_sws_problem Se = S;
  Se.filt.K = 9;
  if (kvae_lgssm_switching_smoother(&Se, nullptr) != KVAE_ERR_ARG) return 17;
  Se = S, Se.filt.A = nullptr;
  if (kvae_lgssm_switching_smoother(&Se, nullptr) != KVAE_ERR_NULL) return 18;
  Se = S, Se.hist_W = nullptr;
  if (kvae_lgssm_switching_smoother(&Se, nullptr) != KVAE_ERR_NULL) return 19;
  Se = S, Se.filt.T = 0;
  if (kvae_lgssm_switching_smoother(&Se, nullptr) != KVAE_ERR_DIMS) return 20;
  if (kvae_lgssm_switching_smoother(nullptr, nullptr) != KVAE_ERR_NULL) return 21;
  return 0;
}

int main() {
  const Shape shapes[] = {{1, 1, 1, 4, 2}, {2, 1, 5, 4, 2}, {2, 2, 7, 4, 2}, {3, 4, 5, 3, 1}, {2, 5, 7, 4, 4}, {2, 3, 8, 2, 3}, {3, 2, 3, 1, 1},
                          {1, 66, 2, 4, 2}};
  return run_shapes(shapes, "SWS-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.T, s.K, s.n, s.m, masked); });
}
