// spf_asan_driver.cpp — TEST-ONLY: the sweep, the lineage walk and the sequence sums of kvae_lgssm_switching_pf
// (csrc/lgssm_spf.h) on emulated workgroups (wave_emu.h), as a standalone program that tests/test_particle_filter.py builds with
// -fsanitize=address,undefined and runs as a child process, through the host simulation's entry point defined there.  Every
// buffer is allocated at its exact size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report; the
// LDS arrays of the emulated workgroup are heap objects of their exact size too.
// Shapes: T = 1, K = 5 / 7 / 8 (table padding), run-time n and m below the padded 4, a mask, a subset of the outputs, a carried
// state (then without mu0 / Sigma0), N = 64 and 256, ess_threshold 0 / 0.5 / 1, T past the stride of the sequence sums.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_spf.h"
#include "switching_fixture.h"

static int run(int B, int G, int T, int K, int n, int m, int N, float thr, bool masked) {
  const int p = 2;
  SwitchingModel sw(B * 1000 + T * 10 + K + N, B, T, K, n, m, masked);
  const vec &mask = sw.mask;
  std::uniform_real_distribution<float> ud(0.f, 1.f);
  const size_t reps = (size_t)B * G, steps = reps * T, parts = reps * N;
  std::vector<float> th(steps * N), ph(steps);   // the draws: after the model, from its generator
  for (auto *v : {&th, &ph})
    for (auto &x : *v) x = std::min(ud(sw.g), 0.99999994f);
  std::vector<float> ll(steps, NAN), seq(reps, NAN), rf(steps * K, NAN), mf(steps * n, NAN), Sf(steps * n * n, NAN), ess(steps, NAN),
      olw(parts, NAN), omu(parts * n, NAN), oS(parts * n * n, NAN);
  std::vector<int32_t> rs(steps, -1), rg(steps * N, -1), an(steps * N, -1), levels(steps, -1), paths(parts * T, -1), oreg(parts, -1);
  kvae_spf_problem P{};
  sw.bind(P);
  P.G = G, P.N = N, P.ess_threshold = thr, P.pf_regime = th.data(), P.pf_resample = ph.data();
  P.ll = ll.data(), P.seq_ll = seq.data(), P.regime_filt = rf.data(), P.mus_filt = mf.data(), P.Sigmas_filt = Sf.data(), P.ess = ess.data();
  P.resampled = rs.data(), P.regimes = rg.data(), P.ancestors = an.data(), P.levels = levels.data(), P.paths = paths.data();
  P.out_log_w = olw.data(), P.out_regime = oreg.data(), P.out_mu = omu.data(), P.out_Sigma = oS.data();
  int before[3];
  for (int i = 0; i < 3; ++i) before[i] = kvae_wemu_switching_pf_launches(i);
  if (kvae_lgssm_switching_pf(&P, nullptr)) return 1;
  for (int i = 0; i < 3; ++i)
    if (kvae_wemu_switching_pf_launches(i) != before[i] + 1) return 2;
  for (const auto *v : {&ll, &seq, &rf, &mf, &Sf, &ess, &olw, &omu, &oS})
    if (!finite_all(*v)) return 3;   // every output element written
  for (int32_t l : levels)
    if (l != 0) return 4;
  for (size_t s = 0; s < steps; ++s) {
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += rf[s * K + k];
    if (fabsf(sum - 1.f) > 1e-5f) return 5;
    const size_t it = (s / ((size_t)G * T)) * T + s % T;
    if (masked && mask[it] == 0.f && ll[s] != 0.f) return 6;
    if (!(ess[s] >= 0.999f && ess[s] <= N * 1.001f)) return 7;
    if (rs[s] != (thr >= 1.f ? 1 : (thr <= 0.f ? 0 : (ess[s] < thr * N ? 1 : 0)))) return 8;
    for (int i = 0; i < N; ++i) {
      const int32_t r = rg[s * N + i], a = an[s * N + i];
      if (r < 0 || r >= K || a < 0 || a >= N || (!rs[s] && a != i)) return 9;
    }
  }
  for (size_t e = 0; e < parts; ++e) {
    if (oreg[e] < 0 || oreg[e] >= K) return 10;
    for (int t = 0; t < T; ++t)
      if (paths[e * T + t] < 0 || paths[e * T + t] >= K) return 11;
  }
  if (T > 8) return 0;   // the long shape is there for the prefetch and the strided sums only
  // a subset of the outputs: the same bits
  std::vector<float> rf2(steps * K, NAN), seq2(reps, NAN), ll2(steps, NAN);
  kvae_spf_problem P2 = P;
  P2.mus_filt = nullptr, P2.Sigmas_filt = nullptr, P2.ess = nullptr, P2.resampled = nullptr, P2.regimes = nullptr, P2.ancestors = nullptr;
  P2.levels = nullptr, P2.paths = nullptr, P2.out_log_w = nullptr, P2.out_regime = nullptr, P2.out_mu = nullptr, P2.out_Sigma = nullptr;
  P2.regime_filt = rf2.data(), P2.ll = ll2.data(), P2.seq_ll = seq2.data();
  if (kvae_lgssm_switching_pf(&P2, nullptr)) return 12;
  if (rf != rf2 || ll != ll2 || seq != seq2) return 13;
  // the second half from the carried state of the first, with its slices of the draws: the bits of the whole
  if (T >= 2) {
    const int T1 = T / 2, T2 = T - T1;
    std::vector<float> y1 = chunk(sw.y, T, p, 0, T1), u1 = chunk(sw.u, T, m, 0, T1), k1 = chunk(mask, T, 1, 0, T1), y2 = chunk(sw.y, T, p, T1, T),
        u2 = chunk(sw.u, T, m, T1, T), k2 = chunk(mask, T, 1, T1, T), th1 = chunk(th, T, N, 0, T1), th2 = chunk(th, T, N, T1, T),
        ph1 = chunk(ph, T, 1, 0, T1), ph2 = chunk(ph, T, 1, T1, T), rfa(reps * T1 * K, NAN), rfb(reps * T2 * K, NAN), lw1(parts, NAN),
        mu1(parts * n, NAN), S1(parts * n * n, NAN), lw2(parts, NAN);
    std::vector<int32_t> reg1(parts, -1), reg2(parts, -1);
    kvae_spf_problem Pa{};
    sw.bind(Pa);
    Pa.G = G, Pa.N = N, Pa.ess_threshold = thr, Pa.T = T1, Pa.y = y1.data(), Pa.u = u1.data(), Pa.mask = masked ? k1.data() : nullptr;
    Pa.pf_regime = th1.data(), Pa.pf_resample = ph1.data();
    Pa.regime_filt = rfa.data(), Pa.out_log_w = lw1.data(), Pa.out_regime = reg1.data(), Pa.out_mu = mu1.data(), Pa.out_Sigma = S1.data();
    if (kvae_lgssm_switching_pf(&Pa, nullptr)) return 14;
    kvae_spf_problem Pb = Pa;
    Pb.T = T2, Pb.mu0 = nullptr, Pb.Sigma0 = nullptr, Pb.y = y2.data(), Pb.u = u2.data(), Pb.mask = masked ? k2.data() : nullptr;
    Pb.pf_regime = th2.data(), Pb.pf_resample = ph2.data();
    Pb.state_log_w = lw1.data(), Pb.state_regime = reg1.data(), Pb.state_mu = mu1.data(), Pb.state_Sigma = S1.data();
    Pb.regime_filt = rfb.data(), Pb.out_log_w = lw2.data(), Pb.out_regime = reg2.data(), Pb.out_mu = nullptr, Pb.out_Sigma = nullptr;
    if (kvae_lgssm_switching_pf(&Pb, nullptr)) return 15;
    for (size_t r = 0; r < reps; ++r)
      for (int t = 0; t < T; ++t)
        for (int k = 0; k < K; ++k) {
          const float w = rf[(r * T + t) * K + k];
          const float c = t < T1 ? rfa[(r * T1 + t) * K + k] : rfb[(r * T2 + (t - T1)) * K + k];
          if (w != c) return 16;
        }
    if (lw2 != olw || reg2 != oreg) return 17;
  }
  // error paths write nothing
  kvae_spf_problem Pe = P;
  Pe.K = 9;
  if (kvae_lgssm_switching_pf(&Pe, nullptr) != KVAE_ERR_ARG) return 18;
  Pe = P, Pe.N = 96;
  if (kvae_lgssm_switching_pf(&Pe, nullptr) != KVAE_ERR_ARG) return 19;
  Pe = P, Pe.A = nullptr;
  if (kvae_lgssm_switching_pf(&Pe, nullptr) != KVAE_ERR_NULL) return 20;
  Pe = P, Pe.regimes = nullptr;
  if (kvae_lgssm_switching_pf(&Pe, nullptr) != KVAE_ERR_NULL) return 21;
  return 0;
}

int main() {
  // B, T, K, n, m, (no horizon,) G, N, ess_threshold
  const Shape shapes[] = {{1, 1, 1, 4, 2, 0, 1, 64, 0.5f},  {2, 1, 5, 4, 2, 0, 1, 64, 1.f},    {2, 4, 5, 3, 1, 0, 2, 64, 0.5f}, {1, 5, 7, 4, 4, 0, 2, 256, 1.f},
                          {2, 3, 8, 2, 3, 0, 1, 128, 0.f},  {1, 2, 3, 1, 1, 0, 1, 256, 0.5f}, {1, 66, 2, 4, 2, 0, 1, 64, 0.5f}};
  return run_shapes(shapes, "SPF-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.G, s.T, s.K, s.n, s.m, s.N, s.thr, masked); });
}
