// swh_asan_driver.cpp — TEST-ONLY: the forward (csrc/lgssm_swf.h, history kept), the forecast (csrc/lgssm_swh.h) and the sequence
// sums of kvae_lgssm_switching_forecast on emulated wavefronts (wave_emu.h), as a standalone program that
// tests/test_switching_forecast.py builds with -fsanitize=address,undefined and runs as a child process, through the host
// simulation's entry point defined there.  Every buffer is allocated at its exact size, so a read or write past the layouts of
// include/kvae_lgssm.h is a sanitizer report.
// Shapes: T = 1, H = 1 and H > T, K = 5 / 7 / 8 (padding lanes and a full grid), run-time n and m below the padded 4, a mask, a
// subset of the outputs, a carried state (then without mu0 / Sigma0), t0 = T - 1, T past the stride of the sequence sums.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_swh.h"
#include "switching_fixture.h"

struct Fore {
  std::vector<float> rf, af, Sf, mf, Sg, ll;
  std::vector<int32_t> lv;
  Fore(size_t q, int K, int n)
      : rf(q * K, NAN), af(q * 2, NAN), Sf(q * 4, NAN), mf(q * n, NAN), Sg(q * n * n, NAN), ll(q, NAN), lv(q, -1) {}
  void bind(kvae_swh_problem &F) {
    F.regime_fore = rf.data(), F.a_fore = af.data(), F.S_fore = Sf.data(), F.mus_fore = mf.data(), F.Sigmas_fore = Sg.data();
    F.ll_fore = ll.data(), F.levels_fore = lv.data();
  }
  bool written() const {
    for (const auto *v : {&rf, &af, &Sf, &mf, &Sg, &ll})
      if (!finite_all(*v)) return false;
    for (int32_t l : lv)
      if (l != 0) return false;
    return true;
  }
};

static int run(int B, int T, int K, int n, int m, int H, bool masked) {
  const int p = 2;
  SwitchingModel sw(B * 1000 + T * 10 + K + H, B, T, K, n, m, masked, H);
  const vec &mask = sw.mask, &ua = sw.u_all;
  const size_t items = (size_t)B * T;
  std::vector<float> rf(items * K, NAN), ll(items, NAN), seq(B, NAN), ap(items * p, NAN), olw((size_t)B * K, NAN), omu((size_t)B * K * n, NAN),
      oS((size_t)B * K * n * n, NAN), hlw(items * K, NAN), hmu(items * K * n, NAN), hS(items * K * n * n, NAN);
  Fore all(items * H, K, n);
  kvae_swh_problem F{};
  kvae_swf_problem &P = F.filt;
  sw.bind(P);
  P.regime_filt = rf.data(), P.ll = ll.data(), P.seq_ll = seq.data(), P.a_pred = ap.data();
  P.out_log_w = olw.data(), P.out_mu = omu.data(), P.out_Sigma = oS.data();
  F.hist_lw = hlw.data(), F.hist_mu = hmu.data(), F.hist_Sigma = hS.data(), F.H = H, F.t0 = 0, F.u_all = ua.data();
  all.bind(F);
  int before[3];
  for (int i = 0; i < 3; ++i) before[i] = kvae_wemu_switching_forecast_launches(i);
  if (kvae_lgssm_switching_forecast(&F, nullptr)) return 1;
  for (int i = 0; i < 3; ++i)
    if (kvae_wemu_switching_forecast_launches(i) != before[i] + 1) return 2;
  for (const auto *v : {&rf, &ll, &seq, &ap, &olw, &omu, &oS, &hlw, &hmu, &hS})
    if (!finite_all(*v)) return 3;   // every output element written
  if (!all.written()) return 4;
  for (size_t q = 0; q < items * H; ++q) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += all.rf[q * K + k];
    if (fabsf(s - 1.f) > 1e-5f) return 5;
    const int t = (int)((q / H) % T), h = (int)(q % H) + 1;
    const size_t b = q / ((size_t)H * T);
    const bool valid = t + h < T && (!masked || mask[b * T + t + h] != 0.f);
    if (!valid && all.ll[q] != 0.f) return 6;
    if (valid && all.ll[q] == 0.f) return 7;
  }
  if (T > 8) return 0;   // the long shape is there for the prefetch and the strided sums only
  // the last origin alone, and a subset of the outputs: the same bits
  Fore last((size_t)B * H, K, n);
  kvae_swh_problem F2 = F;
  last.bind(F2);
  F2.t0 = T - 1, F2.S_fore = nullptr, F2.Sigmas_fore = nullptr, F2.levels_fore = nullptr;
  F2.filt.regime_filt = nullptr, F2.filt.ll = nullptr, F2.filt.seq_ll = nullptr, F2.filt.a_pred = nullptr;
  F2.filt.out_log_w = nullptr, F2.filt.out_mu = nullptr, F2.filt.out_Sigma = nullptr;
  if (kvae_lgssm_switching_forecast(&F2, nullptr)) return 8;
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < H; ++h) {
      const size_t qa = ((size_t)b * T + T - 1) * H + h, ql = (size_t)b * H + h;
      for (int k = 0; k < K; ++k)
        if (all.rf[qa * K + k] != last.rf[ql * K + k]) return 9;
      for (int c = 0; c < n; ++c)
        if (all.mf[qa * n + c] != last.mf[ql * n + c]) return 10;
      if (all.af[qa * 2] != last.af[ql * 2] || all.af[qa * 2 + 1] != last.af[ql * 2 + 1] || all.ll[qa] != last.ll[ql]) return 11;
    }
  // the second half from the carried state of the first (without mu0 / Sigma0): the forecasts of its origins are the bits of the whole
  if (T >= 2) {
    const int T1 = T / 2, T2 = T - T1;
    std::vector<float> y1 = chunk(sw.y, T, p, 0, T1), u1 = chunk(sw.u, T, m, 0, T1), k1 = chunk(mask, T, 1, 0, T1), y2 = chunk(sw.y, T, p, T1, T),
        u2 = chunk(sw.u, T, m, T1, T), ua2 = chunk(ua, T + H, m, T1, T + H), k2 = chunk(mask, T, 1, T1, T), lw1((size_t)B * K, NAN),
        mu1((size_t)B * K * n, NAN), S1((size_t)B * K * n * n, NAN), h1((size_t)B * T2 * K, NAN), h2((size_t)B * T2 * K * n, NAN),
        h3((size_t)B * T2 * K * n * n, NAN);
    kvae_swf_problem Pa = P;   // the first half: the filter alone keeps the state
    Pa.T = T1, Pa.y = y1.data(), Pa.u = u1.data(), Pa.mask = masked ? k1.data() : nullptr;
    Pa.regime_filt = nullptr, Pa.ll = nullptr, Pa.seq_ll = nullptr, Pa.a_pred = nullptr;
    Pa.out_log_w = lw1.data(), Pa.out_mu = mu1.data(), Pa.out_Sigma = S1.data();
    if (kvae_lgssm_switching_filter(&Pa, nullptr)) return 12;
    Fore rest((size_t)B * T2 * H, K, n);
    kvae_swh_problem Fb = F;
    rest.bind(Fb);
    Fb.filt = Pa;
    Fb.filt.T = T2, Fb.filt.mu0 = nullptr, Fb.filt.Sigma0 = nullptr, Fb.filt.y = y2.data(), Fb.filt.u = u2.data();
    Fb.filt.mask = masked ? k2.data() : nullptr, Fb.filt.out_log_w = nullptr, Fb.filt.out_mu = nullptr, Fb.filt.out_Sigma = nullptr;
    Fb.filt.state_log_w = lw1.data(), Fb.filt.state_mu = mu1.data(), Fb.filt.state_Sigma = S1.data();
    Fb.u_all = ua2.data(), Fb.hist_lw = h1.data(), Fb.hist_mu = h2.data(), Fb.hist_Sigma = h3.data();
    if (kvae_lgssm_switching_forecast(&Fb, nullptr)) return 13;
    if (!rest.written()) return 14;
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < T2; ++t)
        for (int h = 0; h < H; ++h) {
          const size_t qa = ((size_t)b * T + T1 + t) * H + h, qr = ((size_t)b * T2 + t) * H + h;
          for (int k = 0; k < K; ++k)
            if (all.rf[qa * K + k] != rest.rf[qr * K + k]) return 15;
          for (int c = 0; c < n * n; ++c)
            if (all.Sg[qa * n * n + c] != rest.Sg[qr * n * n + c]) return 16;
          if (all.ll[qa] != rest.ll[qr]) return 17;   // the second chunk ends where the sequence does
        }
  }
  // error paths write nothing
  kvae_swh_problem Fe = F;
  Fe.filt.K = 9;
  if (kvae_lgssm_switching_forecast(&Fe, nullptr) != KVAE_ERR_ARG) return 18;
  Fe = F, Fe.filt.A = nullptr;
  if (kvae_lgssm_switching_forecast(&Fe, nullptr) != KVAE_ERR_NULL) return 19;
  Fe = F, Fe.u_all = nullptr;
  if (kvae_lgssm_switching_forecast(&Fe, nullptr) != KVAE_ERR_NULL) return 20;
  Fe = F, Fe.H = 0;
  if (kvae_lgssm_switching_forecast(&Fe, nullptr) != KVAE_ERR_DIMS) return 21;
  Fe = F, Fe.t0 = T;
  if (kvae_lgssm_switching_forecast(&Fe, nullptr) != KVAE_ERR_ARG) return 22;
  return 0;
}

int main() {
  // B, T, K, n, m, H
  const Shape shapes[] = {{1, 1, 1, 4, 2, 1}, {2, 1, 5, 4, 2, 3}, {3, 4, 5, 3, 1, 2}, {2, 5, 7, 4, 4, 7},
                          {2, 3, 8, 2, 3, 4}, {3, 2, 3, 1, 1, 1}, {2, 6, 8, 4, 2, 2}, {1, 66, 2, 4, 2, 3}};
  return run_shapes(shapes, "SWH-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.T, s.K, s.n, s.m, s.H, masked); });
}
