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

#include <random>
#include <vector>

#include "../../kalman-vae_amd/csrc/lgssm_swh.h"

static bool finite_all(const std::vector<float> &v) {
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

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
  std::mt19937 g(B * 1000 + T * 10 + K + H);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t items = (size_t)B * T;
  std::vector<float> A((size_t)K * n * n, 0.f), Bm((size_t)K * n * m), Q((size_t)K * n * n, 0.f), C((size_t)p * n), R = {0.05f, 0.f, 0.f, 0.05f},
      Pm((size_t)K * K), mu0(n), Sigma0((size_t)n * n, 0.f), y(items * p), ua((size_t)B * (T + H) * m), u(items * m), mask(masked ? items : 0);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n; ++i) {
      A[((size_t)k * n + i) * n + i] = 0.9f - 0.05f * k;
      if (i + 1 < n) A[((size_t)k * n + i) * n + i + 1] = 0.1f * (k % 2 ? 1.f : -1.f);
      Q[((size_t)k * n + i) * n + i] = 0.02f + 0.01f * k;
    }
  for (int i = 0; i < n; ++i) Sigma0[(size_t)i * n + i] = 0.5f;
  for (auto *v : {&Bm, &C, &mu0, &y, &ua})
    for (auto &x : *v) x = 0.5f * nd(g);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int c = 0; c < m; ++c) u[((size_t)b * T + t) * m + c] = ua[((size_t)b * (T + H) + t) * m + c];
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) Pm[(size_t)i * K + j] = K == 1 ? 1.f : (i == j ? 0.8f : 0.2f / (K - 1));
  for (size_t it = 0; it < mask.size(); ++it) mask[it] = it % 3 == 1 ? 0.f : 1.f;
  std::vector<float> rf(items * K, NAN), ll(items, NAN), seq(B, NAN), ap(items * p, NAN), olw((size_t)B * K, NAN), omu((size_t)B * K * n, NAN),
      oS((size_t)B * K * n * n, NAN), hlw(items * K, NAN), hmu(items * K * n, NAN), hS(items * K * n * n, NAN);
  Fore all(items * H, K, n);
  kvae_swh_problem F{};
  kvae_swf_problem &P = F.filt;
  P.B = B, P.T = T, P.K = K, P.n = n, P.m = m, P.p = p;
  P.A = A.data(), P.Bm = Bm.data(), P.Q = Q.data(), P.C = C.data(), P.R = R.data(), P.P = Pm.data(), P.mu0 = mu0.data();
  P.Sigma0 = Sigma0.data(), P.y = y.data(), P.u = u.data(), P.mask = masked ? mask.data() : nullptr;
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
    std::vector<float> y1((size_t)B * T1 * p), u1((size_t)B * T1 * m), k1(masked ? (size_t)B * T1 : 0), y2((size_t)B * T2 * p),
        u2((size_t)B * T2 * m), ua2((size_t)B * (T2 + H) * m), k2(masked ? (size_t)B * T2 : 0), lw1((size_t)B * K, NAN), mu1((size_t)B * K * n, NAN),
        S1((size_t)B * K * n * n, NAN), h1((size_t)B * T2 * K, NAN), h2((size_t)B * T2 * K * n, NAN), h3((size_t)B * T2 * K * n * n, NAN);
    for (int b = 0; b < B; ++b) {
      for (int t = 0; t < T; ++t) {
        const size_t src = (size_t)b * T + t, dst = t < T1 ? (size_t)b * T1 + t : (size_t)b * T2 + (t - T1);
        for (int c = 0; c < p; ++c) (t < T1 ? y1 : y2)[dst * p + c] = y[src * p + c];
        for (int c = 0; c < m; ++c) (t < T1 ? u1 : u2)[dst * m + c] = u[src * m + c];
        if (masked) (t < T1 ? k1 : k2)[dst] = mask[src];
      }
      for (int t = 0; t < T2 + H; ++t)
        for (int c = 0; c < m; ++c) ua2[((size_t)b * (T2 + H) + t) * m + c] = ua[((size_t)b * (T + H) + T1 + t) * m + c];
    }
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
  const int shapes[8][6] = {{1, 1, 1, 4, 2, 1}, {2, 1, 5, 4, 2, 3}, {3, 4, 5, 3, 1, 2}, {2, 5, 7, 4, 4, 7},
                            {2, 3, 8, 2, 3, 4}, {3, 2, 3, 1, 1, 1}, {2, 6, 8, 4, 2, 2}, {1, 66, 2, 4, 2, 3}};
  int bad = 0;
  for (const auto &s : shapes)
    for (int variant = s[1] > 8 ? 1 : 0; variant < 2; ++variant) {   // the long one once
      const int rc = run(s[0], s[1], s[2], s[3], s[4], s[5], variant == 1);
      printf("(%d,%d,%d,%d,%d,%d) %s %d\n", s[0], s[1], s[2], s[3], s[4], s[5], variant ? "masked" : "observed", rc);
      bad += rc != 0;
    }
  if (bad) return 1;
  printf("SWH-ASAN-OK\n");
  return 0;
}
