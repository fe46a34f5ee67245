// em_asan_driver.cpp — TEST-ONLY: the forward (csrc/lgssm_swf.h, history kept), the backward with the statistics and the sum over the
// sequences (csrc/lgssm_em.h) of kvae_lgssm_switching_em on emulated wavefronts (wave_emu.h), as a standalone program that
// tests/test_switching_em.py builds with -fsanitize=address,undefined and runs as a child process, through the host simulation's
// entry point defined there.  Every buffer is allocated at its exact size, so a read or write past the layouts of
// include/kvae_lgssm.h is a sanitizer report.  Per shape the error codes come first, with every buffer checked untouched; then
// T = 1 and T = 2, K = 5 and K = 7 (padding lanes), a full grid of 8, run-time n = 3 and m = 1, a mask, NULL outputs in several
// combinations, T = 66.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_em.h"
#include "switching_fixture.h"

static bool launched(const int (&before)[4], int f, int b, int r, int s) {
  const int want[4] = {f, b, r, s};
  for (int i = 0; i < 4; ++i)
    if (kvae_wemu_switching_em_launches(i) != before[i] + want[i]) return false;
  return true;
}
static void counters(int (&c)[4]) {
  for (int i = 0; i < 4; ++i) c[i] = kvae_wemu_switching_em_launches(i);
}

static int run(int B, int T, int K, int n, int m, bool masked) {
  const int x = n + m;
  SwitchingModel sw(B * 1000 + T * 10 + K, B, T, K, n, m, masked);
  const vec &mask = sw.mask;
  const size_t items = (size_t)B * T, pitems = (size_t)B * (T > 1 ? T - 1 : 1);
  const size_t G = (size_t)K * (1 + n * n + n * x + x * x) + (size_t)K * K + 2 * n + n * n + 4 + 1 + n + n * n;
  if (kvae_lgssm_switching_em_ws_floats(B, K, n, m) != (int64_t)(B * G)) return 30;
  if (kvae_lgssm_switching_em_ws_floats(B, 0, n, m) != 0) return 31;
  vec ll(items, NAN), seq(B, NAN);
  vec hmu(items * K * n, NAN), hS(items * K * n * n, NAN), hW(items * K * K, NAN), hw((size_t)B * K, NAN);
  vec rs(items * K, NAN), rp(pitems * K * K, NAN), ms(items * n, NAN), Ss(items * n * n, NAN);
  vec ws(B * G, NAN), N(K, NAN), S11((size_t)K * n * n, NAN), S10((size_t)K * n * x, NAN), S00((size_t)K * x * x, NAN), cnt((size_t)K * K, NAN),
      Syz(2 * n, NAN), Szz((size_t)n * n, NAN), Syy(4, NAN), Nobs(1, NAN), z0(n, NAN), z0z0((size_t)n * n, NAN), nseq(1, NAN);
  kvae_sws_problem S{};
  kvae_swf_problem &P = S.filt;
  sw.bind(P);
  P.ll =ll.data(), P.seq_ll = seq.data();
  S.hist_mu = hmu.data(), S.hist_Sigma = hS.data(), S.hist_W = hW.data(), S.hist_w = hw.data();
  S.regime_smooth = rs.data(), S.regime_pairs = rp.data(), S.mus_smooth = ms.data(), S.Sigmas_smooth = Ss.data();
  kvae_em_stats E{};
  E.ws = ws.data(), E.N = N.data(), E.S11 = S11.data(), E.S10 = S10.data(), E.S00 = S00.data(), E.counts = cnt.data(), E.Syz = Syz.data();
  E.Szz = Szz.data(), E.Syy = Syy.data(), E.Nobs = Nobs.data(), E.z0 = z0.data(), E.z0z0 = z0z0.data(), E.nseq = nseq.data();
  const std::vector<const vec *> all = {&ll, &seq, &hmu, &hS, &hW, &hw, &rs, &rp, &ms, &Ss, &ws, &N, &S11, &S10, &S00, &cnt, &Syz, &Szz, &Syy,
                                        &Nobs, &z0, &z0z0, &nseq};
  // ---- the error codes first: nothing launched, not an element of any buffer written ----
  int c0[4];
  counters(c0);
  {
    kvae_sws_problem Se = S;
    kvae_em_stats Ee = E;
    Se.filt.K = 9;
    if (kvae_lgssm_switching_em(&Se, &E, nullptr) != KVAE_ERR_ARG) return 1;
    Se = S, Se.filt.A = nullptr;
    if (kvae_lgssm_switching_em(&Se, &E, nullptr) != KVAE_ERR_NULL) return 2;
    Se = S, Se.hist_W = nullptr;
    if (kvae_lgssm_switching_em(&Se, &E, nullptr) != KVAE_ERR_NULL) return 3;
    Se = S, Se.filt.T = 0;
    if (kvae_lgssm_switching_em(&Se, &E, nullptr) != KVAE_ERR_DIMS) return 4;
    Se = S, Se.filt.state_log_w = hw.data(), Se.filt.state_mu = hmu.data(), Se.filt.state_Sigma = hS.data();
    if (kvae_lgssm_switching_em(&Se, &E, nullptr) != KVAE_ERR_ARG) return 5;   // a carried state
    if (kvae_lgssm_switching_em(nullptr, &E, nullptr) != KVAE_ERR_NULL || kvae_lgssm_switching_em(&S, nullptr, nullptr) != KVAE_ERR_NULL) return 6;
    Ee.ws = nullptr;
    if (kvae_lgssm_switching_em(&S, &Ee, nullptr) != KVAE_ERR_NULL) return 7;
    Se = S, Se.filt.ll = nullptr;
    if (kvae_lgssm_switching_em(&Se, &E, nullptr) != KVAE_ERR_NULL) return 8;   // seq_ll reads ll
    for (const vec *v : all)
      if (!nan_all(*v)) return 9;
    if (!launched(c0, 0, 0, 0, 0)) return 9;
  }
  // ---- the full call: one forward, one backward, one reduction, the sequence sums; every element written ----
  if (kvae_lgssm_switching_em(&S, &E, nullptr)) return 10;
  if (!launched(c0, 1, 1, 1, 1)) return 11;
  for (const vec *v : all)
    if (v != &rp && !finite_all(*v)) return 12;
  if (T > 1 ? !finite_all(rp) : !nan_all(rp)) return 13;   // nothing written to regime_pairs at T = 1
  if (nseq[0] != (float)B) return 14;
  {
    float obs = 0.f;
    for (size_t it = 0; it < items; ++it) obs += masked ? (mask[it] != 0.f ? 1.f : 0.f) : 1.f;
    if (Nobs[0] != obs) return 15;
    float tot = 0.f;
    for (int k = 0; k < K; ++k) tot += N[k];
    if (fabsf(tot - (float)items) > 1e-3f * items) return 16;   // one unit of mass per transition
    if (T == 1)
      for (float c : cnt)
        if (c != 0.f) return 17;                               // counts: t >= 1 only
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c)
        if (Szz[(size_t)r * n + c] != Szz[(size_t)c * n + r] || z0z0[(size_t)r * n + c] != z0z0[(size_t)c * n + r]) return 18;
    for (int k = 0; k < K; ++k)
      for (int r = 0; r < x; ++r)
        for (int c = 0; c < x; ++c)
          if (S00[((size_t)k * x + r) * x + c] != S00[((size_t)k * x + c) * x + r]) return 19;
  }
  // the smoother outputs are the smoother's own bits
  {
    vec rs2(items * K, NAN), rp2(pitems * K * K, NAN), ms2(items * n, NAN), Ss2(items * n * n, NAN), ll2(items, NAN);
    kvae_sws_problem S2 = S;
    S2.filt.ll = ll2.data(), S2.filt.seq_ll = nullptr;
    S2.regime_smooth = rs2.data(), S2.regime_pairs = rp2.data(), S2.mus_smooth = ms2.data(), S2.Sigmas_smooth = Ss2.data();
    if (kvae_lgssm_switching_smoother(&S2, nullptr)) return 20;
    if (rs2 != rs || ms2 != ms || Ss2 != Ss || ll2 != ll) return 21;
    if (T > 1 && rp2 != rp) return 21;
  }
  if (T > 8) return 0;   // the long shape is there for the prefetch only
  // ---- NULL outputs in several combinations: the same bits, the launches they need ----
  {
    vec ws2(B * G, NAN), N2(K, NAN), S102((size_t)K * n * x, NAN), z02(n, NAN), rs2(items * K, NAN);
    kvae_sws_problem S2 = S;
    S2.filt.ll = nullptr, S2.filt.seq_ll = nullptr;
    S2.regime_smooth = nullptr, S2.regime_pairs = nullptr, S2.mus_smooth = nullptr, S2.Sigmas_smooth = nullptr;
    kvae_em_stats E2{};
    E2.ws = ws2.data(), E2.N = N2.data(), E2.S10 = S102.data(), E2.z0 = z02.data();
    int c1[4];
    counters(c1);
    if (kvae_lgssm_switching_em(&S2, &E2, nullptr)) return 22;
    if (!launched(c1, 1, 1, 1, 0)) return 23;
    if (ws2 != ws || N2 != N || S102 != S10 || z02 != z0) return 24;
    // the smoother outputs alone: no reduction (ws is still the backward's to write)
    kvae_em_stats E3{};
    E3.ws = ws2.data();
    S2.regime_smooth = rs2.data();
    counters(c1);
    if (kvae_lgssm_switching_em(&S2, &E3, nullptr)) return 25;
    if (!launched(c1, 1, 1, 0, 0) || rs2 != rs) return 26;
    // nothing asked for: nothing launched
    S2.regime_smooth = nullptr;
    counters(c1);
    if (kvae_lgssm_switching_em(&S2, &E3, nullptr)) return 27;
    if (!launched(c1, 0, 0, 0, 0)) return 28;
    // nseq alone
    vec ns2(1, NAN);
    E3.nseq = ns2.data();
    if (kvae_lgssm_switching_em(&S2, &E3, nullptr) || ns2[0] != (float)B) return 29;
  }
  return 0;
}

int main() {
  const Shape shapes[] = {{1, 1, 1, 4, 2}, {2, 1, 5, 4, 2}, {2, 2, 7, 4, 2}, {3, 4, 5, 3, 1}, {2, 5, 7, 4, 4}, {2, 3, 8, 2, 3}, {3, 2, 3, 1, 1},
                          {1, 66, 2, 4, 2}};
  return run_shapes(shapes, "EM-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.T, s.K, s.n, s.m, masked); });
}
