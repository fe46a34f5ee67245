// swv_asan_driver.cpp — TEST-ONLY: the sweep, backtrace and gather of kvae_lgssm_switching_viterbi (csrc/lgssm_swv.h) on emulated
// wavefronts (wave_emu.h), as a standalone program that tests/test_switching_viterbi.py builds with -fsanitize=address,undefined
// and runs as a child process, through the host simulation's entry point defined there.  Every buffer - the three workspaces
// included - is allocated at its exact size, so a read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.
// Shapes: T = 1, K = 5 / 7 / 8 (padding lanes and a full grid), run-time n and m below the padded 4, a mask, NULL outputs, a carried
// state (then without mu0 / Sigma0), T past the 64 steps one round of the backtrace holds.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_swv.h"
#include "switching_fixture.h"

struct Outs {
  std::vector<int32_t> path, bp, lv;
  std::vector<uint32_t> wbp;
  vec plj, sc, mf, Sf, oJ, omu, oS, wmu, wS;
  Outs(int B, int T, int K, int n)
      : path((size_t)B * T, -1), bp((size_t)B * T * K, -1), lv((size_t)B * T, -1), wbp((size_t)B * T, 0xffffffffu), plj(B, NAN),
        sc((size_t)B * T * K, NAN), mf((size_t)B * T * n, NAN), Sf((size_t)B * T * n * n, NAN), oJ((size_t)B * K, NAN), omu((size_t)B * K * n, NAN),
        oS((size_t)B * K * n * n, NAN), wmu((size_t)B * T * K * n, NAN), wS((size_t)B * T * K * n * n, NAN) {}
  void bind(kvae_swv_problem &V) {
    V.path = path.data(), V.path_log_joint = plj.data(), V.scores = sc.data(), V.backptr = bp.data(), V.mus_filt = mf.data();
    V.Sigmas_filt = Sf.data(), V.levels = lv.data(), V.out_score = oJ.data(), V.out_mu = omu.data(), V.out_Sigma = oS.data();
    V.ws_bp = wbp.data(), V.ws_mu = wmu.data(), V.ws_Sigma = wS.data();
  }
  bool written(int K) const {
    for (const vec *v : {&plj, &sc, &mf, &Sf, &oJ, &omu, &oS})
      if (!finite_all(*v)) return false;
    for (int32_t s : path)
      if (s < 0 || s >= K) return false;
    for (int32_t s : bp)
      if (s < 0 || s >= K) return false;
    for (int32_t l : lv)
      if (l != 0) return false;
    return true;
  }
};

static int run(int B, int T, int K, int n, int m, bool masked) {
  const int p = 2;
  SwitchingModel sw(B * 1000 + T * 10 + K, B, T, K, n, m, masked);
  Outs all(B, T, K, n);
  kvae_swv_problem V{};
  sw.bind(V);
  all.bind(V);
  const int before = kvae_wemu_switching_viterbi_launches(0);
  if (kvae_lgssm_switching_viterbi(&V, nullptr)) return 1;
  if (kvae_wemu_switching_viterbi_launches(0) != before + 1) return 2;
  if (!all.written(K)) return 3;   // every output element written, every regime inside [0, K)
  for (int b = 0; b < B; ++b) {
    // the path follows the back-pointers from the lowest arg max of the last scores, whose maximum is path_log_joint; the beliefs
    // along it are the workspace's rows of (t, path_t)
    int st = 0;
    for (int j = 1; j < K; ++j)
      if (all.sc[((size_t)b * T + T - 1) * K + j] > all.sc[((size_t)b * T + T - 1) * K + st]) st = j;
    if (all.plj[b] != all.sc[((size_t)b * T + T - 1) * K + st]) return 4;
    for (int t = T - 1; t >= 0; --t) {
      const size_t q = (size_t)b * T + t;
      if (all.path[q] != st) return 5;
      for (int c = 0; c < n; ++c)
        if (all.mf[q * n + c] != all.wmu[(q * K + st) * n + c]) return 6;
      for (int c = 0; c < n * n; ++c)
        if (all.Sf[q * n * n + c] != all.wS[(q * K + st) * n * n + c]) return 7;
      if (((all.wbp[q] >> (4 * st)) & 15u) != (uint32_t)all.bp[q * K + st]) return 8;
      st = all.bp[q * K + st];
    }
    for (int j = 0; j < K; ++j)
      if (all.oJ[(size_t)b * K + j] != all.sc[((size_t)b * T + T - 1) * K + j]) return 9;
  }
  if (T > 8) return 0;   // the long shape is there for the prefetch and the second round of the backtrace only
  // a subset of the outputs, without the workspaces nobody reads: the same bits
  Outs some(B, T, K, n);
  kvae_swv_problem V2 = V;
  some.bind(V2);
  V2.mus_filt = nullptr, V2.Sigmas_filt = nullptr, V2.ws_mu = nullptr, V2.ws_Sigma = nullptr, V2.scores = nullptr, V2.levels = nullptr;
  V2.out_score = nullptr, V2.out_mu = nullptr, V2.out_Sigma = nullptr;
  if (kvae_lgssm_switching_viterbi(&V2, nullptr)) return 10;
  if (some.path != all.path || some.bp != all.bp) return 11;
  for (int b = 0; b < B; ++b)
    if (some.plj[b] != all.plj[b]) return 12;
  if (!nan_all(some.mf) || !nan_all(some.Sf) || !nan_all(some.sc) || !nan_all(some.wmu) || !nan_all(some.wS) || !nan_all(some.oJ)) return 13;
  V2 = V, some.bind(V2);
  V2.path = nullptr, V2.mus_filt = nullptr, V2.Sigmas_filt = nullptr, V2.ws_bp = nullptr, V2.ws_mu = nullptr, V2.ws_Sigma = nullptr;
  if (kvae_lgssm_switching_viterbi(&V2, nullptr)) return 14;
  if (some.sc != all.sc || some.oS != all.oS) return 15;
  // the second half from the carried state of the first (without mu0 / Sigma0): scores, back-pointers and state are the bits of the whole
  if (T >= 2) {
    const int T1 = T / 2, T2 = T - T1;
    vec y1 = chunk(sw.y, T, p, 0, T1), u1 = chunk(sw.u, T, m, 0, T1), k1 = chunk(sw.mask, T, 1, 0, T1), y2 = chunk(sw.y, T, p, T1, T),
        u2 = chunk(sw.u, T, m, T1, T), k2 = chunk(sw.mask, T, 1, T1, T);
    Outs a(B, T1, K, n), r(B, T2, K, n);
    kvae_swv_problem Va = V;
    a.bind(Va);
    Va.T = T1, Va.y = y1.data(), Va.u = u1.data(), Va.mask = masked ? k1.data() : nullptr;
    if (kvae_lgssm_switching_viterbi(&Va, nullptr)) return 16;
    kvae_swv_problem Vb = V;
    r.bind(Vb);
    Vb.T = T2, Vb.mu0 = nullptr, Vb.Sigma0 = nullptr, Vb.y = y2.data(), Vb.u = u2.data(), Vb.mask = masked ? k2.data() : nullptr;
    Vb.state_score = a.oJ.data(), Vb.state_mu = a.omu.data(), Vb.state_Sigma = a.oS.data();
    if (kvae_lgssm_switching_viterbi(&Vb, nullptr)) return 17;
    if (!r.written(K)) return 18;
    for (int b = 0; b < B; ++b)
      for (int t = 0; t < T2; ++t)
        for (int j = 0; j < K; ++j) {
          const size_t qa = ((size_t)b * T + T1 + t) * K + j, qr = ((size_t)b * T2 + t) * K + j;
          if (all.sc[qa] != r.sc[qr] || all.bp[qa] != r.bp[qr]) return 19;
        }
    if (r.oJ != all.oJ || r.omu != all.omu || r.oS != all.oS || r.plj != all.plj) return 20;
  }
  // error paths write nothing
  Outs none(B, T, K, n);
  kvae_swv_problem Ve = V;
  none.bind(Ve);
  Ve.K = 9;
  if (kvae_lgssm_switching_viterbi(&Ve, nullptr) != KVAE_ERR_ARG) return 21;
  Ve.K = K, Ve.A = nullptr;
  if (kvae_lgssm_switching_viterbi(&Ve, nullptr) != KVAE_ERR_NULL) return 22;
  Ve.A = V.A, Ve.ws_bp = nullptr;
  if (kvae_lgssm_switching_viterbi(&Ve, nullptr) != KVAE_ERR_NULL) return 23;
  Ve.ws_bp = V.ws_bp, Ve.T = 0;
  if (kvae_lgssm_switching_viterbi(&Ve, nullptr) != KVAE_ERR_DIMS) return 24;
  Ve.T = T, Ve.state_mu = all.omu.data();
  if (kvae_lgssm_switching_viterbi(&Ve, nullptr) != KVAE_ERR_ARG) return 25;
  if (!nan_all(none.sc) || !nan_all(none.plj) || !nan_all(none.mf) || !nan_all(none.wmu)) return 26;
  return 0;
}

int main() {
  // B, T, K, n, m
  const Shape shapes[] = {{1, 1, 1, 4, 2}, {2, 1, 5, 4, 2}, {3, 4, 5, 3, 1}, {2, 5, 7, 4, 4}, {2, 3, 8, 2, 3}, {3, 2, 3, 1, 1}, {2, 6, 8, 4, 2}, {1, 66, 2, 4, 2}};
  return run_shapes(shapes, "SWV-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.T, s.K, s.n, s.m, masked); });
}
