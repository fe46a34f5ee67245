// swm_asan_driver.cpp — TEST-ONLY: the forward (csrc/lgssm_swf.h, history kept) and the adjoint (csrc/lgssm_swm.h) of
// kvae_lgssm_switching_marginal / kvae_lgssm_switching_marginal_bwd on emulated wavefronts (wave_emu.h), as a standalone program
// that tests/test_switching_marginal.py builds with -fsanitize=address,undefined and runs as a child process, through the host
// simulation's entry points defined there.  Every buffer is allocated at its exact size, so a read or write past the layouts of
// include/kvae_lgssm.h is a sanitizer report.  Shapes: T = 1 and T = 2, K = 5 and K = 7 (padding lanes), a full grid of 8, run-time
// n = 3 and m = 1, a mask, NULL outputs in several combinations, either upstream alone, T = 66, the error codes.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include "../../kalman-vae_amd/csrc/lgssm_swm.h"
#include "switching_fixture.h"

static int run(int B, int T, int K, int n, int m, bool masked) {
  const int p = 2;
  SwitchingModel sw(B * 1000 + T * 10 + K, B, T, K, n, m, masked);
  const vec &mask = sw.mask;
  const size_t items = (size_t)B * T;
  std::vector<float> gll(items), gseq(B);   // the upstreams: drawn after the model, from its stream
  sw.draw(gll), sw.draw(gseq);
  const size_t G = (size_t)K * (2 * n * n + n * m) + 2 * n + (size_t)K * K + n + (size_t)n * n;
  if (kvae_lgssm_switching_marginal_ws_floats(B, K, n, m) != (int64_t)(B * G)) return 30;
  std::vector<float> ll(items, NAN), seq(B, NAN), hlw(items * K, NAN), hmu(items * K * n, NAN), hS(items * K * n * n, NAN);
  std::vector<float> ws(B * G, NAN), gA((size_t)K * n * n, NAN), gB((size_t)K * n * m, NAN), gQ((size_t)K * n * n, NAN), gC((size_t)p * n, NAN),
      gP((size_t)K * K, NAN), gm(n, NAN), gS((size_t)n * n, NAN), gY(items * p, NAN), gU(items * m, NAN), llr(items, NAN);
  kvae_swm_problem M{};
  kvae_swf_problem &P = M.filt;
  sw.bind(P);
  P.ll =ll.data(), P.seq_ll = seq.data();
  M.hist_lw = hlw.data(), M.hist_mu = hmu.data(), M.hist_Sigma = hS.data();
  kvae_swm_grads Gr{};
  Gr.g_ll = gll.data(), Gr.g_seq = gseq.data(), Gr.ws = ws.data();
  Gr.gA = gA.data(), Gr.gB = gB.data(), Gr.gQ = gQ.data(), Gr.gC = gC.data(), Gr.g_logP = gP.data(), Gr.g_mu0 = gm.data();
  Gr.g_Sigma0 = gS.data(), Gr.gY = gY.data(), Gr.gU = gU.data(), Gr.ll_recomputed = llr.data();
  // error paths first: nothing may be written
  {
    kvae_swm_problem E = M;
    E.filt.K = 9;
    if (kvae_lgssm_switching_marginal(&E, nullptr) != KVAE_ERR_ARG || kvae_lgssm_switching_marginal_bwd(&E, &Gr, nullptr) != KVAE_ERR_ARG) return 1;
    E = M, E.filt.A = nullptr;
    if (kvae_lgssm_switching_marginal(&E, nullptr) != KVAE_ERR_NULL || kvae_lgssm_switching_marginal_bwd(&E, &Gr, nullptr) != KVAE_ERR_NULL) return 2;
    E = M, E.hist_lw = nullptr;
    if (kvae_lgssm_switching_marginal(&E, nullptr) != KVAE_ERR_NULL || kvae_lgssm_switching_marginal_bwd(&E, &Gr, nullptr) != KVAE_ERR_NULL) return 3;
    E = M, E.filt.T = 0;
    if (kvae_lgssm_switching_marginal(&E, nullptr) != KVAE_ERR_DIMS) return 4;
    E = M, E.filt.state_log_w = hlw.data(), E.filt.state_mu = hmu.data(), E.filt.state_Sigma = hS.data();
    if (kvae_lgssm_switching_marginal(&E, nullptr) != KVAE_ERR_ARG || kvae_lgssm_switching_marginal_bwd(&E, &Gr, nullptr) != KVAE_ERR_ARG) return 5;
    if (kvae_lgssm_switching_marginal(nullptr, nullptr) != KVAE_ERR_NULL || kvae_lgssm_switching_marginal_bwd(&M, nullptr, nullptr) != KVAE_ERR_NULL) return 6;
    kvae_swm_grads Ge = Gr;
    Ge.g_ll = nullptr, Ge.g_seq = nullptr;
    if (kvae_lgssm_switching_marginal_bwd(&M, &Ge, nullptr) != KVAE_ERR_NULL) return 7;
    Ge = Gr, Ge.ws = nullptr;
    if (kvae_lgssm_switching_marginal_bwd(&M, &Ge, nullptr) != KVAE_ERR_NULL) return 8;
    for (const auto *v : {&ll, &seq, &hlw, &hmu, &hS, &ws, &gA, &gB, &gQ, &gC, &gP, &gm, &gS, &gY, &gU, &llr})
      if (!nan_all(*v)) return 9;
  }
  const int b0 = kvae_wemu_switching_marginal_launches(0), b2 = kvae_wemu_switching_marginal_launches(2), b3 = kvae_wemu_switching_marginal_launches(3);
  if (kvae_lgssm_switching_marginal(&M, nullptr)) return 10;
  if (kvae_lgssm_switching_marginal_bwd(&M, &Gr, nullptr)) return 11;
  if (kvae_wemu_switching_marginal_launches(0) != b0 + 1 || kvae_wemu_switching_marginal_launches(2) != b2 + 1 ||
      kvae_wemu_switching_marginal_launches(3) != b3 + 1)
    return 12;
  for (const auto *v : {&ll, &seq, &hmu, &hS, &ws, &gA, &gB, &gQ, &gC, &gP, &gm, &gS, &gY, &gU})
    if (!finite_all(*v)) return 13;   // every element written
  for (float x : hlw)
    if (std::isnan(x)) return 13;
  if (llr != ll) return 26;   // the adjoint's recomputed pair steps give the forward's bits
  // the forward's values are the filter's own bits
  {
    std::vector<float> ll2(items, NAN);
    kvae_swf_problem F = P;
    F.ll = ll2.data(), F.seq_ll = nullptr;
    if (kvae_lgssm_switching_filter(&F, nullptr)) return 14;
    if (ll2 != ll) return 15;
  }
  if (masked)
    for (size_t it = 0; it < items; ++it)
      if (mask[it] == 0.f && (gY[it * 2] != 0.f || gY[it * 2 + 1] != 0.f)) return 16;
  if (T > 8) return 0;   // the long shape is there for the prefetch only
  // subsets of the outputs and of the upstreams: the same bits where the upstreams are the same
  {
    std::vector<float> ws2(B * G, NAN), gA2((size_t)K * n * n, NAN), gY2(items * p, NAN), gU2(items * m, NAN), gS2((size_t)n * n, NAN);
    kvae_swm_grads G2{};
    G2.g_ll = gll.data(), G2.g_seq = gseq.data(), G2.ws = ws2.data(), G2.gA = gA2.data(), G2.g_Sigma0 = gS2.data();
    if (kvae_lgssm_switching_marginal_bwd(&M, &G2, nullptr)) return 17;
    if (gA2 != gA || gS2 != gS || ws2 != ws) return 18;
    const int r3 = kvae_wemu_switching_marginal_launches(3);
    kvae_swm_grads G3{};
    G3.g_ll = gll.data(), G3.g_seq = gseq.data(), G3.ws = ws2.data(), G3.gY = gY2.data(), G3.gU = gU2.data();
    if (kvae_lgssm_switching_marginal_bwd(&M, &G3, nullptr)) return 19;
    if (gY2 != gY || gU2 != gU || kvae_wemu_switching_marginal_launches(3) != r3) return 20;   // no reduction for gY / gU alone
    const int r2 = kvae_wemu_switching_marginal_launches(2);
    kvae_swm_grads G4{};
    G4.g_ll = gll.data(), G4.ws = ws2.data();
    if (kvae_lgssm_switching_marginal_bwd(&M, &G4, nullptr)) return 21;
    if (kvae_wemu_switching_marginal_launches(2) != r2) return 22;                             // no output: no launch
    G4.gC = gC.data(), G4.g_logP = gP.data();
    if (kvae_lgssm_switching_marginal_bwd(&M, &G4, nullptr)) return 23;                        // g_ll alone
    G4.g_ll = nullptr, G4.g_seq = gseq.data(), G4.g_mu0 = gm.data();
    if (kvae_lgssm_switching_marginal_bwd(&M, &G4, nullptr)) return 24;                        // g_seq alone
    if (!finite_all(gC) || !finite_all(gP) || !finite_all(gm)) return 25;
  }
  return 0;
}

int main() {
  const Shape shapes[] = {{1, 1, 1, 4, 2}, {2, 1, 5, 4, 2}, {2, 2, 7, 4, 2}, {3, 4, 5, 3, 1}, {2, 5, 7, 4, 4}, {2, 3, 8, 2, 3}, {3, 2, 3, 1, 1},
                          {1, 66, 2, 4, 2}};
  return run_shapes(shapes, "SWM-ASAN-OK", [](const Shape &s, bool masked) { return run(s.B, s.T, s.K, s.n, s.m, masked); });
}
