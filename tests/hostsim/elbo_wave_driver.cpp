// elbo_wave_driver.cpp — TEST-ONLY: the 64-LANE form of the ELBO bodies (csrc/lgssm_elbo.h: elbo_probe_body, elbo_body) on emulated
// wavefronts, as a standalone program that tests/test_elbo_steps.py builds twice - with -fsanitize=address,undefined and with
// -fsanitize=thread - and runs as a child process.  The host simulation (hostsim.cpp) and the thread-per-step kernels run these
// bodies with KV_PAR as a serial loop; the form the wave-per-step kernels k_elbo_probe<D> / k_elbo<D> run - lanes striding KV_PAR,
// KV_LANE0 sections, KV_SYNC() between phases - is built here: lgssm_elbo.h WITHOUT KVAE_HOSTSIM and without KV_TPP over the stub
// <hip/hip_runtime.h> (wave_emu.h), so KV_LANE is the emulated lane, KV_SYNC() the emulator's rendezvous and ElboLds<D> one heap
// object per emulated wavefront, NaN-filled and of exact size.  The lanes are host threads and the rendezvous is a mutex and a
// condition variable, so under ThreadSanitizer an LDS element written in one phase and read in the same phase by another lane -
// a missing KV_SYNC(), a side effect outside KV_LANE0: the phase rules at the top of lgssm_vm.h - is a reported data race.
// Every output is compared bit for bit with the serial host build of the same bodies (the same fmaf chains), which this file
// also holds: it is compiled a second time with -DELBO_DRIVER_SERIAL into an object of its own (KVAE_HOSTSIM is a compile-time
// property of the bodies).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

struct ElboRun;   // the problem and its buffers, below
extern "C" void elbo_driver_serial(int dims, const ElboRun *r);

#if defined(ELBO_DRIVER_SERIAL)
#define KVAE_HOSTSIM 1
#include <memory>
#else
#define kvae kvae_wave   // (its own namespace, as kvae_lgssm_tpp.hip renames it: the execution model is a property of the bodies)
#include "wave_emu.h"
// what lgssm_elbo.h uses of HIP beyond the emulator's vocabulary (only lane 0 of a wavefront records a level, and the emulated
// wavefronts of a launch run one after the other; a real atomic all the same)
static inline int32_t atomicMax(int32_t *p, int32_t v) {
  int32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return cur;
}
#endif
#include "../../kalman-vae_amd/csrc/lgssm_elbo.h"

using namespace kvae;

struct ElboRun {
  kvae_lgssm_problem P;
  const float *mus, *Sigs, *eps;
  float *terms, *ws, *g_mus, *g_Sigs;   // ws, g_mus / g_Sigs may be NULL
  int32_t *levels;
  const kvae_lgssm_input_grads *G;      // NULL without gradients
};

#if defined(ELBO_DRIVER_SERIAL)
template <class D>
static void serial(const ElboRun &r) {   // run_elbo of hostsim.cpp
  auto L = std::make_unique<ElboLds<D>>();
  const kvae_lgssm_problem &P = r.P;
  const D d(P.n, P.m, P.p);
  r.levels[0] = r.levels[1] = 0;
  for (int b = 0; b < P.B; ++b)
    for (int t = 0; t < P.T; ++t) {
      memset(L.get(), 0xFF, sizeof(*L));
      elbo_probe_body(d, P, r.Sigs, r.mus, r.eps, r.ws, r.levels, b, t, *L);
    }
  for (int b = 0; b < P.B; ++b)
    for (int t = 0; t < P.T; ++t) {
      memset(L.get(), 0xFF, sizeof(*L));
      elbo_body(d, P, r.mus, r.Sigs, r.eps, r.terms, r.levels, r.ws, r.g_mus, r.g_Sigs, r.G, b, t, *L);
    }
}
extern "C" void elbo_driver_serial(int dims, const ElboRun *r) {
  if (dims == 0) serial<SDims<4, 4, 2>>(*r);
  else if (dims == 1) serial<SDims<16, 16, 2>>(*r);
  else serial<RDims>(*r);
}
#else
#include <cmath>
#include <random>
#include <vector>

// one emulated wavefront per (b,t), as k_elbo_probe<D> / k_elbo<D> launch them (grid = B T, 64 threads)
template <class D>
static void wave(const ElboRun &r) {
  const kvae_lgssm_problem &P = r.P;
  const D d(P.n, P.m, P.p);
  r.levels[0] = r.levels[1] = 0;
  const unsigned grid = (unsigned)(P.B * P.T);
  wemu::launch_wg({grid, 1, 1}, 64, 0, [&] {
    ElboLds<D> &L = *static_cast<ElboLds<D> *>(wemu::block_shared(0, sizeof(ElboLds<D>)));
    const int b = (int)blockIdx.x / P.T, t = (int)blockIdx.x - b * P.T;
    elbo_probe_body(d, P, r.Sigs, r.mus, r.eps, r.ws, r.levels, b, t, L);
  });
  wemu::launch_wg({grid, 1, 1}, 64, 0, [&] {
    ElboLds<D> &L = *static_cast<ElboLds<D> *>(wemu::block_shared(0, sizeof(ElboLds<D>)));
    const int b = (int)blockIdx.x / P.T, t = (int)blockIdx.x - b * P.T;
    elbo_body(d, P, r.mus, r.Sigs, r.eps, r.terms, r.levels, r.ws, r.g_mus, r.g_Sigs, r.G, b, t, L);
  });
}

struct Variant {
  bool grads, ws;
  int lvS, lvQ;   // 0, 2 or 5: the ONE poisoned Sigma_s / Q
  bool q_shared, masked;
};
static const Variant kVariants[8] = {{true, true, 0, 0, false, false}, {true, false, 2, 0, true, true},  {false, true, 5, 5, false, true},
                                     {true, true, 5, 5, true, false},  {false, false, 0, 0, true, true}, {true, false, 5, 5, false, true},
                                     {true, true, 2, 0, false, true},  {false, true, 2, 0, true, false}};

// dense SPD: c I + s W W^T
static void spd(std::vector<float> &out, size_t at, int n, float c, float s, std::mt19937 &g) {
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> W((size_t)n * n);
  for (auto &x : W) x = nd(g);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      float acc = i == j ? c : 0.f;
      for (int k = 0; k < n; ++k) acc += s * W[(size_t)i * n + k] * W[(size_t)j * n + k];
      out[at + (size_t)i * n + j] = acc;
    }
}
static void poison(std::vector<float> &out, size_t at, int n, int idx, float good, float bad) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) out[at + (size_t)i * n + j] = i != j ? 0.f : (i == idx ? bad : good);
}

static int run(int dims, int n, int m, int p, int B, int T, const Variant &v) {
  std::mt19937 g(1000 * n + 100 * m + 10 * T + v.lvS + 3 * v.lvQ);
  std::normal_distribution<float> nd(0.f, 1.f);
  const size_t items = (size_t)B * T, nn = (size_t)n * n;
  std::vector<float> mus(items * n), eps(items * n), Sig(items * nn), Y(items * p), U(items * m), A(items * nn), Bm(items * n * m),
      C(items * p * n), Q(v.q_shared ? nn : items * nn), R((size_t)p * p), mu0((size_t)B * n), S0((size_t)B * nn), mask(v.masked ? items : 0);
  for (auto *x : {&mus, &eps, &Y, &U, &Bm, &C, &mu0})
    for (auto &e : *x) e = 0.3f * nd(g);
  for (size_t q = 0; q < items; ++q) {
    spd(Sig, q * nn, n, 0.3f, 0.01f, g);
    if (!v.q_shared) spd(Q, q * nn, n, 0.02f, 0.0005f, g);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) A[q * nn + (size_t)i * n + j] = (i == j ? 0.9f : 0.f) + 0.08f * nd(g);
  }
  if (v.q_shared) spd(Q, 0, n, 0.02f, 0.0005f, g);
  spd(R, 0, p, 0.03f, 0.01f, g);
  for (int b = 0; b < B; ++b) spd(S0, b * nn, n, 0.5f, 0.04f, g);
  if (v.lvS) poison(Sig, (items - 1) * nn, n, 0, 0.2f, v.lvS == 2 ? -5e-5f : -1.0f);
  if (v.lvQ) poison(Q, v.q_shared ? 0 : (items - 1) * nn, n, n > 2 ? 2 : n - 1, 0.02f, -1.0f);
  for (size_t q = 0; q < mask.size(); ++q) mask[q] = q % 3 == 1 ? 0.f : 1.f;

  ElboRun r[2];
  std::vector<float> terms[2], ws[2], g_mus[2], g_Sig[2], gA[2], gB[2], gC[2], gQ[2], gY[2], gU[2];
  std::vector<int32_t> levels[2];
  kvae_lgssm_input_grads G[2];
  for (int k = 0; k < 2; ++k) {
    kvae_lgssm_problem &P = r[k].P;
    memset(&P, 0, sizeof(P));
    P.B = B, P.T = T, P.n = n, P.m = m, P.p = p;
    P.A = {A.data(), (int64_t)T * n * n, (int64_t)n * n};
    P.Bm = {Bm.data(), (int64_t)T * n * m, (int64_t)n * m};
    P.C = {C.data(), (int64_t)T * p * n, (int64_t)p * n};
    P.Q = {Q.data(), v.q_shared ? 0 : (int64_t)T * n * n, v.q_shared ? 0 : (int64_t)n * n};
    P.R = R.data(), P.mu0 = mu0.data(), P.mu0_sb = n, P.Sigma0 = S0.data(), P.Sigma0_sb = (int64_t)nn;
    P.Y = Y.data(), P.U = U.data(), P.mask = v.masked ? mask.data() : nullptr;
    terms[k].assign(items * 4, NAN), levels[k].assign(3, -1);
    if (v.ws) ws[k].assign(items * n, NAN);
    r[k].mus = mus.data(), r[k].Sigs = Sig.data(), r[k].eps = eps.data();
    r[k].terms = terms[k].data(), r[k].levels = levels[k].data(), r[k].ws = v.ws ? ws[k].data() : nullptr;
    r[k].g_mus = r[k].g_Sigs = nullptr, r[k].G = nullptr;
    if (v.grads) {
      g_mus[k].assign(items * n, NAN), g_Sig[k].assign(items * nn, NAN), gA[k].assign(items * nn, NAN), gB[k].assign(items * n * m, NAN);
      gC[k].assign(items * p * n, NAN), gQ[k].assign(items * nn, NAN), gY[k].assign(items * p, NAN), gU[k].assign(items * m, NAN);
      memset(&G[k], 0, sizeof(G[k]));
      G[k].gA = {gA[k].data(), (int64_t)T * n * n, (int64_t)n * n};
      G[k].gB = {gB[k].data(), (int64_t)T * n * m, (int64_t)n * m};
      G[k].gC = {gC[k].data(), (int64_t)T * p * n, (int64_t)p * n};
      G[k].gQ = {gQ[k].data(), (int64_t)T * n * n, (int64_t)n * n};
      G[k].gY = gY[k].data(), G[k].gU = gU[k].data();
      r[k].g_mus = g_mus[k].data(), r[k].g_Sigs = g_Sig[k].data(), r[k].G = &G[k];
    }
  }
  elbo_driver_serial(dims, &r[0]);
  if (dims == 0) wave<SDims<4, 4, 2>>(r[1]);
  else if (dims == 1) wave<SDims<16, 16, 2>>(r[1]);
  else wave<RDims>(r[1]);
  const int wantQ = T > 1 ? v.lvQ : 0;   // Q_0 is never factorised
  if (levels[0][0] != v.lvS || levels[0][1] != wantQ) return 1;
  if (levels[1][0] != levels[0][0] || levels[1][1] != levels[0][1]) return 2;
  for (float x : terms[1])
    if (!std::isfinite(x)) return 3;   // every (b,t) written
  int rc = 10;
  for (auto *pair : {terms, ws, g_mus, g_Sig, gA, gB, gC, gQ, gY, gU}) {
    if (pair[0].size() != pair[1].size() || (pair[0].size() && memcmp(pair[0].data(), pair[1].data(), pair[0].size() * sizeof(float)) != 0))
      return rc;   // 10 terms, 11 ws, 12 g_mus, 13 g_Sigmas, 14 gA, 15 gB, 16 gC, 17 gQ, 18 gY, 19 gU: not the bits of the serial form
    ++rc;
  }
  return 0;
}

int main() {
  const int shapes[4][4] = {{0, 4, 4, 2}, {1, 16, 16, 2}, {2, 5, 3, 2}, {2, 16, 16, 16}};
  int bad = 0;
  for (int di = 0; di < 4; ++di)
    for (int T = 1; T <= 3; ++T)
      for (int k = 0; k < 3; ++k) {   // nine runs per shape: each of the eight variants at least once
        const int vi = (di + T + 3 * k) % 8;
        const Variant &v = kVariants[vi];
        const int *s = shapes[di];
        const int rc = run(s[0], s[1], s[2], s[3], 2, T, v);
        printf("(%d,%d,%d) B=2 T=%d grads=%d ws=%d levels=(%d,%d) q_shared=%d mask=%d: %d\n", s[1], s[2], s[3], T, v.grads, v.ws, v.lvS, v.lvQ,
               v.q_shared, v.masked, rc);
        bad += rc != 0;
      }
  if (bad) return 1;
  printf("ELBO-WAVE-OK\n");
  return 0;
}
#endif
