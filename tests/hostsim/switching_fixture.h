// switching_fixture.h — TEST-ONLY: what the sanitizer drivers of the switching read-outs share ({swf,sws,swm,swh,em,spf}_asan_driver.cpp):
// the model they run on, the checks that a buffer was written / left alone, the split of a sequence into two chunks, and main's
// loop over shapes x {observed, masked}.  Each driver keeps its own run(), its shape list and its token.
#pragma once

#include <math.h>
#include <stdio.h>

#include <random>
#include <vector>

typedef std::vector<float> vec;

static inline bool finite_all(const vec &v) {
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return true;
}
static inline bool nan_all(const vec &v) {
  for (float x : v)
    if (!std::isnan(x)) return false;
  return true;
}

// K regimes of a diagonal-plus-superdiagonal A_k and a diagonal Q_k, each of its own size; Sigma0 = 0.5 I; a sticky P (0.8 on the
// diagonal); R = 0.05 I; every third step hidden when masked.  Bm, C, mu0, y and the controls of the T + H steps are drawn in this
// order from mt19937(seed) through ONE normal distribution (it keeps half of every pair it draws): draw() continues the stream for
// the vectors a driver adds.  u holds the first T steps of u_all.
struct SwitchingModel {
  int B, T, K, n, m;
  std::mt19937 g;
  std::normal_distribution<float> nd{0.f, 1.f};
  vec A, Bm, Q, C, R{0.05f, 0.f, 0.f, 0.05f}, Pm, mu0, Sigma0, y, u_all, u, mask;

  SwitchingModel(unsigned seed, int B_, int T_, int K_, int n_, int m_, bool masked, int H = 0)
      : B(B_), T(T_), K(K_), n(n_), m(m_), g(seed), A((size_t)K * n * n, 0.f), Bm((size_t)K * n * m), Q((size_t)K * n * n, 0.f),
        C((size_t)2 * n), Pm((size_t)K * K), mu0(n), Sigma0((size_t)n * n, 0.f), y((size_t)B * T * 2), u_all((size_t)B * (T + H) * m),
        u((size_t)B * T * m), mask(masked ? (size_t)B * T : 0) {
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < n; ++i) {
        A[((size_t)k * n + i) * n + i] = 0.9f - 0.05f * k;
        if (i + 1 < n) A[((size_t)k * n + i) * n + i + 1] = 0.1f * (k % 2 ? 1.f : -1.f);
        Q[((size_t)k * n + i) * n + i] = 0.02f + 0.01f * k;
      }
    for (int i = 0; i < n; ++i) Sigma0[(size_t)i * n + i] = 0.5f;
    for (vec *v : {&Bm, &C, &mu0, &y, &u_all}) draw(*v);
    for (int b = 0; b < B; ++b)
      for (int e = 0; e < T * m; ++e) u[(size_t)b * T * m + e] = u_all[(size_t)b * (T + H) * m + e];
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j) Pm[(size_t)i * K + j] = K == 1 ? 1.f : (i == j ? 0.8f : 0.2f / (K - 1));
    for (size_t it = 0; it < mask.size(); ++it) mask[it] = it % 3 == 1 ? 0.f : 1.f;
  }
  void draw(vec &v) {
    for (float &x : v) x = 0.5f * nd(g);
  }
  // the dimensions and the eleven operand pointers that kvae_swf_problem and kvae_spf_problem share
  template <class Problem>
  void bind(Problem &P) {
    P.B = B, P.T = T, P.K = K, P.n = n, P.m = m, P.p = 2;
    P.A = A.data(), P.Bm = Bm.data(), P.Q = Q.data(), P.C = C.data(), P.R = R.data(), P.P = Pm.data(), P.mu0 = mu0.data();
    P.Sigma0 = Sigma0.data(), P.y = y.data(), P.u = u.data(), P.mask = mask.empty() ? nullptr : mask.data();
  }
};

// the steps [t0, t1) of every row of a per-step array [rows, T, c], allocated at its exact size (an empty array stays empty: no mask)
static inline vec chunk(const vec &v, int T, int c, int t0, int t1) {
  const size_t rows = v.size() / ((size_t)T * c), len = (size_t)(t1 - t0) * c;
  vec out(rows * len);
  for (size_t r = 0; r < rows; ++r)
    for (size_t e = 0; e < len; ++e) out[r * len + e] = v[(r * T + t0) * c + e];
  return out;
}

struct Shape {
  int B, T, K, n, m, H = 0, G = 0, N = 0;   // H: the forecast's horizon; G, N, thr: the particle filter's replicates, particles, threshold
  float thr = 0.f;
};

// main(): run(shape, masked) over every shape, observed and masked (the long one, T > 8, masked only); the token when all returned 0
template <size_t S, class Run>
static int run_shapes(const Shape (&shapes)[S], const char *token, Run run) {
  int bad = 0;
  for (const Shape &s : shapes)
    for (int masked = s.T > 8 ? 1 : 0; masked < 2; ++masked) {
      const int rc = run(s, masked == 1);
      printf("(%d,%d,%d,%d,%d; H %d, G %d, N %d, thr %g) %s %d\n", s.B, s.T, s.K, s.n, s.m, s.H, s.G, s.N, s.thr, masked ? "masked" : "observed", rc);
      bad += rc != 0;
    }
  if (bad) return 1;
  printf("%s\n", token);
  return 0;
}
