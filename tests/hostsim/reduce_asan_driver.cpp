// reduce_asan_driver.cpp — TEST-ONLY: k_rnn_wgrad_partial<RT> / k_rnn_wgrad_final (csrc/rnn_wgrad.h), the streaming mixture kernels
// (csrc/mix_wave.h) and the linear heads (csrc/small_linear.h) on emulated workgroups (wave_emu.h, through the launch code of
// wave_emu_reduce.cpp), as a stand-alone program that tests/test_wave_emu_reduce.py builds with -fsanitize=address,undefined and
// runs as a child process.  Every input, output, workspace and partials buffer is a heap block of EXACTLY the size the layouts
// and the size functions state (a strided operand ends with its last row), so a read or write past one - a clamped load that is
// not clamped, a dead wavefront that stores, a workspace one problem short - is a sanitizer report; the results are compared with
// double-precision loops as well.  Shapes: the ragged and limit cases of the test file.
#include "wave_emu_reduce.cpp"

#include <random>
#include <vector>

typedef std::vector<float> vec;

static int g_notes[64];
extern "C" void kvae_wemu_rnn_note(int which) { g_notes[which] += 1; }

static std::mt19937 g_rng(12345);
static void fill(vec &v, float scale = 1.f) {
  std::normal_distribution<float> nd(0.f, 1.f);
  for (auto &e : v) e = scale * nd(g_rng);
}
static bool close(double got, double want, double scale) { return fabs(got - want) <= 2e-5 * scale + 1e-30 && std::isfinite(got); }

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
struct WgSpec { int Bsz, T, H, I, R, shift; };
struct WgBufs {
  vec d, h, x, g_wh, g_wx, g_b;
  int64_t hs;   // row stride of h: 2H with the operand in the upper half when shift > 0 (the reverse GRU direction's layout)
};
static int run_wgrad(const std::vector<WgSpec> &specs, int max_chunks, int fill_wgs) {
  const int n = (int)specs.size();
  std::vector<WgBufs> b(n);
  std::vector<kvae_wgrad_problem> probs(n);
  for (int i = 0; i < n; ++i) {
    const WgSpec &s = specs[i];
    const int64_t N = (int64_t)s.Bsz * s.T;
    WgBufs &w = b[i];
    w.hs = s.shift > 0 ? 2 * s.H : s.H;
    w.d.resize(N * s.R), w.h.resize(N * w.hs), w.x.resize(N * s.I);
    fill(w.d), fill(w.h), fill(w.x);
    w.g_wh.assign((size_t)s.R * s.H, NAN), w.g_wx.assign((size_t)s.R * s.I, NAN), w.g_b.assign(s.R, NAN);
    kvae_wgrad_problem &p = probs[i];
    p.d = w.d.data(), p.h = s.H ? w.h.data() + (s.shift > 0 ? s.H : 0) : nullptr, p.x = s.I ? w.x.data() : nullptr;
    p.g_wh = s.H ? w.g_wh.data() : nullptr, p.g_wx = s.I ? w.g_wx.data() : nullptr, p.g_b = w.g_b.data();
    p.d_stride = s.R, p.h_stride = w.hs, p.x_stride = s.I, p.N = N;
    p.R = s.R, p.H = s.H, p.I = s.I, p.bias = 1, p.T = s.T, p.shift = s.shift;
  }
  kvae_wemu_wgrad_max_chunks(max_chunks), kvae_wemu_wgrad_fill(fill_wgs);
  vec ws((size_t)kvae_wemu_wgrad_ws_floats(probs.data(), n), NAN);
  const int rc = kvae_wemu_wgrad(probs.data(), n, ws.data());
  kvae_wemu_wgrad_max_chunks(-1), kvae_wemu_wgrad_fill(-1);
  if (rc) return 1;
  for (int i = 0; i < n; ++i) {
    const WgSpec &s = specs[i];
    const kvae_wgrad_problem &p = probs[i];
    const int C = s.H + s.I + 1;
    for (int r = 0; r < s.R; ++r)
      for (int c = 0; c < C; ++c) {
        double want = 0.0, scale = 0.0;
        for (int64_t q = 0; q < p.N; ++q) {
          double xv = 1.0;
          if (c < s.H) {
            const int t = (int)(q % s.T) + s.shift;
            xv = (t >= 0 && t < s.T) ? p.h[(q + s.shift) * p.h_stride + c] : 0.0;
          } else if (c < s.H + s.I) {
            xv = p.x[q * p.x_stride + (c - s.H)];
          }
          want += (double)p.d[q * p.d_stride + r] * xv, scale += fabs((double)p.d[q * p.d_stride + r] * xv);
        }
        const float got = c < s.H ? b[i].g_wh[(size_t)r * s.H + c] : (c < s.H + s.I ? b[i].g_wx[(size_t)r * s.I + c - s.H] : b[i].g_b[r]);
        if (!close(got, want, scale)) return 2 + i;
      }
  }
  return 0;
}

// ---- mixture -----------------------------------------------------------------------------------------------------------------
static int run_mix(int64_t rows, int K, int E, int fcap, int bcap) {
  vec alpha(rows * K), base((size_t)K * E), up(rows * E), out(rows * E, NAN), g_alpha(rows * K), g_base((size_t)K * E, NAN);
  fill(alpha, 0.3f), fill(base), fill(up), fill(g_alpha);
  const vec g_alpha0 = g_alpha;
  const int64_t cap = (rows + 15) / 16;   // kvae_mix_bwd_partials
  vec partials((size_t)cap * K * E, NAN);
  kvae_wemu_mix_fwd_max_slabs(fcap), kvae_wemu_mix_bwd_max_slabs(bcap);
  const int ran_f = kvae_wemu_mix_fwd(alpha.data(), base.data(), out.data(), rows, K, E);
  const int ran_b = kvae_wemu_mix_bwd(alpha.data(), base.data(), up.data(), g_alpha.data(), g_base.data(), partials.data(), rows, K, E, 1, cap);
  kvae_wemu_mix_fwd_max_slabs(-1), kvae_wemu_mix_bwd_max_slabs(-1);
  if (!ran_f || !ran_b) return 1;
  for (int64_t r = 0; r < rows; ++r) {
    for (int e = 0; e < E; ++e) {
      double want = 0.0, scale = 0.0;
      for (int k = 0; k < K; ++k) want += (double)alpha[r * K + k] * base[(size_t)k * E + e], scale += fabs((double)alpha[r * K + k] * base[(size_t)k * E + e]);
      if (!close(out[r * E + e], want, scale)) return 2;
    }
    for (int k = 0; k < K; ++k) {
      double want = g_alpha0[r * K + k], scale = fabs(want);
      for (int e = 0; e < E; ++e) want += (double)up[r * E + e] * base[(size_t)k * E + e], scale += fabs((double)up[r * E + e] * base[(size_t)k * E + e]);
      if (!close(g_alpha[r * K + k], want, scale)) return 3;
    }
  }
  for (int k = 0; k < K; ++k)
    for (int e = 0; e < E; ++e) {
      double want = 0.0, scale = 0.0;
      for (int64_t r = 0; r < rows; ++r) want += (double)alpha[r * K + k] * up[r * E + e], scale += fabs((double)alpha[r * K + k] * up[r * E + e]);
      if (!close(g_base[(size_t)k * E + e], want, scale)) return 4;
    }
  return 0;
}

// ---- linear heads --------------------------------------------------------------------------------------------------------------
static int run_linear(int64_t N, int F, int O, bool softmax, int64_t xs, int min_blocks) {
  vec x((size_t)(N - 1) * xs + F), W((size_t)O * F), bias(O), y((size_t)N * O, NAN), g((size_t)N * O), gl((size_t)N * O, NAN), dx((size_t)N * F, NAN);
  fill(x), fill(W, 0.3f), fill(bias), fill(g);
  kvae_wemu_linear_min_blocks(min_blocks);
  kvae_wemu_linear_fwd(x.data(), xs, N, F, W.data(), bias.data(), O, softmax, y.data());
  kvae_wemu_linear_min_blocks(-1);
  kvae_wemu_linear_bwd_input(g.data(), softmax ? y.data() : nullptr, N, F, W.data(), O, softmax ? gl.data() : nullptr, dx.data(), F);
  for (int64_t n = 0; n < N; ++n) {
    std::vector<double> z(O), glw(O);
    double mx = -1e300, sum = 0.0, dot = 0.0, zs = 0.0;
    for (int o = 0; o < O; ++o) {
      z[o] = bias[o];
      for (int f = 0; f < F; ++f) z[o] += (double)x[n * xs + f] * W[(size_t)o * F + f];
      mx = z[o] > mx ? z[o] : mx, zs = fabs(z[o]) > zs ? fabs(z[o]) : zs;
    }
    if (softmax) {
      for (int o = 0; o < O; ++o) sum += (z[o] = exp(z[o] - mx));
      for (int o = 0; o < O; ++o) z[o] /= sum, dot += (double)g[n * O + o] * z[o];
      zs = 1.0;
    }
    for (int o = 0; o < O; ++o) {
      if (!close(y[n * O + o], z[o], 8.0 * (zs + 1.0))) return 1;
      glw[o] = softmax ? z[o] * (g[n * O + o] - dot) : g[n * O + o];
      if (softmax && !close(gl[n * O + o], glw[o], 8.0)) return 2;
    }
    for (int f = 0; f < F; ++f) {
      double want = 0.0, scale = 1.0;
      for (int o = 0; o < O; ++o) want += glw[o] * W[(size_t)o * F + f], scale += fabs(glw[o] * W[(size_t)o * F + f]);
      if (!close(dx[n * F + f], want, 8.0 * scale)) return 3;
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  auto note = [&](const char *what, int rc) {
    printf("%s %d\n", what, rc);
    fflush(stdout);
    bad += rc != 0;
  };
  // the product's pair; four problems of different R / column groups / N (two chunks each under a fill of 16: the second chunk
  // of the 5-row problem starts past its end); the ABI limits
  note("wgrad pair", run_wgrad({{3, 7, 50, 2, 200, -1}, {3, 7, 50, 0, 3, 0}}, -1, -1));
  note("wgrad mixed", run_wgrad({{3, 7, 13, 3, 5, -1}, {4, 11, 100, 0, 60, 1}, {5, 1, 13, 3, 150, 0}, {10, 7, 98, 2, 250, -1}}, -1, 16));
  note("wgrad limits", run_wgrad({{3, 3, 200, 55, 256, 1}}, -1, -1));
  // chunks of four stages, the last partial, chunk starts inside a sequence, every shift; T = 1
  for (int shift = -1; shift <= 1; ++shift) note("wgrad stages T=33", run_wgrad({{6, 33, 13, 3, 37, shift}}, 2, -1));
  note("wgrad stages T=32", run_wgrad({{7, 32, 13, 3, 37, -1}}, 2, -1));
  note("wgrad stages T=1", run_wgrad({{198, 1, 13, 3, 37, 1}}, 2, -1));
  note("wgrad one row tile, no x", run_wgrad({{5, 1, 50, 0, 5, 1}}, -1, -1));
  // mixture: every instance width, one row, capped slabs (19 / 25 rows per slab), a second round of the fold
  note("mix 21x8x768", run_mix(21, 8, 768, -1, -1));
  note("mix 1x3x128", run_mix(1, 3, 128, -1, -1));
  note("mix 37x2x128 capped", run_mix(37, 2, 128, 2, 2));
  note("mix 75x5x260 capped", run_mix(75, 5, 260, 3, 3));
  note("mix 1041x2x128", run_mix(1041, 2, 128, -1, -1));
  note("mix 45x3x544", run_mix(45, 3, 544, -1, -1));
  // linear heads: 64 / 32 / 16 rows per block with a ragged last block, one block, strided rows, the widest W, softmax at O = 1, 16
  note("linear 70 rows at 64", run_linear(70, 17, 5, false, 17, 1));
  note("linear 70 rows at 32", run_linear(70, 17, 5, false, 17, 2));
  note("linear 70 rows at 16", run_linear(70, 17, 5, false, 17, -1));
  note("linear softmax 70 rows at 64, strided", run_linear(70, 50, 7, true, 300, 1));
  note("linear 40 rows, one block, strided", run_linear(40, 17, 5, false, 102, 0));
  note("linear 128 x 96", run_linear(5, 128, 96, false, 128, -1));
  note("linear softmax O=1", run_linear(3, 50, 1, true, 50, -1));
  note("linear softmax O=16", run_linear(21, 50, 16, true, 50, -1));
  note("linear one row", run_linear(1, 100, 49, false, 100, -1));
  if (bad) return 1;
  printf("REDUCE-ASAN-OK\n");
  return 0;
}
