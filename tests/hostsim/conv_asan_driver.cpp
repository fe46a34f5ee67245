// conv_asan_driver.cpp — TEST-ONLY: the encoder's convolution kernels (csrc/vae_conv_mid.h: k_enc_mid_fwd / bwd_data / wrw<16 | 8>;
// csrc/vae_conv_edge.h: k_enc_stem_fwd / k_enc_stem_wrw / k_enc_stem_wrw_mfma<true | false>) on emulated workgroups (wave_emu.h,
// through the launch code of wave_emu_conv.cpp), as a stand-alone program that tests/test_wave_emu_conv.py builds twice - with
// -fsanitize=address,undefined and with -fsanitize=thread - and runs as a child process.  Every operand is a heap block that ENDS
// with its last element and the LDS arrays are the emulator's exact-size allocations.  The kernels' global traffic goes through
// buffer resources, which the emulator turns into plain accesses wherever an access is below num_records: a resource longer than
// its tensor, or a prefetch that is not past the end, is an AddressSanitizer report (on the card it reads a neighbour's memory
// into frames that are dropped); an LDS image rewritten while another wavefront still reads it out - the barriers that only
// matter when a wave is late - is a ThreadSanitizer report.  The results are compared with double-precision loops as well.
#include "wave_emu_conv.cpp"

#include <random>
#include <vector>

static int g_notes[64];
extern "C" void kvae_wemu_rnn_note(int which) { g_notes[which] += 1; }
static int took(int which) {   // launches of one instance since the last look
  const int n = g_notes[which];
  g_notes[which] = 0;
  return n;
}

// n elements that end where the heap block ends
template <class T>
struct BufT {
  explicit BufT(size_t n) : n(n) {
    void *raw = nullptr;
    if (posix_memalign(&raw, 16, sizeof(T) * n + (n == 0)) != 0) abort();
    p = static_cast<T *>(raw);
    memset(p, 0xFF, sizeof(T) * n);   // NaNs / all bits
  }
  BufT(const BufT &) = delete;
  ~BufT() { free(p); }
  T &operator[](size_t i) { return p[i]; }
  T *p;
  size_t n;
};
typedef BufT<float> Buf;
static std::mt19937 g_rng(97);
static void fill(Buf &b, float scale, bool relu) {
  std::normal_distribution<float> nd(0.f, 1.f);
  for (size_t i = 0; i < b.n; ++i) {
    const float v = scale * nd(g_rng);
    b[i] = relu && v < 0.f ? 0.f : v;
  }
}
static bool close(double got, double want, double scale) { return std::isfinite(got) && fabs(got - want) <= 2e-5 * scale + 1e-30; }

// out = relu(conv3x3 stride 2 pad 1 (x[N,C,S,S], W[32,C,3,3]) + b) and its gradients given the upstream g, in double
struct Ref {
  std::vector<double> out, pre, dx, dw, db;
};
static Ref reference(const float *x, const float *W, const float *b, const float *g, int64_t N, int C, int S) {
  const int O = S / 2;
  Ref r;
  r.out.assign(N * 32 * O * O, 0.0), r.pre = r.out, r.dx.assign(N * C * S * S, 0.0), r.dw.assign(32 * C * 9, 0.0), r.db.assign(32, 0.0);
  for (int64_t n = 0; n < N; ++n)
    for (int co = 0; co < 32; ++co)
      for (int oh = 0; oh < O; ++oh)
        for (int ow = 0; ow < O; ++ow) {
          double acc = b[co];
          for (int ci = 0; ci < C; ++ci)
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx) {
                const int y = 2 * oh + ky - 1, xx = 2 * ow + kx - 1;
                if (y < 0 || y >= S || xx < 0 || xx >= S) continue;
                acc += (double)W[(co * C + ci) * 9 + ky * 3 + kx] * x[((n * C + ci) * S + y) * S + xx];
              }
          const int64_t oi = ((n * 32 + co) * O + oh) * O + ow;
          r.out[oi] = acc > 0.0 ? acc : 0.0, r.pre[oi] = acc;
          if (!(acc > 0.0)) continue;
          r.db[co] += g[oi];
          for (int ci = 0; ci < C; ++ci)
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx) {
                const int y = 2 * oh + ky - 1, xx = 2 * ow + kx - 1;
                if (y < 0 || y >= S || xx < 0 || xx >= S) continue;
                const int64_t ii = ((n * C + ci) * S + y) * S + xx;
                r.dw[(co * C + ci) * 9 + ky * 3 + kx] += (double)g[oi] * x[ii];
                r.dx[ii] += (double)g[oi] * W[(co * C + ci) * 9 + ky * 3 + kx];
              }
        }
  return r;
}
static double amax(const std::vector<double> &v) {
  double m = 1e-30;
  for (double e : v) m = fmax(m, fabs(e));
  return m;
}
// rows of partials -> their column sums against `want`
static int check_partials(Buf &part, int64_t rows, int cols, const std::vector<double> &want) {
  const double scale = amax(want);
  for (int c = 0; c < cols; ++c) {
    double s = 0.0;
    for (int64_t r = 0; r < rows; ++r) s += part[r * cols + c];
    if (!close(s, want[c], scale)) return 1;
  }
  return 0;
}
// the upstream gradient is zeroed where the double pre-activation is too close to 0 for the mask to be anyone's but rounding's
static void zero_near(Buf &g, const float *x, const float *W, const float *b, int64_t N, int C, int S) {
  Buf zero(g.n);
  for (size_t i = 0; i < g.n; ++i) zero[i] = 0.f;
  const Ref r = reference(x, W, b, zero.p, N, C, S);
  for (size_t i = 0; i < g.n; ++i)
    if (fabs(r.pre[i]) < 1e-4) g[i] = 0.f;
}

// ---- enc_mid ---------------------------------------------------------------------------------------------------------------------
static int run_mid(int64_t N, int side, int cap) {
  const int O = side / 2;
  Buf x(N * 32 * side * side), W(EM_W), b(32), out(N * 32 * O * O), g(out.n), dx(x.n);
  fill(x, 1.f, true), fill(W, 0.08f, false), fill(b, 0.1f, false), fill(g, 1.f, false);
  zero_near(g, x.p, W.p, b.p, N, 32, side);
  kvae_wemu_enc_mid_max_wgs(cap);
  const int64_t rows = kvae_wemu_enc_mid_rows(N, side);
  Buf wp(rows * EM_W), bp(rows * 32);
  kvae_wemu_enc_mid_fwd(x.p, W.p, b.p, out.p, N, side);
  kvae_wemu_enc_mid_bwd(x.p, W.p, out.p, g.p, dx.p, wp.p, bp.p, N, side);
  kvae_wemu_enc_mid_max_wgs(-1);
  const int s = side == 16 ? 0 : 1;
  if (took(kMidFwd + s) != 1 || took(kMidData + s) != 1 || took(kMidWrw + s) != 1) return 1;
  const Ref r = reference(x.p, W.p, b.p, g.p, N, 32, side);
  const double so = amax(r.out), sx = amax(r.dx);
  for (size_t i = 0; i < out.n; ++i)
    if (!close(out[i], r.out[i], so)) return 2;
  for (size_t i = 0; i < dx.n; ++i)
    if (!close(dx[i], r.dx[i], sx)) return 3;
  if (check_partials(wp, rows, EM_W, r.dw)) return 4;
  if (check_partials(bp, rows, 32, r.db)) return 5;
  return 0;
}

// ---- stem ------------------------------------------------------------------------------------------------------------------------
static int run_stem(int64_t N, int cap) {
  Buf x(N * 1024), W(32 * 9), b(32), out(N * 32 * 256), g(out.n);
  BufT<uint32_t> bits(N * 256);
  fill(x, 1.f, true), fill(W, 0.3f, false), fill(b, 0.1f, false), fill(g, 1.f, false);
  zero_near(g, x.p, W.p, b.p, N, 1, 32);
  kvae_wemu_enc_stem_fwd(x.p, W.p, b.p, out.p, bits.p, N);
  if (took(kStemFwd) != 1) return 1;
  const Ref r = reference(x.p, W.p, b.p, g.p, N, 1, 32);
  const double so = amax(r.out);
  for (size_t i = 0; i < out.n; ++i)
    if (!close(out[i], r.out[i], so)) return 2;
  kvae_wemu_stem_max_rows(cap);
  const int64_t rows = kvae_wemu_conv_edge_rows(N);
  const int slot[3] = {kStemWrw, kStemWrwMfma, kStemWrwMfma + 1};
  int bad = 0;
  for (int mode = 0; mode < 3 && !bad; ++mode) {   // KVAE_STEM_MFMA = 0 | 1 | 2
    Buf wp(rows * 32 * 9), bp(rows * 32);
    kvae_wemu_stem_mode(mode);
    if (kvae_wemu_enc_stem_bwd(x.p, mode == 1 ? nullptr : out.p, mode == 1 ? bits.p : nullptr, g.p, wp.p, bp.p, N) != KVAE_OK) bad = 3;
    else if (took(slot[mode]) != 1) bad = 4;
    else if (check_partials(wp, rows, 32 * 9, r.dw)) bad = 5;
    else if (check_partials(bp, rows, 32, r.db)) bad = 6;
  }
  kvae_wemu_stem_mode(-1), kvae_wemu_stem_max_rows(-1);
  return bad;
}

int main() {
  int bad = 0;
  auto expect = [&](const char *what, long a, long b, int rc) {
    if (rc) {
      printf("FAIL %s(%ld, %ld): %d\n", what, a, b, rc);
      bad += 1;
    }
  };
  if (kvae_wemu_conv_selftest() != 0) printf("FAIL selftest\n"), bad += 1;
  // residues of the frames per iteration (2 | 8), one iteration per workgroup
  for (int64_t N : {1, 2, 3, 5}) expect("mid16", N, -1, run_mid(N, 16, -1));
  for (int64_t N : {1, 7, 8, 9, 13, 17}) expect("mid8", N, -1, run_mid(N, 8, -1));
  for (int64_t N : {1, 2, 3}) expect("stem", N, -1, run_stem(N, -1));
  // persistent rounds: five iterations on two and on three workgroups; five frames on two weight-gradient workgroups of the stem
  for (int cap : {2, 3}) {
    expect("mid16", 9, cap, run_mid(9, 16, cap));
    expect("mid8", 33, cap, run_mid(33, 8, cap));
  }
  expect("stem", 5, 2, run_stem(5, 2));
  if (bad == 0) printf("CONV-SAN-OK\n");
  return bad != 0;
}
