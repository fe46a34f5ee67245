// step_asan_driver.cpp — TEST-ONLY: k_grad_sumsq / k_clip_adam (csrc/clip_adam.h), k_loss_head_fwd / bwd (csrc/vae_heads.h), the
// three column-sum kernels (csrc/colsum.h), k_emission_means (csrc/emission_means.h) and the five conv-epilogue kernels
// (csrc/vae_epilogue.h) on emulated workgroups (wave_emu.h, through the launch code of wave_emu_step.cpp), as a stand-alone
// program that tests/test_wave_emu_step.py builds twice - with -fsanitize=address,undefined and with -fsanitize=thread - and runs
// as a child process.  Every operand is a heap block that ENDS with its last element (a misaligned operand starts one float into
// its block), the LDS arrays are the emulator's exact-size allocations: a float4 load one quad past a buffer, a row of the
// four-rows-in-flight loop past `rows`, a bin past C r^2 is an AddressSanitizer report; an LDS slot read before its barrier, or
// any unordered access other than the float atomics of the bias bins, is a ThreadSanitizer report.  The results are compared
// with double-precision loops as well.
#include "wave_emu_step.cpp"

#include <random>
#include <vector>

static int g_notes[64];
extern "C" void kvae_wemu_rnn_note(int which) { g_notes[which] += 1; }
static int took(int which) {   // launches of one instance since the last look
  const int n = g_notes[which];
  g_notes[which] = 0;
  return n;
}

// n floats that end where the heap block ends, `off` floats past a 16-byte boundary
struct Buf {
  Buf(size_t n, int off = 0, float fillv = NAN) : n(n) {
    void *raw = nullptr;
    if (posix_memalign(&raw, 16, sizeof(float) * (n + off) + (n + off == 0)) != 0) abort();
    base = static_cast<float *>(raw), p = base + off;
    for (size_t i = 0; i < n; ++i) p[i] = fillv;
  }
  Buf(const Buf &) = delete;
  ~Buf() { free(base); }
  float &operator[](size_t i) { return p[i]; }
  float *base, *p;
  size_t n;
};
static std::mt19937 g_rng(4321);
static void fill(Buf &b, float scale = 1.f) {
  std::normal_distribution<float> nd(0.f, 1.f);
  for (size_t i = 0; i < b.n; ++i) b[i] = scale * nd(g_rng);
}
static bool close(double got, double want, double scale) { return fabs(got - want) <= 2e-5 * scale + 1e-30 && std::isfinite(got); }

// ---- clip + Adam ---------------------------------------------------------------------------------------------------------------
static int run_adam(int64_t n, int n_seg, int parts_cap, int blocks_cap, int frozen_seg, int off) {
  Buf p(n, off), g(n, off), m(n, off), v(n, off), steps(n_seg), active(n_seg), norm(1), div(1);
  fill(p, 1e-2f), fill(g), fill(m, 0.1f);
  for (int64_t i = 0; i < n; ++i) v[i] = 1e-3f + 1e-2f * (float)(i % 7);
  std::vector<int32_t> seg_of(n);
  for (int64_t i = 0; i < n; ++i) seg_of[i] = (int32_t)(i * n_seg / n);
  for (int s = 0; s < n_seg; ++s) steps[s] = (float)(s % 5), active[s] = s == frozen_seg ? 0.f : 1.f;
  div[0] = 3.f;
  kvae_wemu_clip_adam_parts(parts_cap), kvae_wemu_clip_adam_max_blocks(blocks_cap);
  const unsigned parts = ca_parts(n, parts_cap < 0 ? CA_BLOCKS : parts_cap);
  Buf ws(parts);
  std::vector<double> p0(p.p, p.p + n), m0(m.p, m.p + n), v0(v.p, v.p + n);
  const float lr = 3e-3f, b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, wd = 1e-2f, clip = 0.5f;
  kvae_wemu_clip_adam(p.p, g.p, m.p, v.p, n, n_seg > 1 ? seg_of.data() : nullptr, n_seg, active.p, steps.p, nullptr, lr, b1, b2, eps, wd,
                      clip, div.p, norm.p, ws.p);
  kvae_wemu_clip_adam_parts(-1), kvae_wemu_clip_adam_max_blocks(-1);
  if (took(kSumsq) != 1 || took(kClipAdam) != 1) return 1;
  double ss = 0.0;
  for (int64_t i = 0; i < n; ++i)
    if (active[n_seg > 1 ? seg_of[i] : 0] != 0.f) ss += (double)g[i] / 3.0 * g[i] / 3.0;
  if (!close(norm[0], sqrt(ss), sqrt(ss))) return 2;
  const double scale = (1.0 / 3.0) * fmin((double)clip / (sqrt(ss) + 1e-6), 1.0);
  for (int64_t i = 0; i < n; ++i) {
    const int s = n_seg > 1 ? seg_of[i] : 0;
    if (active[s] == 0.f) {
      if (p[i] != (float)p0[i] || m[i] != (float)m0[i] || v[i] != (float)v0[i]) return 3;
      continue;
    }
    const double step = (s % 5) + 1, gi = (double)g[i] * scale + (double)wd * p0[i];
    const double mi = m0[i] + (gi - m0[i]) * (1.0 - (double)b1), vi = (double)b2 * v0[i] + (1.0 - (double)b2) * gi * gi;
    const double upd = (double)lr / (1.0 - pow((double)b1, step)) * mi / (sqrt(vi) / sqrt(1.0 - pow((double)b2, step)) + (double)eps);
    if (steps[s] != (float)step) return 4;
    if (!close(m[i], mi, fabs(mi) + 1e-3) || !close(v[i], vi, fabs(vi) + 1e-6) || !close(p[i], p0[i] - upd, fabs(p0[i]) + fabs(upd)))
      return 5;
  }
  if (frozen_seg >= 0 && steps[frozen_seg] != (float)(frozen_seg % 5)) return 6;
  return 0;
}

// ---- loss head -----------------------------------------------------------------------------------------------------------------
static int run_head(int64_t n, bool masked, int off_lpx, int off_mask) {
  Buf lpx(n, off_lpx), regf(n), mask(masked ? n : 0, off_mask), kf(1), beta(1), out(6), coef(3), g(1), g_lpx(n), g_regf(n), g_kf(1);
  fill(lpx, 50.f), fill(regf), fill(kf);
  for (size_t i = 0; i < mask.n; ++i) mask[i] = (i % 3) ? 1.f : 0.f;
  beta[0] = 0.7f, g[0] = 2.5f;
  const float scale = 0.3f, vae_w = 1.5f, kf_w = 0.8f;
  kvae_wemu_loss_head_fwd(lpx.p, regf.p, masked ? mask.p : nullptr, kf.p, beta.p, scale, vae_w, kf_w, nullptr, out.p, coef.p, n);
  kvae_wemu_epi_max_blocks(3);
  kvae_wemu_loss_head_bwd(g.p, coef.p, masked ? mask.p : nullptr, g_lpx.p, g_regf.p, g_kf.p, n);
  kvae_wemu_epi_max_blocks(-1);
  if (took(kHeadFwd) != 1 || took(kHeadBwd) != 1) return 1;
  double s0 = 0, s1 = 0, s2 = 0, a0 = 0, a1 = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double mk = masked ? mask[i] : 1.0;
    s0 += lpx[i] * mk, s1 += regf[i] * mk, s2 += mk, a0 += fabs(lpx[i] * mk), a1 += fabs(regf[i] * mk);
  }
  const double denom = s2 > 1.0 ? s2 : 1.0;
  if (!close(out[4], s0 / denom, a0 / denom + 1e-30) || !close(out[5], s1 / denom, a1 / denom + 1e-30)) return 2;
  if (!close(coef[0], -(double)vae_w * scale / denom, 1.0 / denom) || !close(coef[1], -(double)vae_w * 0.7f / denom, 1.0 / denom) ||
      coef[2] != kf_w)
    return 3;
  if (out[0] != -out[1] || out[2] != kf[0]) return 4;
  for (int64_t i = 0; i < n; ++i) {
    const float mk = masked ? mask[i] : 1.f;
    if (g_lpx[i] != g[0] * coef[0] * mk || g_regf[i] != g[0] * coef[1] * mk) return 5;
  }
  return g_kf[0] == -coef[2] * g[0] ? 0 : 6;
}

// ---- column sums ---------------------------------------------------------------------------------------------------------------
static int check_colsum(Buf &x, Buf &out, int64_t rows, int64_t cols) {
  for (int64_t c = 0; c < cols; ++c) {
    double want = 0.0, scale = 0.0;
    for (int64_t r = 0; r < rows; ++r) want += x[r * cols + c], scale += fabs(x[r * cols + c]);
    if (!close(out[c], want, scale)) return 2;
  }
  return 0;
}
static int run_colsum(int64_t rows, int64_t cols, int off_in, int off_out) {
  Buf x(rows * cols, off_in), out(cols, off_out);
  fill(x);
  kvae_wemu_colsum(x.p, out.p, rows, cols);
  const bool v4 = cols % 4 == 0 && !off_in && !off_out;
  if (took(kColsumV4) != (v4 ? 1 : 0) || took(kColsum) != (v4 ? 0 : 1)) return 1;
  return check_colsum(x, out, rows, cols);
}
static int run_colsum2(int64_t ra, int64_t ca, int64_t rb, int64_t cb, int off_b) {
  Buf a(ra * ca), b(rb * cb), oa(ca), ob(cb, off_b);
  fill(a), fill(b);
  kvae_wemu_colsum2(a.p, oa.p, ra, ca, b.p, ob.p, rb, cb);
  const bool pair = ca % 4 == 0 && cb % 4 == 0 && !off_b;
  if (took(kColsumV4Pair) != (pair ? 1 : 0) || took(kColsumV4) + took(kColsum) != (pair ? 0 : 2)) return 1;
  const int rc = check_colsum(a, oa, ra, ca);
  return rc ? rc : check_colsum(b, ob, rb, cb);
}

// ---- emission means --------------------------------------------------------------------------------------------------------------
static int run_emission(int B, int T, int n, int p, bool both) {
  const int64_t BT = (int64_t)B * T;
  Buf Cm(BT * p * n), ms(BT * n), mf(both ? BT * n : 0), a_s(BT * p), a_f(both ? BT * p : 0);
  fill(Cm), fill(ms), fill(mf);
  kvae_lgssm_problem prob;
  memset(&prob, 0, sizeof(prob));
  prob.B = B, prob.T = T, prob.n = n, prob.m = n, prob.p = p;
  prob.C.ptr = Cm.p, prob.C.sb = (int64_t)T * p * n, prob.C.st = (int64_t)p * n;
  kvae_wemu_emission_means(&prob, ms.p, both ? mf.p : nullptr, a_s.p, both ? a_f.p : nullptr);
  if (took(kEmission) != 1) return 1;
  for (int64_t q = 0; q < BT; ++q)
    for (int i = 0; i < p; ++i) {
      double s = 0, f = 0, sa = 0, fa = 0;
      for (int k = 0; k < n; ++k) {
        const double c = Cm[(q * p + i) * n + k];
        s += c * ms[q * n + k], sa += fabs(c * ms[q * n + k]);
        if (both) f += c * mf[q * n + k], fa += fabs(c * mf[q * n + k]);
      }
      if (!close(a_s[q * p + i], s, sa) || (both && !close(a_f[q * p + i], f, fa))) return 2;
    }
  return 0;
}

// ---- conv epilogues --------------------------------------------------------------------------------------------------------------
struct Shape { int64_t N; int C, H, W, r; };
static int64_t src_of(const Shape &s, int64_t o, int *ch) {   // pixel_shuffle, written from its definition
  const int OW = s.W * s.r, OH = s.H * s.r;
  const int ow = (int)(o % OW), oh = (int)(o / OW % OH), c = (int)(o / ((int64_t)OW * OH) % s.C);
  const int64_t n = o / ((int64_t)OW * OH * s.C);
  *ch = c * s.r * s.r + (oh % s.r) * s.r + ow % s.r;
  return ((n * s.C * s.r * s.r + *ch) * s.H + oh / s.r) * s.W + ow / s.r;
}
static int run_epi_fwd(Shape s, int off_in, int off_out, int relu, int cap, int want_kernel) {
  const int Cin = s.C * s.r * s.r;
  const int64_t total = s.N * Cin * s.H * s.W;
  Buf in(total, off_in), bias(Cin), out(total, off_out);
  fill(in), fill(bias);
  kvae_wemu_epi_max_blocks(cap);
  kvae_wemu_epilogue_fwd(in.p, bias.p, out.p, s.N, s.C, s.H, s.W, s.r, relu);
  kvae_wemu_epi_max_blocks(-1);
  const int ran[3] = {took(kEpiFwd), took(kEpiFwdV4), took(kEpiFwdV4 + 1)};
  for (int k = 0; k < 3; ++k)
    if (ran[k] != (k == want_kernel ? 1 : 0)) return 1;
  for (int64_t o = 0; o < total; ++o) {
    int ch;
    const int64_t i = src_of(s, o, &ch);
    float want = in[i] + bias[ch];
    if (relu && !(want > 0.f)) want = 0.f;
    if (out[o] != want) return 2;
  }
  return 0;
}
static int run_epi_bwd(Shape s, int relu, bool want_bias, int per_chunk, int cap) {
  const int Cin = s.C * s.r * s.r;
  const int64_t total = s.N * Cin * s.H * s.W;
  kvae_wemu_epi_samples_per_chunk(per_chunk), kvae_wemu_epi_max_blocks(cap);
  const int64_t rows = kvae_wemu_bias_partial_rows(s.N);
  Buf g(total), out(relu ? total : 0), g_in(total), bp(want_bias ? rows * Cin : 0);
  fill(g), fill(out);
  if (relu) out[0] = 0.f, out[1] = -0.f, out[2] = NAN;
  kvae_wemu_epilogue_bwd(g.p, relu ? out.p : nullptr, g_in.p, want_bias ? bp.p : nullptr, s.N, s.C, s.H, s.W, s.r, relu);
  kvae_wemu_epi_samples_per_chunk(-1), kvae_wemu_epi_max_blocks(-1);
  if (took(kEpiBwdBias) != (want_bias ? 1 : 0) || took(kEpiBwd) != (want_bias ? 0 : 1)) return 1;
  std::vector<double> sum(Cin, 0.0), mag(Cin, 0.0);
  for (int64_t o = 0; o < total; ++o) {
    int ch;
    const int64_t i = src_of(s, o, &ch);
    const float want = (relu && !(out[o] > 0.f)) ? 0.f : g[o];
    if (g_in[i] != want) return 2;
    sum[ch] += want, mag[ch] += fabs(want);
  }
  for (int ch = 0; ch < Cin && want_bias; ++ch) {
    double got = 0.0;
    for (int64_t r = 0; r < rows; ++r) got += bp[r * Cin + ch];
    if (!close(got, sum[ch], mag[ch])) return 3;
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
  // clip + Adam: the block edges, a frozen segment, misaligned buffers, the most segments; both grid-stride loops through lowered
  // caps (2 partials, 3 blocks: 1793 = 2 rounds of 768 + 257)
  for (int64_t n : {1, 255, 256, 257, 1025}) note("adam one segment", run_adam(n, 1, -1, -1, -1, 0));
  note("adam 3 segments, one frozen", run_adam(348, 3, -1, -1, 1, 0));
  note("adam misaligned", run_adam(348, 3, -1, -1, -1, 1));
  note("adam 1024 segments", run_adam(2049, 1024, -1, -1, 700, 0));
  note("adam capped grids", run_adam(1793, 3, 2, 3, -1, 0));
  // loss head: n at the float4 / scalar gate and the edges of the 1024-thread block, with and without a mask, misaligned operands
  for (int64_t n : {1, 3, 4, 1023, 1024, 1025, 4097}) {
    note("head masked", run_head(n, true, 0, 0));
    note("head all observed", run_head(n, false, 0, 0));
  }
  note("head 4096 exact quads", run_head(4096, true, 0, 0));
  note("head 4100 second vector round", run_head(4100, false, 0, 0));
  note("head lpx misaligned", run_head(4096, true, 1, 0));
  note("head mask misaligned", run_head(1024, true, 0, 1));
  // column sums: every remainder of the four-rows-in-flight loop; cols one quad short of, at and past a block of 64 lanes
  for (int64_t rows : {1, 7, 8, 9, 25, 32, 33}) {
    for (int64_t cols : {4, 252, 256, 260}) note("colsum v4", run_colsum(rows, cols, 0, 0));
    for (int64_t cols : {1, 63, 65}) note("colsum scalar", run_colsum(rows, cols, 0, 0));
    note("colsum input misaligned", run_colsum(rows, 8, 1, 0));
    note("colsum output misaligned", run_colsum(rows, 256, 0, 1));
  }
  note("colsum pair", run_colsum2(33, 260, 7, 4, 0));
  note("colsum pair, unequal blocks", run_colsum2(9, 4, 25, 516, 0));
  note("colsum2 two launches (cols)", run_colsum2(33, 260, 7, 3, 0));
  note("colsum2 two launches (pointer)", run_colsum2(9, 4, 25, 8, 1));
  // emission means: one element, a second block (258 outputs), the largest dimensions
  note("emission 1x1x1x1", run_emission(1, 1, 1, 1, true));
  note("emission 43x3x4x2", run_emission(43, 3, 4, 2, true));
  note("emission 5x13x16x16 smoothed only", run_emission(5, 13, 16, 16, false));
  // conv epilogue forward: v4<1>, v4<2> (one and three quads per row), scalar by shape and by pointer; grid-stride rounds (cap 3)
  for (int relu = 0; relu <= 1; ++relu) {
    note("epi fwd v4<1>", run_epi_fwd({3, 5, 3, 4, 1}, 0, 0, relu, -1, 1));
    note("epi fwd v4<2> W/2=1", run_epi_fwd({2, 3, 3, 2, 2}, 0, 0, relu, -1, 2));
    note("epi fwd v4<2>", run_epi_fwd({2, 3, 3, 6, 2}, 0, 0, relu, -1, 2));
    note("epi fwd scalar W=5", run_epi_fwd({2, 3, 3, 5, 1}, 0, 0, relu, -1, 0));
    note("epi fwd scalar W=3 r=2", run_epi_fwd({2, 3, 3, 3, 2}, 0, 0, relu, -1, 0));
    note("epi fwd scalar r=3", run_epi_fwd({2, 3, 5, 7, 3}, 0, 0, relu, -1, 0));
    note("epi fwd in misaligned", run_epi_fwd({3, 5, 3, 4, 1}, 1, 0, relu, -1, 0));
    note("epi fwd out misaligned", run_epi_fwd({2, 3, 3, 6, 2}, 0, 1, relu, -1, 0));
  }
  note("epi fwd v4<2> rounds", run_epi_fwd({150, 2, 1, 6, 2}, 0, 0, 1, 3, 2));
  note("epi fwd v4<1> rounds", run_epi_fwd({150, 3, 1, 16, 1}, 0, 0, 1, 3, 1));
  note("epi fwd scalar rounds", run_epi_fwd({200, 1, 1, 1, 3}, 0, 0, 1, 3, 0));
  // backward: the chunk edges (N = 1, 31, 32, 33, 65 at 32 samples per chunk; 3, 4, 5 at 2), a ragged last block, 260 channels,
  // relu off with `out` NULL, no bias partials (and its grid-stride rounds)
  for (int64_t N : {1, 31, 32, 33, 65}) note("epi bwd chunks of 32", run_epi_bwd({N, 3, 2, 2, 2}, 1, true, -1, -1));
  for (int64_t N : {3, 4, 5}) note("epi bwd chunks of 2", run_epi_bwd({N, 3, 2, 2, 2}, 1, true, 2, -1));
  note("epi bwd ragged block", run_epi_bwd({2, 3, 5, 7, 2}, 1, true, -1, -1));
  note("epi bwd 260 channels", run_epi_bwd({2, 65, 1, 2, 2}, 1, true, -1, -1));
  note("epi bwd relu off", run_epi_bwd({33, 3, 2, 2, 2}, 0, true, -1, -1));
  note("epi bwd r=3", run_epi_bwd({2, 3, 5, 7, 3}, 1, true, -1, -1));
  note("epi bwd no bias r=3", run_epi_bwd({2, 3, 5, 7, 3}, 1, false, -1, -1));
  note("epi bwd no bias relu off", run_epi_bwd({3, 5, 3, 4, 1}, 0, false, -1, -1));
  note("epi bwd no bias rounds", run_epi_bwd({200, 1, 1, 1, 3}, 1, false, -1, 3));
  if (bad) return 1;
  printf("STEP-SAN-OK\n");
  return 0;
}
