// decode_asan_driver.cpp — TEST-ONLY: both bodies of kvae_regime_decode (csrc/regime_decode.h: the lane grid of K <= 8 on emulated
// wavefronts (wave_emu.h), the LDS body of 8 < K <= 16 as the host simulation runs it), as a standalone program that
// tests/test_regime_decode.py builds with -fsanitize=address,undefined and runs as a child process, through the host simulation's
// entry point defined there.  Every buffer is allocated at its exact size - the workspace at kvae_regime_decode_ws_bytes - so a
// read or write past the layouts of include/kvae_lgssm.h is a sanitizer report.  Shapes: T = 1 (no transition is read), T = 2 on
// the full grid (the prefetch has no next step), ragged K, the LDS body at its smallest and largest K, and for both bodies more
// steps than the 64 backpointer words one pass of the backtrace reads back.
#define KVAE_HOSTSIM 1
#define KVAE_WAVE_EMU 1
#include "wave_emu.h"

#include <memory>
#include <random>
#include <vector>

#include "../../kalman-vae_amd/csrc/regime_decode.h"

static int run(int B, int T, int K) {
  std::mt19937 g(B * 1000 + T * 10 + K);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> logits((size_t)B * T * K * K), init((size_t)B * K), P((size_t)K * K, K > 1 ? 0.2f / (K - 1) : 1.f);
  for (auto &x : logits) x = nd(g);
  for (auto &x : init) x = nd(g);
  for (int k = 0; k < K && K > 1; ++k) P[(size_t)k * K + k] = 0.8f;
  std::vector<float> marg((size_t)B * T * K, NAN), kl((size_t)B * T, NAN), plq(B, NAN);
  std::vector<int32_t> path((size_t)B * T, -1);
  const int64_t wsb = kvae_regime_decode_ws_bytes(B, T, K);
  if (wsb != (int64_t)B * T * (K <= 8 ? 4 : 8)) return 1;
  std::unique_ptr<uint64_t[]> ws8;
  std::unique_ptr<uint32_t[]> ws4;
  void *ws;
  if (K <= 8) ws4.reset(new uint32_t[(size_t)B * T]), ws = ws4.get();
  else ws8.reset(new uint64_t[(size_t)B * T]), ws = ws8.get();
  const int before = kvae_wemu_regime_decode_launches(K <= 8 ? 0 : 1);
  if (kvae_regime_decode(logits.data(), init.data(), P.data(), marg.data(), path.data(), plq.data(), kl.data(), ws, B, T, K, nullptr))
    return 2;
  if (kvae_wemu_regime_decode_launches(K <= 8 ? 0 : 1) != before + 1) return 3;
  for (const auto *v : {&marg, &kl, &plq})
    for (float x : *v)
      if (!std::isfinite(x)) return 4;   // every output element written
  for (int32_t s : path)
    if (s < 0 || s >= K) return 5;
  // partial outputs: no workspace without a path, nothing else touched
  std::vector<float> marg2((size_t)B * T * K, NAN);
  if (kvae_regime_decode(logits.data(), init.data(), P.data(), marg2.data(), nullptr, nullptr, nullptr, nullptr, B, T, K, nullptr)) return 6;
  for (size_t e = 0; e < marg.size(); ++e)
    if (marg[e] != marg2[e]) return 7;
  return 0;
}

int main() {
  const int shapes[7][3] = {{2, 1, 8}, {2, 2, 8}, {3, 5, 3}, {2, 3, 9}, {1, 4, 16}, {1, 66, 2}, {1, 65, 10}};
  int bad = 0;
  for (const auto &s : shapes) {
    const int rc = run(s[0], s[1], s[2]);
    printf("(%d,%d,%d) %d\n", s[0], s[1], s[2], rc);
    bad += rc != 0;
  }
  if (bad) return 1;
  printf("DECODE-ASAN-OK\n");
  return 0;
}
