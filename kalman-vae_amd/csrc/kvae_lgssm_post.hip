// kvae_lgssm_post.hip — kvae_lgssm_posterior_sample (include/kvae_lgssm.h): joint posterior samples of latent paths in three
// launches, all gains at once | the paths | the emission.  The bodies are csrc/lgssm_post.h (also run on emulated wavefronts by the CPU tier);
// this unit holds the __global__ wrappers, the instantiations and the entry points.
#include <hip/hip_runtime.h>

#include "lgssm_post.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_post;

template <int NC, int LPI>
__global__ __launch_bounds__(64) void k_post_gains(kvae_psample_problem P) {
  __shared__ GainLds<NC, LPI> L;
  gains_wave<NC, LPI>(P, L);
}
__global__ __launch_bounds__(64) void k_post_paths_n4(kvae_psample_problem P) { paths_n4_wave(P); }
__global__ __launch_bounds__(64) void k_post_paths_n16(kvae_psample_problem P) { paths_n16_wave(P); }
__global__ __launch_bounds__(64) void k_post_emit(kvae_psample_problem P) { emit_wave(P); }
__global__ __launch_bounds__(64) void k_post_paths_lds(kvae_psample_problem P) {
  __shared__ PathLds L;
  paths_lds_wave(P, L);
}

extern "C" int64_t kvae_lgssm_posterior_sample_ws_floats(const kvae_psample_problem *prob) { return post_ws_floats(prob); }

extern "C" int kvae_lgssm_posterior_sample(const kvae_psample_problem *prob, void *stream) {
  const int rc = post_check(prob);
  if (rc) return rc;
  const kvae_psample_problem &P = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gg(post_gain_grid(P)), pg(post_path_grid(P)), blk(64);
  if (post_runs(P, KVAE_PSAMPLE_GAINS)) {
    switch (post_gain_kind(P)) {
      case 0: k_post_gains<4, 16><<<gg, blk, 0, s>>>(P); break;
      case 1: k_post_gains<16, 64><<<gg, blk, 0, s>>>(P); break;
      default: k_post_gains<0, 64><<<gg, blk, 0, s>>>(P); break;
    }
    const int rg = kvae_launch_status("k_post_gains");
    if (rg) return rg;
  }
  if (!post_runs(P, KVAE_PSAMPLE_PATHS)) return KVAE_OK;
  switch (post_path_kind(P)) {
    case 0: k_post_paths_n4<<<pg, blk, 0, s>>>(P); break;
    case 1: k_post_paths_n16<<<pg, blk, 0, s>>>(P); break;
    default: k_post_paths_lds<<<pg, blk, 0, s>>>(P); break;
  }
  const int rp = kvae_launch_status("k_post_paths");
  if (rp) return rp;
  k_post_emit<<<dim3(post_emit_grid(P)), blk, 0, s>>>(P);
  return kvae_launch_status("k_post_emit");
}
