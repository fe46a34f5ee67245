// kvae_lgssm_swm.hip — kvae_lgssm_switching_marginal / kvae_lgssm_switching_marginal_bwd (include/kvae_lgssm.h): log p(a | u) of the
// switching model with the regimes summed out (GPB2) and its adjoint.  Forward: the filter's sweep with its history kept, the
// per-sequence sums if asked for.  Backward: one wavefront per sequence over that history, then the sum of the per-sequence partials.
// The bodies are csrc/lgssm_swf.h and csrc/lgssm_swm.h (also run on emulated wavefronts by the CPU tier); this unit holds the
// __global__ wrappers and the entry points.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf; the compiler fuses nothing else (the note in kvae_lgssm_swf.hip): the
// forward here must give the bits of k_swf_sweep, the adjoint must recompute them, and the copies every group keeps of a reduced
// value must stay equal.
#pragma clang fp contract(off)

#include "lgssm_swm.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_swm;

__global__ __launch_bounds__(64) void k_swm_fwd(kvae_swf_problem P, kvae_swf::History H) { kvae_swf::sweep_wave<2>(P, H); }
__global__ __launch_bounds__(64) void k_swm_seq(kvae_swf_problem P) { kvae_swf::seq_wave(P); }
__global__ __launch_bounds__(64) void k_swm_bwd(kvae_swm_problem M, kvae_swm_grads G) { back_wave(M, G); }
__global__ __launch_bounds__(64) void k_swm_reduce(kvae_swm_problem M, kvae_swm_grads G) { reduce_thread(M, G); }

extern "C" int kvae_lgssm_switching_marginal(const kvae_swm_problem *prob, void *stream) {
  const int rc = swm_check(prob);
  if (rc) return rc;
  const kvae_swm_problem &M = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64), grid((unsigned)M.filt.B);
  k_swm_fwd<<<grid, blk, 0, s>>>(M.filt, swm_history(M));
  const int rs = kvae_launch_status("k_swm_fwd");
  if (rs || !M.filt.seq_ll) return rs;
  k_swm_seq<<<grid, blk, 0, s>>>(M.filt);
  return kvae_launch_status("k_swm_seq");
}

extern "C" int kvae_lgssm_switching_marginal_bwd(const kvae_swm_problem *prob, const kvae_swm_grads *g, void *stream) {
  const int rc = swm_bwd_check(prob, g);
  if (rc) return rc;
  const kvae_swm_problem &M = *prob;
  const kvae_swm_grads &G = *g;
  if (!swm_wants_back(G)) return KVAE_OK;
  hipStream_t s = (hipStream_t)stream;
  k_swm_bwd<<<dim3((unsigned)M.filt.B), dim3(64), 0, s>>>(M, G);
  const int rs = kvae_launch_status("k_swm_bwd");
  if (rs || !swm_wants_params(G)) return rs;
  k_swm_reduce<<<dim3(swm_reduce_grid(M)), dim3(64), 0, s>>>(M, G);
  return kvae_launch_status("k_swm_reduce");
}

extern "C" int64_t kvae_lgssm_switching_marginal_ws_floats(int32_t B, int32_t K, int32_t n, int32_t m) {
  return B < 1 || K < 1 || n < 1 || m < 1 ? 0 : (int64_t)B * layout(K, n, m).G;
}
