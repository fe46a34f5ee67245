// kvae_lgssm_pred_bwd.hip — kvae_lgssm_predictive_bwd (include/kvae_lgssm.h): the adjoint of kvae_lgssm_predictive, every (b, t)
// item in one launch.  The bodies are csrc/lgssm_pred.h (also run on emulated wavefronts by the CPU tier); this unit holds the
// __global__ wrappers and the entry point (a unit of its own: the resource report of kvae_lgssm_pred.hip stays the forward's).
#include <hip/hip_runtime.h>

// As kvae_lgssm_pred.hip: every multiply-add of the bodies is an explicit fmaf and the compiler fuses nothing else, so that S, r
// and the ladder level are recomputed to the forward's bits and no output's bits depend on which outputs are requested.
#pragma clang fp contract(off)

#include "lgssm_pred.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_pred;

__global__ __launch_bounds__(64) void k_pred_bwd_n4(kvae_pred_problem P, kvae_pred_grads G) { bwd_n4_wave(P, G); }
__global__ __launch_bounds__(64) void k_pred_bwd_n16(kvae_pred_problem P, kvae_pred_grads G) { bwd_n16_wave(P, G); }
__global__ __launch_bounds__(64) void k_pred_bwd_rt(kvae_pred_problem P, kvae_pred_grads G) { bwd_rt_wave(P, G); }

// one launch over the B*T items
extern "C" int kvae_lgssm_predictive_bwd(const kvae_pred_problem *prob, const kvae_pred_grads *g, void *stream) {
  const int rc = pred_bwd_check(prob, g);
  if (rc) return rc;
  const kvae_pred_problem &P = *prob;
  const kvae_pred_grads &G = *g;
  if (!pred_bwd_wants(G)) return KVAE_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64), grid(pred_bwd_grid(P, G));
  switch (pred_bwd_kind(P, G)) {
    case 0: k_pred_bwd_n4<<<grid, blk, 0, s>>>(P, G); break;
    case 1: k_pred_bwd_n16<<<grid, blk, 0, s>>>(P, G); break;
    default: k_pred_bwd_rt<<<grid, blk, 0, s>>>(P, G); break;
  }
  return kvae_launch_status("k_pred_bwd");
}
