// kvae_lgssm_swf.hip — kvae_lgssm_switching_filter (include/kvae_lgssm.h): the causal switching Kalman filter (GPB2) of a whole
// sequence in one launch, one wavefront per sequence, the per-sequence sums in a second.  The bodies are csrc/lgssm_swf.h (also run
// on emulated wavefronts by the CPU tier); this unit holds the __global__ wrappers and the entry point.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf.  The compiler fuses nothing else: a product that feeds a DPP reduction
// would otherwise be fused into the first addition in one partner's order and not the other's, the lanes of a group would no
// longer hold the same bits, and the bits of an output would depend on which others are requested.
#pragma clang fp contract(off)

#include "lgssm_swf.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_swf;

__global__ __launch_bounds__(64) void k_swf_sweep(kvae_swf_problem P) { sweep_wave<0>(P); }
__global__ __launch_bounds__(64) void k_swf_seq(kvae_swf_problem P) { seq_wave(P); }

extern "C" int kvae_lgssm_switching_filter(const kvae_swf_problem *prob, void *stream) {
  const int rc = swf_check(prob);
  if (rc) return rc;
  const kvae_swf_problem &P = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64), grid((unsigned)P.B);
  if (swf_wants_sweep(P)) {
    k_swf_sweep<<<grid, blk, 0, s>>>(P);
    const int rs = kvae_launch_status("k_swf_sweep");
    if (rs) return rs;
  }
  if (!P.seq_ll) return KVAE_OK;
  k_swf_seq<<<grid, blk, 0, s>>>(P);
  return kvae_launch_status("k_swf_seq");
}
