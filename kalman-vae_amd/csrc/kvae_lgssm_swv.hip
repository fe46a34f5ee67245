// kvae_lgssm_swv.hip — kvae_lgssm_switching_viterbi (include/kvae_lgssm.h): the approximate Viterbi decoder of the switching model.
// One launch, one wavefront per sequence: the sweep over the K^2 pair steps with a selection in place of the GPB2 collapse, then the
// backtrace and the gather of the survivor beliefs by the same wavefront.  The body is csrc/lgssm_swv.h (also run on emulated
// wavefronts by the CPU tier); this unit holds the __global__ wrapper and the entry point.
#include <hip/hip_runtime.h>

// Every multiply-add of the body is an explicit fmaf; the compiler fuses nothing else (the note in kvae_lgssm_swf.hip): the pair
// step must give the bits of the filter's, and the copies every group keeps of a reduced value must stay equal.
#pragma clang fp contract(off)

#include "lgssm_swv.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_swv;

__global__ __launch_bounds__(64) void k_swv_sweep(kvae_swv_problem V) { viterbi_wave(V); }

extern "C" int kvae_lgssm_switching_viterbi(const kvae_swv_problem *prob, void *stream) {
  const int rc = swv_check(prob);
  if (rc) return rc;
  const kvae_swv_problem &V = *prob;
  if (!swv_wants_sweep(V)) return KVAE_OK;
  k_swv_sweep<<<dim3((unsigned)V.B), dim3(64), 0, (hipStream_t)stream>>>(V);
  return kvae_launch_status("k_swv_sweep");
}
