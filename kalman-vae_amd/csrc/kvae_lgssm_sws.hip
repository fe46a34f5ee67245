// kvae_lgssm_sws.hip — kvae_lgssm_switching_smoother (include/kvae_lgssm.h): the switching Kalman smoother (GPB2) of a whole sequence,
// one wavefront per sequence: the filter's sweep with its history kept, the backward pass over that history, the per-sequence sums of
// the filter if asked for - at most three launches.  The bodies are csrc/lgssm_swf.h and csrc/lgssm_sws.h (also run on emulated
// wavefronts by the CPU tier); this unit holds the __global__ wrappers and the entry point.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf; the compiler fuses nothing else (the note in kvae_lgssm_swf.hip): the
// forward here must give the bits of k_swf_sweep, and the copies every group keeps of a reduced value must stay equal.
#pragma clang fp contract(off)

#include "lgssm_sws.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_sws;

__global__ __launch_bounds__(64) void k_sws_fwd(kvae_swf_problem P, kvae_swf::History H) { kvae_swf::sweep_wave<1>(P, H); }
__global__ __launch_bounds__(64) void k_sws_back(kvae_sws_problem S) { back_wave(S); }
__global__ __launch_bounds__(64) void k_sws_seq(kvae_swf_problem P) { kvae_swf::seq_wave(P); }

extern "C" int kvae_lgssm_switching_smoother(const kvae_sws_problem *prob, void *stream) {
  const int rc = sws_check(prob);
  if (rc) return rc;
  const kvae_sws_problem &S = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64), grid((unsigned)S.filt.B);
  const bool back = sws_wants_back(S);
  if (back || kvae_swf::swf_wants_sweep(S.filt)) {
    k_sws_fwd<<<grid, blk, 0, s>>>(S.filt, sws_history(S));
    const int rs = kvae_launch_status("k_sws_fwd");
    if (rs) return rs;
  }
  if (back) {
    k_sws_back<<<grid, blk, 0, s>>>(S);
    const int rs = kvae_launch_status("k_sws_back");
    if (rs) return rs;
  }
  if (!S.filt.seq_ll) return KVAE_OK;
  k_sws_seq<<<grid, blk, 0, s>>>(S.filt);
  return kvae_launch_status("k_sws_seq");
}
