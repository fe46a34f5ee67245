// kvae_lgssm_swh.hip — kvae_lgssm_switching_forecast (include/kvae_lgssm.h): multi-horizon forecasts of the switching model (GPB2).
// The filter's sweep with its history kept, one wavefront per sequence; the forecast over that history, one wavefront per
// (sequence, origin); the per-sequence sums of the filter if asked for - at most three launches.  The bodies are csrc/lgssm_swf.h
// and csrc/lgssm_swh.h (also run on emulated wavefronts by the CPU tier); this unit holds the __global__ wrappers and the entry
// point.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf; the compiler fuses nothing else (the note in kvae_lgssm_swf.hip): the
// forward here must give the bits of k_swf_sweep, a horizon step the bits of the filter's hidden step, and the copies every group
// keeps of a reduced value must stay equal.
#pragma clang fp contract(off)

#include "lgssm_swh.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_swh;

__global__ __launch_bounds__(64) void k_swh_fwd(kvae_swf_problem P, kvae_swf::History H) { kvae_swf::sweep_wave<2>(P, H); }
__global__ __launch_bounds__(64) void k_swh_forecast(kvae_swh_problem F) { forecast_wave(F); }
__global__ __launch_bounds__(64) void k_swh_seq(kvae_swf_problem P) { kvae_swf::seq_wave(P); }

extern "C" int kvae_lgssm_switching_forecast(const kvae_swh_problem *prob, void *stream) {
  const int rc = swh_check(prob);
  if (rc) return rc;
  const kvae_swh_problem &F = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64), grid((unsigned)F.filt.B);
  const bool fore = swh_wants_forecast(F);
  if (fore || kvae_swf::swf_wants_sweep(F.filt)) {
    k_swh_fwd<<<grid, blk, 0, s>>>(F.filt, swh_history(F));
    const int rs = kvae_launch_status("k_swh_fwd");
    if (rs) return rs;
  }
  if (fore) {
    k_swh_forecast<<<dim3(swh_grid(F)), blk, 0, s>>>(F);
    const int rs = kvae_launch_status("k_swh_forecast");
    if (rs) return rs;
  }
  if (!F.filt.seq_ll) return KVAE_OK;
  k_swh_seq<<<grid, blk, 0, s>>>(F.filt);
  return kvae_launch_status("k_swh_seq");
}
