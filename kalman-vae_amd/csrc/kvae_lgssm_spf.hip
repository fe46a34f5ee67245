// kvae_lgssm_spf.hip — kvae_lgssm_switching_pf (include/kvae_lgssm.h): the Rao-Blackwellised particle filter of the switching
// model, a whole sequence in one launch, one workgroup of N particles per (sequence, replicate); the lineages in a second launch,
// the per-replicate sums in a third.  The bodies are csrc/lgssm_spf.h (also run on emulated workgroups by the CPU tier); this
// unit holds the __global__ wrappers and the entry point.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf; the compiler fuses nothing else (the note in kvae_lgssm_swf.hip): the
// predict of the drawn regime must give the bits of the same predict in the loop over the regimes, and the bits of an output
// must not depend on which others are requested.
#pragma clang fp contract(off)

#include "lgssm_spf.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_spf;

__global__ __launch_bounds__(MAX_PARTICLES) void k_spf_sweep(kvae_spf_problem P) { sweep_block(P); }
__global__ __launch_bounds__(MAX_PARTICLES) void k_spf_paths(kvae_spf_problem P) { paths_block(P); }
__global__ __launch_bounds__(64) void k_spf_seq(kvae_swf_problem S) { kvae_swf::seq_wave(S); }

extern "C" int kvae_lgssm_switching_pf(const kvae_spf_problem *prob, void *stream) {
  const int rc = spf_check(prob);
  if (rc) return rc;
  const kvae_spf_problem &P = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk((unsigned)P.N), grid((unsigned)(P.B * P.G));
  if (spf_wants_sweep(P)) {
    k_spf_sweep<<<grid, blk, 0, s>>>(P);
    const int rs = kvae_launch_status("k_spf_sweep");
    if (rs) return rs;
  }
  if (P.paths) {
    k_spf_paths<<<grid, blk, 0, s>>>(P);
    const int rs = kvae_launch_status("k_spf_paths");
    if (rs) return rs;
  }
  if (!P.seq_ll) return KVAE_OK;
  k_spf_seq<<<grid, dim3(64), 0, s>>>(seq_problem(P));
  return kvae_launch_status("k_spf_seq");
}
