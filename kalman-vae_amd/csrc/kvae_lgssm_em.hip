// kvae_lgssm_em.hip — kvae_lgssm_switching_em (include/kvae_lgssm.h): the E-step of EM for the switching dynamics, one wavefront per
// sequence: the filter's sweep with its history kept, the smoother's backward pass with the expected sufficient statistics
// accumulated on the fly (one row of ws per sequence), the sum of the rows over the sequences, the per-sequence sums of the filter if
// asked for - at most four launches.  The bodies are csrc/lgssm_swf.h and csrc/lgssm_em.h (also run on emulated wavefronts by the
// CPU tier); this unit holds the __global__ wrappers and the entry points.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf; the compiler fuses nothing else (the note in kvae_lgssm_swf.hip): the
// forward here must give the bits of k_swf_sweep, the backward's smoother outputs the bits of k_sws_back, and the copies every
// group keeps of a reduced value must stay equal.
#pragma clang fp contract(off)

#include "lgssm_em.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_em;

__global__ __launch_bounds__(64) void k_em_fwd(kvae_swf_problem P, kvae_swf::History H) { kvae_swf::sweep_wave<1>(P, H); }
__global__ __launch_bounds__(64) void k_em_back(kvae_sws_problem S, kvae_em_stats E) { back_wave(S, E); }
__global__ __launch_bounds__(64) void k_em_reduce(kvae_sws_problem S, kvae_em_stats E) { reduce_thread(S, E); }
__global__ __launch_bounds__(64) void k_em_seq(kvae_swf_problem P) { kvae_swf::seq_wave(P); }

extern "C" int kvae_lgssm_switching_em(const kvae_sws_problem *prob, const kvae_em_stats *st, void *stream) {
  const int rc = em_check(prob, st);
  if (rc) return rc;
  const kvae_sws_problem &S = *prob;
  const kvae_em_stats &E = *st;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64), grid((unsigned)S.filt.B);
  const bool stats = em_wants_stats(E), back = stats || kvae_sws::sws_wants_back(S);
  if (back || kvae_swf::swf_wants_sweep(S.filt)) {
    k_em_fwd<<<grid, blk, 0, s>>>(S.filt, kvae_sws::sws_history(S));
    const int rs = kvae_launch_status("k_em_fwd");
    if (rs) return rs;
  }
  if (back) {
    k_em_back<<<grid, blk, 0, s>>>(S, E);
    const int rs = kvae_launch_status("k_em_back");
    if (rs) return rs;
  }
  if (stats) {
    k_em_reduce<<<dim3(em_reduce_grid(S)), blk, 0, s>>>(S, E);
    const int rs = kvae_launch_status("k_em_reduce");
    if (rs) return rs;
  }
  if (!S.filt.seq_ll) return KVAE_OK;
  k_em_seq<<<grid, blk, 0, s>>>(S.filt);
  return kvae_launch_status("k_em_seq");
}

extern "C" int64_t kvae_lgssm_switching_em_ws_floats(int32_t B, int32_t K, int32_t n, int32_t m) { return em_ws_floats(B, K, n, m); }
