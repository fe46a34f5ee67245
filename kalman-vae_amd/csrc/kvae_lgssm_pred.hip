// kvae_lgssm_pred.hip — kvae_lgssm_predictive (include/kvae_lgssm.h): the predictive density of every (b, t) item in one launch,
// the per-sequence sums in a second (its adjoint: kvae_lgssm_pred_bwd.hip).  The bodies are csrc/lgssm_pred.h (also run on emulated wavefronts by the CPU tier); this
// unit holds the __global__ wrappers and the entry point.
#include <hip/hip_runtime.h>

// Every multiply-add of the bodies is an explicit fmaf.  The compiler fuses nothing else: a product that feeds both a DPP move
// and an add (row_sum) would otherwise be fused in one partner's order and not the other's, and the lanes of a row would no
// longer hold the same bits.
#pragma clang fp contract(off)

#include "lgssm_pred.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_pred;

__global__ __launch_bounds__(64) void k_pred_items_n4(kvae_pred_problem P) { items_n4_wave(P); }
__global__ __launch_bounds__(64) void k_pred_items_n16(kvae_pred_problem P) { items_n16_wave(P); }
__global__ __launch_bounds__(64) void k_pred_items_rt(kvae_pred_problem P) { items_rt_wave(P); }
__global__ __launch_bounds__(64) void k_pred_seq(kvae_pred_problem P) { seq_wave(P); }

extern "C" int kvae_lgssm_predictive(const kvae_pred_problem *prob, void *stream) {
  const int rc = pred_check(prob);
  if (rc) return rc;
  const kvae_pred_problem &P = *prob;
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64);
  if (pred_wants_items(P)) {
    const dim3 grid(pred_item_grid(P));
    switch (pred_kind(P)) {
      case 0: k_pred_items_n4<<<grid, blk, 0, s>>>(P); break;
      case 1: k_pred_items_n16<<<grid, blk, 0, s>>>(P); break;
      default: k_pred_items_rt<<<grid, blk, 0, s>>>(P); break;
    }
    const int ri = kvae_launch_status("k_pred_items");
    if (ri) return ri;
  }
  if (!P.seq_ll) return KVAE_OK;
  k_pred_seq<<<dim3((unsigned)P.B), blk, 0, s>>>(P);
  return kvae_launch_status("k_pred_seq");
}
