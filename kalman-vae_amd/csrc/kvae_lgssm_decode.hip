// kvae_lgssm_decode.hip — kvae_regime_decode (include/kvae_lgssm.h): marginals, MAP path and KL of the regime posterior in one
// launch, one wavefront per sequence.  The bodies are csrc/regime_decode.h (also run by the CPU tier's host simulation); this unit
// holds the __global__ wrappers and the entry points.
#include <hip/hip_runtime.h>

#include "regime_decode.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae;

__global__ __launch_bounds__(64) void k_regime_decode_grid(const float *logits, const float *init_logits, const float *Pm,
                                                           float *marginals, int32_t *path, float *path_logq, float *kl,
                                                           uint32_t *ws, int T, int K) {
  const int b = blockIdx.x;
  rdec::decode_grid(logits, init_logits, Pm, marginals, path, path_logq, kl, path ? ws + (int64_t)b * T : nullptr, b, T, K);
}
__global__ __launch_bounds__(64) void k_regime_decode_lds(const float *logits, const float *init_logits, const float *Pm,
                                                          float *marginals, int32_t *path, float *path_logq, float *kl,
                                                          uint64_t *ws, int T, int K) {
  __shared__ rdec::DecodeLds L;
  const int b = blockIdx.x;
  rdec::decode_body(logits, init_logits, Pm, marginals, path, path_logq, kl, path ? ws + (int64_t)b * T : nullptr, b, T, K, L);
}

extern "C" int64_t kvae_regime_decode_ws_bytes(int64_t B, int32_t T, int32_t K) { return rdec::decode_ws_bytes(B, T, K); }

extern "C" int kvae_regime_decode(const float *logits, const float *init_logits, const float *P, float *marginals, int32_t *path,
                                  float *path_logq, float *kl, void *ws, int32_t B, int32_t T, int32_t K, void *stream) {
  const int rc = rdec::decode_check(logits, init_logits, P, path, path_logq, ws, B, T, K);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (K <= 8) {
    k_regime_decode_grid<<<dim3(B), dim3(64), 0, s>>>(logits, init_logits, P, marginals, path, path_logq, kl, (uint32_t *)ws, T, K);
    return kvae_launch_status("k_regime_decode_grid");
  }
  k_regime_decode_lds<<<dim3(B), dim3(64), 0, s>>>(logits, init_logits, P, marginals, path, path_logq, kl, (uint64_t *)ws, T, K);
  return kvae_launch_status("k_regime_decode_lds");
}
