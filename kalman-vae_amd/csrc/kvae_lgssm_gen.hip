// kvae_lgssm_gen.hip — kvae_lgssm_generate (include/kvae_lgssm.h): the closed-loop rollout of KVAE.generate in one launch.
// The body is csrc/lgssm_gen.h (also run on emulated wavefronts by the CPU tier); this unit holds the __global__ wrappers, the
// instantiations and the argument checks.
#include <hip/hip_runtime.h>

#include "lgssm_gen.h"

extern "C" int kvae_launch_status(const char *what);   // kvae_lgssm.hip: hipGetLastError -> KVAE_OK / KVAE_ERR_LAUNCH

using namespace kvae_gen;

template <int G, int NC, int MC, bool SWITCH>
__global__ __launch_bounds__(64) void k_generate(kvae_gen_problem P) {
  __shared__ Lds<G, !SWITCH> L;
  generate_wave<G, NC, MC, SWITCH>(P, L);
}

template <int G>
static void launch_generate(const kvae_gen_problem &P, unsigned grid, hipStream_t s) {
  if (P.kind == 1) k_generate<G, 0, 0, true><<<dim3(grid), dim3(64), 0, s>>>(P);
  else if (P.n == 4 && P.m == 4) k_generate<G, 4, 4, false><<<dim3(grid), dim3(64), 0, s>>>(P);
  else if (P.n == 16 && P.m == 16) k_generate<G, 16, 16, false><<<dim3(grid), dim3(64), 0, s>>>(P);
  else k_generate<G, 0, 0, false><<<dim3(grid), dim3(64), 0, s>>>(P);
}

extern "C" int kvae_lgssm_generate(const kvae_gen_problem *prob, void *stream) {
  const int rc = gen_check(prob);
  if (rc) return rc;
  const int64_t R = (int64_t)prob->B * prob->S;
  const int G = gen_rollouts_per_wave(R);
  const unsigned grid = (unsigned)((R + G - 1) / G);
  if (G == 4) launch_generate<4>(*prob, grid, (hipStream_t)stream);
  else launch_generate<8>(*prob, grid, (hipStream_t)stream);
  return kvae_launch_status("k_generate");
}
