// kvae_lgssm_rnn.hip — parameter gradients of the alpha-network recurrences and their linear heads (rnn_wgrad.h,
// small_linear.h): what round 2 left to rocBLAS inside the captured LGSSM chain.  Public entry points: kvae_lgssm.hip.
#include <hip/hip_runtime.h>

#include "../../include/kvae_lgssm.h"
#include "rnn_wgrad.h"
#include "small_linear.h"

using namespace kvae;

static_assert(sizeof(kvae_wgrad_problem) == sizeof(WgradProblem), "C-ABI struct and kernel struct must agree");

extern "C" int64_t kvae_rnn_wgrad_ws_floats(const kvae_wgrad_problem *probs, int32_t n) {
  return wg_ws_floats(probs, n, WG_MAX_CHUNKS);
}

// returns 0, or a KVAE_ERR_* code for bad arguments (nothing launched)
extern "C" int kvae_rnn_launch_wgrad(const kvae_wgrad_problem *probs, int32_t n, float *ws, hipStream_t s) {
  WgradBatch batch;
  batch.n = n;
  for (int i = 0; i < n; ++i) {
    const kvae_wgrad_problem &p = probs[i];
    const int bad = wg_check(p);
    if (bad) return bad == 1 ? KVAE_ERR_NULL : KVAE_ERR_ARG;
    WgradProblem &q = batch.p[i];
    q.d = p.d, q.h = p.h, q.x = p.x, q.g_wh = p.g_wh, q.g_wx = p.g_wx, q.g_b = p.g_b;
    q.d_stride = p.d_stride, q.h_stride = p.h_stride, q.x_stride = p.x_stride, q.N = p.N;
    q.R = p.R, q.H = p.H, q.I = p.I, q.bias = p.bias, q.T = p.T, q.shift = p.shift;
  }
  // split-K: about two workgroups per CU over all problems and column groups, at least one 32-row stage each (rnn_wgrad.h)
  const WgGeom g = wg_geometry(probs, n, WG_MAX_CHUNKS, WG_FILL);
  const dim3 grid((unsigned)g.chunks, (unsigned)g.groups, (unsigned)n), block(256);
#define KVAE_WGRAD_PARTIAL(RT) k_rnn_wgrad_partial<RT><<<grid, block, 0, s>>>(batch, ws, g.stride, g.chunks)
  KVAE_WGRAD_DISPATCH(g.rt, KVAE_WGRAD_PARTIAL);
#undef KVAE_WGRAD_PARTIAL
  k_rnn_wgrad_final<<<dim3((unsigned)g.final_blocks, (unsigned)n), block, 0, s>>>(batch, ws, g.stride, g.chunks);
  return KVAE_OK;
}

extern "C" int kvae_rnn_launch_linear_fwd(const float *x, int64_t xs, int64_t N, int F, const float *W, const float *b, int O,
                                          int softmax, float *y, hipStream_t s) {
  const int rows = sl_rows_per_block(F, O, N, SL_MIN_BLOCKS);
  const size_t lds = sizeof(float) * sl_fwd_lds_floats(F, O, rows);
  const dim3 grid((unsigned)sl_fwd_blocks(N, rows));
  if (softmax)
    k_linear_softmax_fwd<<<grid, dim3(256), lds, s>>>(x, xs, N, F, W, b, O, y, rows);
  else
    k_linear_fwd<<<grid, dim3(256), lds, s>>>(x, xs, N, F, W, b, O, y, rows);
  return KVAE_OK;
}

extern "C" int kvae_rnn_launch_linear_bwd_input(const float *g, const float *y, int64_t N, int F, const float *W, int O,
                                                float *g_logit, float *dx, int64_t dxs, hipStream_t s) {
  const size_t lds = sizeof(float) * sl_bwd_lds_floats(F, O);
  const dim3 grid((unsigned)sl_bwd_blocks(N, F));
  if (y)
    k_linear_softmax_bwd_input<<<grid, dim3(256), lds, s>>>(g, y, N, F, W, O, g_logit, dx, dxs);
  else
    k_linear_bwd_input<<<grid, dim3(256), lds, s>>>(g, N, F, W, O, dx, dxs);
  return KVAE_OK;
}
