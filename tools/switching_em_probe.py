#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_em_statistics at one shape per invocation: the kernel (kvae_lgssm_switching_em: the forward with its
history kept, the backward with the statistics, the sum over the sequences, the sequence sums) asked for the twelve statistics and
log_lik_seq - what KalmanFilter.em_step asks for - the smoother's own call (lgssm_ops.switching_smoother, all outputs: remeasured in
the same run, the figure of DESIGN.md section 15), the filter's (section 14) and the torch restatement on the same device
(lgssm_ops.switching_em_statistics_torch).  HIP-event times, median of `iters` calls after warm-up.
`em_back_us_per_step` is (statistics) - (filter, log_lik_seq alone) over T: the backward pass with the accumulation (T transitions),
the history stores and the reduction, next to `smoother_back_us_per_step` = (smoother) - (filter), both with all outputs, over T.
The statistics of the kernel and of the float32 restatement are compared with the float64 restatement run on the device (largest
distance over the largest magnitude of the statistic).  One shape per process, so that a caller can put every shape under its own
time limit:
usage: python tools/switching_em_probe.py B,T,K [iters]      shapes of DESIGN.md section 15: 32,100,7  256,50,3  512,200,7"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd"), str(ROOT / "tools")]
import torch  # noqa: E402,F401

from kvae.kalman import lgssm_ops  # noqa: E402
from switching_filter_probe import inputs, med_ms  # noqa: E402


def main():
    B, T, K = (int(v) for v in sys.argv[1].split(","))
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    args = inputs(B, T, K)
    want = lgssm_ops._EM_STATS + ("log_lik_seq",)
    e_ms = med_ms(lambda: lgssm_ops.switching_em_statistics(*args, want=want, impl="hip"), iters)
    s_ms = med_ms(lambda: lgssm_ops.switching_smoother(*args, impl="hip"), iters)
    f_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, impl="hip"), iters)
    l_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, want=("log_lik_seq",), impl="hip"), iters)
    t_ms = med_ms(lambda: lgssm_ops.switching_em_statistics(*args, want=want, impl="torch"), 2)
    ker = lgssm_ops.switching_em_statistics(*args, want=want, impl="hip")
    f32 = lgssm_ops.switching_em_statistics(*args, want=want, impl="torch")
    ref = lgssm_ops.switching_em_statistics_torch(*(a.double() for a in args), want=want)   # float64, on the device
    rel = lambda got: {k: float((got[k].double() - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1.0)) for k in lgssm_ops._EM_STATS}
    print(json.dumps(dict(B=B, T=T, K=K, n=4, m=4, em_ms=round(e_ms, 4), smoother_ms=round(s_ms, 4), filter_ms=round(f_ms, 4),
                          filter_loglik_ms=round(l_ms, 4), torch_ms=round(t_ms, 3), speedup=round(t_ms / e_ms, 1),
                          em_back_us_per_step=round(1e3 * (e_ms - l_ms) / T, 3),
                          smoother_back_us_per_step=round(1e3 * (s_ms - f_ms) / T, 3), kernel_vs_float64=rel(ker),
                          float32_torch_vs_float64=rel(f32))), flush=True)


if __name__ == "__main__":
    main()
