#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_smoother at one shape per invocation: the kernel (kvae_lgssm_switching_smoother: the forward with
its history kept, the backward, the sequence sums) with all outputs, with regime_smooth + mus_smooth alone, the filter's own call
(lgssm_ops.switching_filter, all outputs: remeasured in the same run, the figure of DESIGN.md section 14) and the torch restatement
on the same device (lgssm_ops.switching_smoother_torch).  HIP-event times, median of `iters` calls after warm-up.
`back_us_per_step` is (smoother, all outputs) - (filter, all outputs) over T: the backward pass and the history stores, against the
filter's `filter_us_per_step`.  One shape per process, so that a caller can put every shape under its own time limit:
usage: python tools/switching_smoother_probe.py B,T,K [iters]      shapes of DESIGN.md section 15: 32,100,7  256,50,3  512,200,7"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd"), str(ROOT / "tools")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from switching_filter_probe import inputs, med_ms  # noqa: E402

SMOOTH = ("regime_smooth", "regime_pairs", "mus_smooth", "Sigmas_smooth")


def main():
    B, T, K = (int(v) for v in sys.argv[1].split(","))
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    args = inputs(B, T, K)
    lean = ("regime_smooth", "mus_smooth")
    s_ms = med_ms(lambda: lgssm_ops.switching_smoother(*args, impl="hip"), iters)
    l_ms = med_ms(lambda: lgssm_ops.switching_smoother(*args, want=lean, impl="hip"), iters)
    f_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, impl="hip"), iters)
    t_ms = med_ms(lambda: lgssm_ops.switching_smoother(*args, impl="torch"), max(2, iters // 10))
    ker = lgssm_ops.switching_smoother(*args, impl="hip")
    ref = lgssm_ops.switching_smoother_torch(*(a.double().cpu() for a in args))
    diff = {k: float((ker[k].double().cpu() - ref[k]).abs().max()) for k in SMOOTH}
    print(json.dumps(dict(B=B, T=T, K=K, n=4, m=4, smoother_ms=round(s_ms, 4), smoother_regimes_mean_ms=round(l_ms, 4),
                          filter_ms=round(f_ms, 4), torch_ms=round(t_ms, 3), speedup=round(t_ms / s_ms, 1),
                          filter_us_per_step=round(1e3 * f_ms / T, 3), back_us_per_step=round(1e3 * (s_ms - f_ms) / T, 3),
                          max_abs_vs_float64=diff)), flush=True)


if __name__ == "__main__":
    main()
