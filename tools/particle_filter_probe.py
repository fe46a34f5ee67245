#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_pf at one shape per invocation: the kernels (kvae_lgssm_switching_pf: one launch for the sweep,
one for the lineages, one for the sequence sums) against the torch restatement on the same device (lgssm_ops.switching_pf_torch:
T steps of about forty small launches), all outputs requested, and the kernels with the log-likelihood and the regime beliefs
alone.  HIP-event times, median of `iters` calls after warm-up (the restatement: median of 2).  `us_per_step` is the kernel time
over T: the work is a T-deep dependent chain per replicate, one workgroup of N particles each.  One shape per process, so that a
caller can put every shape under its own time limit:
usage: python tools/particle_filter_probe.py B,T,K,N,G [iters]    shapes of DESIGN.md section 18: 32,100,7,256,4  256,50,3,64,1  512,200,7,256,1"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd"), str(ROOT / "tools")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from switching_filter_probe import DEV, inputs, med_ms  # noqa: E402


def med_ms_torch(fn, warm):
    """The median of 2 calls of the restatement, after `warm` (the same call on two steps: the restatement itself runs for a minute
    at the largest shape)."""
    warm()
    torch.cuda.synchronize()
    ts = []
    for _ in range(2):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    B, T, K, N, G = (int(v) for v in sys.argv[1].split(","))
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    args = inputs(B, T, K)
    g = torch.Generator().manual_seed(B + T + K + N + G)
    th, ph = torch.rand(B, G, T, N, generator=g).to(DEV), torch.rand(B, G, T, generator=g).to(DEV)
    lean = ("log_lik", "log_lik_seq", "regime_filt")
    run = lambda **kw: lgssm_ops.switching_pf(*args, th, ph, ess_threshold=0.5, **kw)
    k_ms = med_ms(lambda: run(impl="hip"), iters)
    l_ms = med_ms(lambda: run(want=lean, impl="hip"), iters)
    f_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, want=lean, impl="hip"), iters)
    short = args[:8] + (args[8][:, :2], args[9][:, :2])
    t_ms = med_ms_torch(lambda: run(impl="torch"),
                        lambda: lgssm_ops.switching_pf(*short, th[:, :, :2], ph[:, :, :2], ess_threshold=0.5, impl="torch"))
    ker = run(impl="hip")
    print(json.dumps(dict(B=B, T=T, K=K, N=N, G=G, n=4, m=4, kernel_ms=round(k_ms, 4), kernel_loglik_regimes_ms=round(l_ms, 4),
                          torch_ms=round(t_ms, 3), speedup=round(t_ms / k_ms, 1), us_per_step=round(1e3 * k_ms / T, 3),
                          gpb2_filter_ms=round(f_ms, 4), gpb2_us_per_step=round(1e3 * f_ms / T, 3),
                          resampled_share=round(float(ker["resampled"].float().mean()), 3), ess_mean=round(float(ker["ess"].mean()), 1))),
          flush=True)


if __name__ == "__main__":
    main()
