#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_filter at one shape per invocation: the kernel (kvae_lgssm_switching_filter: one launch for the
sweep, one for the sequence sums) against the torch restatement on the same device (lgssm_ops.switching_filter_torch: T steps of
about thirty small launches), all outputs requested, and the kernel with the regime beliefs and the log-likelihood alone.
HIP-event times, median of `iters` calls after warm-up.  `us_per_step` is the kernel time over T: the work is a T-deep dependent
chain per sequence, one wavefront each.  One shape per process, so that a caller can put every shape under its own time limit:
usage: python tools/switching_filter_probe.py B,T,K [iters]        shapes of DESIGN.md section 14: 32,100,7  256,50,3  512,200,7"""
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from kvae.kalman.switch_dyn_param import StickyRegimePrior  # noqa: E402

DEV = "cuda"
N, M = 4, 4


def med_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def inputs(B, T, K):
    """Rotations of different angle and sign scaled by <= 0.97, Q_k of different size, moderate observation noise; Y is noise of
    the model's scale (the time does not depend on the data)."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + K)
    A = torch.zeros(K, N, N)
    for k in range(K):
        th, sc = (0.15 + 0.25 * k) * (1.0 if k % 2 == 0 else -1.0), 0.97 - 0.03 * k
        for o, f in ((0, 1.0), (2, -0.7)):
            c, s = math.cos(f * th), math.sin(f * th)
            A[k, o:o + 2, o:o + 2] = sc * torch.tensor([[c, -s], [s, c]])
    Bm = 0.3 * torch.randn(K, N, M, generator=g)
    Q = torch.stack([(0.02 + 0.015 * k) * torch.eye(N) for k in range(K)])
    Cm, R = 0.8 * torch.randn(2, N, generator=g), 0.05 * torch.eye(2)
    P = StickyRegimePrior(K, 0.8).transition_matrix
    Y, U = torch.randn(B, T, 2, generator=g), torch.randn(B, T, M, generator=g)
    return tuple(t.to(DEV) for t in (A, Bm, Q, Cm, R, P, torch.zeros(N), 0.5 * torch.eye(N), Y, U))


def main():
    B, T, K = (int(v) for v in sys.argv[1].split(","))
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    args = inputs(B, T, K)
    lean = ("regime_filt", "log_lik", "log_lik_seq")
    k_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, impl="hip"), iters)
    l_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, want=lean, impl="hip"), iters)
    t_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, impl="torch"), max(2, iters // 10))
    ker = lgssm_ops.switching_filter(*args, impl="hip")
    ref = lgssm_ops.switching_filter_torch(*(a.double().cpu() for a in args))
    diff = {k: float((ker[k].double().cpu() - ref[k]).abs().max()) for k in ("regime_filt", "log_lik", "log_lik_seq", "mus_filt")}
    print(json.dumps(dict(B=B, T=T, K=K, n=N, m=M, kernel_ms=round(k_ms, 4), kernel_regimes_loglik_ms=round(l_ms, 4),
                          torch_ms=round(t_ms, 3), speedup=round(t_ms / k_ms, 1), us_per_step=round(1e3 * k_ms / T, 3),
                          max_abs_vs_float64=diff)), flush=True)


if __name__ == "__main__":
    main()
