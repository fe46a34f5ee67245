#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_viterbi at one shape per invocation: the kernel (kvae_lgssm_switching_viterbi: one launch - the
sweep, the backtrace and the gather of the survivor beliefs by the same wavefront) with all outputs, with path + path_log_joint
alone (no belief workspace written) and with the state alone (the sweep without any backtrace), against the torch restatement on
the same device (lgssm_ops.switching_viterbi_torch) and against switching_filter on the same inputs in the same process.  HIP-event
times, median of `iters` calls after warm-up (the restatement: median of max(2, iters // 10)).  us_per_step is the kernel time over
T: the work is a T-deep dependent chain per sequence, one wavefront each.  One shape per process, so that a caller can put every
shape under its own time limit:
usage: python tools/viterbi_probe.py B,T,K [iters]        shapes of DESIGN.md section 20: 32,100,7  256,50,3  512,200,7"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd"), str(ROOT / "tools")]
from kvae.kalman import lgssm_ops  # noqa: E402
from switching_filter_probe import M, inputs, med_ms  # noqa: E402


def main():
    B, T, K = (int(v) for v in sys.argv[1].split(","))
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    args = inputs(B, T, K)
    run = lambda **kw: lgssm_ops.switching_viterbi(*args, **kw)
    all_ms = med_ms(lambda: run(impl="hip"), iters)
    path_ms = med_ms(lambda: run(want=("path", "path_log_joint"), impl="hip"), iters)
    sweep_ms = med_ms(lambda: run(want=("state",), impl="hip"), iters)
    filt_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, impl="hip"), iters)
    filt_state_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, want=("state",), impl="hip"), iters)
    t_ms = med_ms(lambda: run(impl="torch"), max(2, iters // 10))
    ker = run(impl="hip")
    ref = lgssm_ops.switching_viterbi_torch(*(a.double().cpu() for a in args)) if B * T <= 20000 else None
    diff = None if ref is None else dict(path_log_joint=float((ker["path_log_joint"].double().cpu() - ref["path_log_joint"]).abs().max()),
                                         paths_equal=float((ker["path"].cpu() == ref["path"]).all(1).double().mean()))
    print(json.dumps(dict(B=B, T=T, K=K, n=4, m=M, kernel_ms=round(all_ms, 4), kernel_path_only_ms=round(path_ms, 4),
                          kernel_sweep_only_ms=round(sweep_ms, 4), us_per_step=round(1e3 * all_ms / T, 3),
                          sweep_us_per_step=round(1e3 * sweep_ms / T, 3), filter_ms=round(filt_ms, 4),
                          filter_sweep_only_ms=round(filt_state_ms, 4), filter_us_per_step=round(1e3 * filt_state_ms / T, 3),
                          torch_ms=round(t_ms, 3), speedup_vs_torch=round(t_ms / all_ms, 1), vs_float64=diff)), flush=True)


if __name__ == "__main__":
    main()
