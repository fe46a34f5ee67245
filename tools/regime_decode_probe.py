#!/usr/bin/env python3
"""Timing of lgssm_ops.regime_decode at three shapes: the kernel (kvae_regime_decode: one launch) against the torch restatement
on the device (lgssm_ops.regime_decode_torch: T - 1 iterations of about ten small launches), all outputs requested, and the
kernel with the marginals and KL alone (no Viterbi sweep, no backtrace).  HIP-event times, median of `iters` calls after warm-up.
`us_per_step` is the kernel time over T: the work is a T-deep dependent chain per sequence, one wavefront each.
usage: python tools/regime_decode_probe.py [iters]"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from kvae.kalman.switch_dyn_param import StickyRegimePrior  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = "cuda"
SHAPES = [(32, 100, 7), (256, 50, 3), (512, 200, 7)]   # (B, T, K): BASELINE configs[3], configs[1]-sized, the configs[4] shard


def med_ms(fn, iters=ITERS):
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


def main():
    for B, T, K in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + 10 * T + K)
        logits = torch.randn(B, T, K, K, generator=g).to(DEV)
        init = torch.randn(B, K, generator=g).to(DEV)
        P = StickyRegimePrior(K, 0.8).transition_matrix.to(DEV)
        k_ms = med_ms(lambda: lgssm_ops.regime_decode(logits, init, P, impl="kernel"))
        m_ms = med_ms(lambda: lgssm_ops.regime_decode(logits, init, P, want=("marginals", "kl"), impl="kernel"))
        t_ms = med_ms(lambda: lgssm_ops.regime_decode(logits, init, P, impl="torch"), iters=max(3, ITERS // 4))
        ker = lgssm_ops.regime_decode(logits, init, P, impl="kernel")
        ref = lgssm_ops.regime_decode_torch(logits.double(), init.double(), P.double())
        diff = {k: float((ker[k].double() - ref[k]).abs().max() / ref[k].abs().max()) for k in ("marginals", "kl", "path_logq")}
        row = dict(B=B, T=T, K=K, kernel_ms=round(k_ms, 4), kernel_marginals_kl_ms=round(m_ms, 4), torch_ms=round(t_ms, 3),
                   speedup=round(t_ms / k_ms, 1), us_per_step=round(1e3 * k_ms / T, 3),
                   paths_equal_float64=bool(torch.equal(ker["path"], ref["path"])), max_rel_vs_float64=diff)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
