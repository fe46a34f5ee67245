#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_log_marginal, one JSON line per invocation (needs an MI355X).
usage: python tools/regime_marginal_probe.py B,T,K [iters]      one shape: 32,100,7  256,50,3  512,200,7 (n = m = 4)
         forward + backward of the op - seq_ll.sum().backward() with every operand differentiated: kvae_lgssm_switching_marginal
         (two launches) and kvae_lgssm_switching_marginal_bwd (two launches) - HIP events, median of `iters` calls after warm-up;
         against float32 autograd of the restatement on the same device (lgssm_ops.switching_log_marginal_torch, median of 2), and
         next to switching_filter's own call (regimes, log-likelihood), remeasured in the same run.
       python tools/regime_marginal_probe.py step [steps]       the captured train step (Trainer, hipGraph, side stream) at
         bench.py's c4 preset (BASELINE configs[3]) under kf_objective "elbo", "marginal" and "regime_marginal": three trainers on
         models of the same seed, three alternating windows of `steps` steps, host clock around a synchronise, ms per step.
One shape per process, so that a caller can put every shape under its own time limit."""
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "kalman-vae_amd"), str(ROOT / "tools")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from switching_filter_probe import inputs, med_ms  # noqa: E402


def shape(B, T, K, iters):
    args = inputs(B, T, K)
    leaves = [a.clone().requires_grad_(i not in (4, 5)) for i, a in enumerate(args)]   # R and P are constants of the model

    def fb(impl):
        for a in leaves:
            a.grad = None
        lgssm_ops.switching_log_marginal(*leaves, impl=impl)["seq_ll"].sum().backward()

    k_ms = med_ms(lambda: fb("hip"), iters)
    with torch.no_grad():
        f_ms = med_ms(lambda: lgssm_ops.switching_log_marginal(*args, impl="hip"), iters)
        filt_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, want=("regime_filt", "log_lik", "log_lik_seq"), impl="hip"), iters)
    ts = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fb("torch")
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    t_ms = statistics.median(ts)
    ref = [a.grad.clone() for a in leaves if a.grad is not None]
    fb("hip")
    got = [a.grad for a in leaves if a.grad is not None]
    diff = max(float((g - r).abs().max() / r.abs().max().clamp_min(1.0)) for g, r in zip(got, ref))
    print(json.dumps(dict(B=B, T=T, K=K, n=4, m=4, fwd_bwd_ms=round(k_ms, 4), fwd_ms=round(f_ms, 4), bwd_ms=round(k_ms - f_ms, 4),
                          switching_filter_ms=round(filt_ms, 4), torch_autograd_ms=round(t_ms, 1), speedup=round(t_ms / k_ms, 1),
                          bwd_us_per_step=round(1e3 * (k_ms - f_ms) / T, 3), max_rel_vs_float32_autograd=diff)), flush=True)


def step(steps, windows=3):
    import bench
    from kvae.train.synthetic import bouncing_ball
    from kvae.train.train import Trainer
    dev = torch.device("cuda:0")
    a = bench.parse_args(["--config", "c4"])
    for k, v in bench.PRESETS["c4"].items():
        if getattr(a, k.replace("-", "_"), None) is None:
            setattr(a, k, v)
    x = bouncing_ball(a.batch, a.seq_len, 1234).float().to(dev)
    objectives = ("elbo", "marginal", "regime_marginal")
    tr, out = {}, {"preset": "c4", "steps_per_window": steps}
    for obj in objectives:
        _, model = bench.build_model(a, dev)
        model.to(dev).train()
        tr[obj] = Trainer(model, lr=1e-3, use_graph=True, reference_logging=True, kf_objective=obj)
        for _ in range(5):
            o = tr[obj].step(x)
        torch.cuda.synchronize()
        out[obj + "_loss"], out[obj + "_elbo_kf"], out[obj + "_captures"] = float(o["loss"]), float(o["elbo_kf"]), tr[obj].captures
        out[obj + "_ms"] = []
    for _ in range(windows):
        for obj in objectives:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr[obj].step(x)
            torch.cuda.synchronize()
            out[obj + "_ms"].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "regime_marginal_probe needs a HIP device: nothing here is measured without one"
    if sys.argv[1] == "step":
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 100)
    else:
        B, T, K = (int(v) for v in sys.argv[1].split(","))
        shape(B, T, K, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
