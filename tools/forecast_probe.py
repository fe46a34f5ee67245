#!/usr/bin/env python3
"""Timing of lgssm_ops.switching_forecast at one shape per invocation: the kernels (kvae_lgssm_switching_forecast: the filter's
sweep with its history kept, the forecast over B T (sequence, origin) items, the sequence sums) with all outputs and with
regime_fore + a_fore + log_lik_fore alone, against the torch restatement on the same device (lgssm_ops.switching_forecast_torch)
and against what the package offered before this call existed: one masked switching_filter call per origin over T + H steps (its
tail hidden), timed on three origins and SCALED to T - it covers the moments only, a hidden step stores log_lik = 0.
HIP-event times, median of `iters` calls after warm-up (the restatement: median of 2 after a warm-up call at H = 2; one call
where B T H exceeds 2e6).  forecast_ms is the forecast launch alone,
by difference: the call with the forecast outputs only minus the call with the filter's state only (the forward launch alone).
us_per_item_step is forecast_ms over B T H next to the filter's time per (sequence, step) from the same process.  One shape per
process, so that a caller can put every shape under its own time limit:
usage: python tools/forecast_probe.py B,T,K,H [iters]   shapes of DESIGN.md section 19: 32,100,7  256,50,3  512,200,7 at H = 10, 50"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd"), str(ROOT / "tools")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from switching_filter_probe import DEV, M, inputs, med_ms  # noqa: E402


def med_ms_few(fn, warm, reps):
    """The median of `reps` calls of the restatement after `warm` (the same call at two horizons: the restatement itself runs for
    minutes at the largest shape)."""
    warm()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    B, T, K, H = (int(v) for v in sys.argv[1].split(","))
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    args = inputs(B, T, K)
    g = torch.Generator().manual_seed(B + T + K + H)
    U_all = torch.cat([args[9], torch.randn(B, H, M, generator=g).to(DEV)], 1)
    a9 = args[:9]
    lean = ("regime_fore", "a_fore", "log_lik_fore")
    run = lambda **kw: lgssm_ops.switching_forecast(*a9, U_all, H, **kw)
    all_ms = med_ms(lambda: run(impl="hip"), iters)
    lean_ms = med_ms(lambda: run(want=lean, impl="hip"), iters)
    fore_ms = med_ms(lambda: run(want=lgssm_ops._SWH_FORE, impl="hip"), iters)
    fwd_ms = med_ms(lambda: run(want=("state",), impl="hip"), iters)
    filt_ms = med_ms(lambda: lgssm_ops.switching_filter(*args, impl="hip"), iters)
    reps = 2 if B * T * H <= 2000000 else 1
    t_ms = med_ms_few(lambda: run(impl="torch"), lambda: lgssm_ops.switching_forecast(*a9, U_all[:, :T + 2], 2, impl="torch"), reps)
    # before this call: one masked filter call per origin over T + H steps
    Y_ext = torch.cat([args[8], torch.zeros(B, H, 2, device=DEV)], 1)
    want = ("regime_pred", "a_pred", "S", "mus_filt", "Sigmas_filt")

    def masked(t):
        hide = torch.zeros(B, T + H, device=DEV)
        hide[:, :t + 1] = 1.0
        return lgssm_ops.switching_filter(*args[:8], Y_ext, U_all, mask=hide, want=want, impl="hip")

    origins = (0, T // 2, T - 1)
    per_origin = statistics.median(med_ms(lambda t=t: masked(t), max(3, iters // 4)) for t in origins)
    ker = run(impl="hip")
    ref = lgssm_ops.switching_forecast_torch(*(a.double().cpu() for a in a9), U_all.double().cpu(), H, want=("a_fore", "log_lik_fore")) \
        if B * T * H <= 200000 else None
    diff = None if ref is None else {k: float((ker[k].double().cpu() - ref[k]).abs().max()) for k in ("a_fore", "log_lik_fore")}
    launch = max(fore_ms - fwd_ms, 0.0)
    print(json.dumps(dict(B=B, T=T, K=K, H=H, n=4, m=M, call_ms=round(all_ms, 4), lean_call_ms=round(lean_ms, 4),
                          forecast_outputs_only_ms=round(fore_ms, 4), forward_only_ms=round(fwd_ms, 4), forecast_ms=round(launch, 4),
                          us_per_item_step=round(1e3 * launch / (B * T * H), 5), filter_ms=round(filt_ms, 4),
                          filter_us_per_seq_step=round(1e3 * filt_ms / (B * T), 5), torch_ms=round(t_ms, 3), torch_calls=reps,
                          speedup_vs_torch=round(t_ms / all_ms, 1), masked_filter_ms_per_origin=round(per_origin, 4),
                          masked_filter_ms_scaled_to_T=round(per_origin * T, 2), origins_timed=list(origins),
                          max_abs_vs_float64=diff)), flush=True)


if __name__ == "__main__":
    main()
