#!/usr/bin/env python3
"""Timing of KVAE.sample_imputations at three shapes: the two launches of kvae_lgssm_posterior_sample separately (gains of all
B*T items | the B*S paths), the torch path on the same inputs (lgssm_ops.posterior_paths_torch) in the same process, kernel and
torch alternating, and end-to-end `sample_imputations` with decoding (encode + filter + draws + both launches + decoder).
HIP-event times, median (min .. max) of `iters` calls after warm-up.  Per launch it prints the algorithmic bytes (every operand
read once, every output written once) and their fraction of the 8 TB/s HBM figure over the measured time, and for the paths the
dependent chain (T steps, one n-term matvec each), and says which binds.
usage: python tools/posterior_probe.py [iters]"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402
from kvae.model.model import KVAE  # noqa: E402
from kvae.utils.config import KVAEConfig  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
DEV = "cuda"
HBM = 8e12
SHAPES = [dict(name="lstm_K3", kind="lstm", K=3, z=4, B=256, S=16, T=50),
          dict(name="switching_K7", kind="switching", K=7, z=4, B=32, S=64, T=100),
          dict(name="lstm_K3_z16", kind="lstm", K=3, z=16, B=512, S=4, T=200)]


def time_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def stats(ts):
    return dict(med=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def main():
    torch.manual_seed(0)
    for sh in SHAPES:
        cfg = KVAEConfig(dynamics_model=sh["kind"], num_modes=sh["K"], z_dim=sh["z"], scheduled_beta=False)
        model = KVAE(cfg).to(DEV).eval()
        with torch.no_grad():
            model.kalman_filter.dyn_params.A.add_(0.05 * torch.randn_like(model.kalman_filter.dyn_params.A))
        B, S, T, n, p = sh["B"], sh["S"], sh["T"], sh["z"], cfg.a_dim
        x = (torch.rand(B, T, 1, 32, 32, device=DEV) > 0.7).float()
        mask = torch.ones(B, T, device=DEV)
        mask[:, 4:16] = 0
        kf = model.kalman_filter
        with torch.no_grad():
            a_vae, _, _ = model.encode_sequence(x)
            kf.dyn_params.reset_state()
            post = kf.sample_posterior(a_vae, torch.zeros(B, T, cfg.u_dim, device=DEV), mask, num_samples=1, noise=False)
        mf, Sf, mp, Sp, A_l, _, C_l = post["filter"]
        Q = kf._last.transition_noise()
        eps = torch.randn(B, S, T, n, device=DEV)
        ops = dict(mus_filt=mf, Sigmas_filt=Sf, mus_pred=mp, Sigmas_pred=Sp, A=A_l, Cm=C_l, Q=Q, S=S, eps=eps)
        call = lgssm_ops.PosteriorCall(**ops)
        gains, paths, both, torch_ms = [], [], [], []
        with torch.no_grad():
            for it in range(ITERS + 2):   # kernel and torch alternate in one process; the first two rounds warm up
                g_ms = time_ms(lambda: call.run(call.GAINS))
                p_ms = time_ms(lambda: call.run(call.PATHS))
                b_ms = time_ms(lambda: call.run())
                t_ms = time_ms(lambda: lgssm_ops.posterior_paths_torch(**ops)) if it < 2 + max(3, ITERS // 3) else None
                if it >= 2:
                    gains.append(g_ms), paths.append(p_ms), both.append(b_ms)
                    if t_ms is not None:
                        torch_ms.append(t_ms)
            zt, at, _ = lgssm_ops.posterior_paths_torch(**ops)
            diff = max(float((u - v).abs().max() / v.abs().max().clamp_min(1e-30)) for u, v in ((call.z, zt), (call.a, at)))
            e2e = [time_ms(lambda: model.sample_imputations(x, mask, num_samples=S)) for _ in range(2 + max(3, ITERS // 2))][2:]
        rec = 2 * n * n + n
        per_step_q = Q.dim() == 4
        gain_bytes = 4 * B * T * (2 * n * n + n * n + (n * n if per_step_q else 0) + 2 * n + rec + 1)   # Sf, Sp, A, (Q), mf, mp | record, level
        path_bytes = 4 * (B * T * (rec + p * n) + B * S * T * (n + n + p))                            # records, C | eps, z, a
        g_med, p_med = statistics.median(gains), statistics.median(paths)
        row = dict(shape=sh["name"], B=B, S=S, T=T, n=n, items=B * T, paths=B * S,
                   gains_ms=stats(gains), paths_ms=stats(paths), both_ms=stats(both), torch_ms=stats(torch_ms),
                   speedup=round(statistics.median(torch_ms) / statistics.median(both), 1),
                   sample_imputations_e2e_ms=stats(e2e),
                   gains_bytes_per_item=gain_bytes // (B * T), gains_mb=round(gain_bytes / 1e6, 3),
                   gains_hbm_fraction=round(gain_bytes / (g_med * 1e-3) / HBM, 4),
                   paths_bytes_per_path_step=round(path_bytes / (B * S * T), 1), paths_mb=round(path_bytes / 1e6, 3),
                   paths_hbm_fraction=round(path_bytes / (p_med * 1e-3) / HBM, 4),
                   paths_chain_steps=T, paths_us_per_step=round(p_med * 1e3 / T, 3),
                   binds=dict(gains="latency of the phase chain per item (LDS + barriers); bytes are far from the HBM figure"
                              if gain_bytes / (g_med * 1e-3) / HBM < 0.3 else "HBM bytes",
                              paths="the dependent chain over T" if path_bytes / (p_med * 1e-3) / HBM < 0.3 else "HBM bytes"),
                   max_rel_kernel_vs_torch=diff)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
