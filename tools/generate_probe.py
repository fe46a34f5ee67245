#!/usr/bin/env python3
"""Timing of KVAE.generate at three shapes: the rollout kernel alone (kvae_lgssm_generate), the torch rollout path on the same
inputs (lgssm_ops.rollout_torch), and end-to-end `generate` with decoding (encode + conditioning filter + draws + rollout +
decoder).  HIP-event times, median of `iters` calls after warm-up.  The f32 fraction is the rollout's useful FLOPs over the
kernel time against the MI355X vector / matrix f32 peak (157.3 TFLOP/s).
usage: python tools/generate_probe.py [iters]"""
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
PEAK_F32 = 157.3e12
T0 = 10
SHAPES = [dict(name="lstm_K3", kind="lstm", K=3, z=4, B=256, S=16, H=50),
          dict(name="switching_K7", kind="switching", K=7, z=4, B=32, S=64, H=100),
          dict(name="lstm_K3_z16", kind="lstm", K=3, z=16, B=512, S=4, H=200)]


def med_ms(fn, iters=ITERS):
    for _ in range(2):
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


def flops_per_step(kind, K, n, m, p, hidden=50):
    f = 2 * K * (n * n + n * m) + 2 * n * n   # mixing-free state update (sum_k w_k A_k z, B_k u) + process noise
    f += 2 * (K if kind == "lstm" else 1) * p * n + 2 * p * p
    if kind == "lstm" and K > 1:
        f += 2 * 4 * hidden * (p + hidden + 1) + 2 * K * hidden + 4 * K   # cell + head + softmax
    else:
        f += 2 * K * K   # regime step
    return f


def main():
    torch.manual_seed(0)
    rows = []
    for sh in SHAPES:
        cfg = KVAEConfig(dynamics_model=sh["kind"], num_modes=sh["K"], z_dim=sh["z"], scheduled_beta=False)
        model = KVAE(cfg).to(DEV).eval()
        with torch.no_grad():
            model.kalman_filter.dyn_params.A.add_(0.05 * torch.randn_like(model.kalman_filter.dyn_params.A))
        B, S, H, n, m, p, K = sh["B"], sh["S"], sh["H"], sh["z"], cfg.u_dim, cfg.a_dim, sh["K"]
        x = (torch.rand(B, T0, 1, 32, 32, device=DEV) > 0.7).float()
        # the rollout's operands, as generate builds them
        with torch.no_grad():
            a_vae, _, _ = model.encode_sequence(x)
            hand = model.kalman_filter.condition(a_vae, torch.zeros(B, T0, m, device=DEV))
        kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
        args = dict(eps0=torch.randn(B, S, n, device=DEV), eps_z=torch.randn(B, S, H, n, device=DEV),
                    eps_a=torch.randn(B, S, H, p, device=DEV))
        if sh["kind"] == "switching":
            args.update(P=dyn._prior_matrix(DEV, torch.float32), s0=hand["s"],
                        gumbel=-torch.empty(B, S, H, K, device=DEV).exponential_().log())
            LQ = lgssm_ops.safe_cholesky(dyn.Q.detach())
        else:
            lstm = dyn.lstm
            args.update(lstm=tuple(t.detach() for t in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
                                                       dyn.head_w.weight, dyn.head_w.bias)), h0=hand["h"], c0=hand["c"], y0=hand["y"])
            LQ = lgssm_ops.safe_cholesky(kf.Q)
        ops = (sh["kind"], dyn.A.detach(), dyn.B.detach(), dyn.C.detach(), hand["mu"], lgssm_ops.safe_cholesky(hand["Sigma"]),
               torch.randn(B, H, m, device=DEV), LQ, lgssm_ops.safe_cholesky(kf.R), S, H)
        with torch.no_grad():
            k_ms = med_ms(lambda: lgssm_ops.rollout(*ops, impl="kernel", **args))
            t_ms = med_ms(lambda: lgssm_ops.rollout(*ops, impl="torch", **args), iters=max(3, ITERS // 3))
            ka = lgssm_ops.rollout(*ops, impl="kernel", **args)
            ta = lgssm_ops.rollout(*ops, impl="torch", **args)
            diff = max(float((u - v).abs().max() / v.abs().max().clamp_min(1e-30)) for u, v in zip(ka, ta))
            e_ms = med_ms(lambda: model.generate(x, H, num_samples=S), iters=max(3, ITERS // 2))
        R = B * S
        fl = flops_per_step(sh["kind"], K, n, m, p) * R * H
        row = dict(shape=sh["name"], B=B, S=S, H=H, R=R, K=K, n=n, kernel_ms=round(k_ms, 4), torch_rollout_ms=round(t_ms, 3),
                   speedup=round(t_ms / k_ms, 1), generate_e2e_ms=round(e_ms, 3), gflop=round(fl / 1e9, 3),
                   f32_fraction=round(fl / (k_ms * 1e-3) / PEAK_F32, 4), max_rel_kernel_vs_torch=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
