#!/usr/bin/env python3
"""Timing of lgssm_ops.predictive (kvae_lgssm_predictive: the item launch + the sequence sums) against the torch restatement on
the device (lgssm_ops.predictive_torch), all outputs requested, at four shapes, and of KVAE.score and
KVAE.log_likelihood(num_samples=16) end to end.  HIP-event times: the median of `iters` single calls after warm-up (launch
overheads included), and `b2b_ms`, one event pair around 50 back-to-back calls over 50 (what the two kernels take when the queue
is kept full).  bytes_per_item counts what the algorithm must move: reads 4 (n^2 + n + p n + p + 1), writes 4 (p + p^2 + 2) + 4;
hbm_fraction = items x bytes_per_item / b2b time over the 8 TB/s peak of the HBM.
usage: python tools/predictive_probe.py [iters] [out.txt]   (default out: profiles/r07_predictive_probe.txt)"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "kalman-vae_amd")]
import torch  # noqa: E402

from kvae.kalman import lgssm_ops  # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "r07_predictive_probe.txt"
DEV = "cuda"
HBM_BYTES_PER_S = 8e12
# (name, rows, T, n, C per step out of a packed record?)
SHAPES = [("lstm K=3 B=256 T=50 n=4", 256, 50, 4, True), ("switching K=7 B=32 T=100 n=4", 32, 100, 4, False),
          ("z=u=16 B=512 T=200", 512, 200, 16, True), ("lstm K=3 B=256 T=50 n=4, 16 samples per sequence", 4096, 50, 4, True)]


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


def b2b_ms(fn, reps=50):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def kernel_rows(emit):
    p = 2
    for name, B, T, n, per_step in SHAPES:
        g = torch.Generator().manual_seed(1000 * B + 10 * T + n)
        M = torch.randn(B, T, n, n, generator=g)
        Sp = (M @ M.mT / n + 0.5 * torch.eye(n)).to(DEV)
        mp, Y = torch.randn(B, T, n, generator=g).to(DEV), torch.randn(B, T, p, generator=g).to(DEV)
        R = (0.03 ** 2 * torch.eye(p)).to(DEV)
        mask = (torch.rand(B, T, generator=g) > 0.2).float().to(DEV)
        if per_step:   # the lstm record A | B | C of one step
            E = n * n + n * n + p * n
            packed = torch.randn(B, T, E, generator=g).to(DEV)
            slots = lgssm_ops.Slots(C=2 * n * n)
            Cm = packed[..., 2 * n * n:].unflatten(-1, (p, n))
        else:
            packed, slots, Cm = None, lgssm_ops.Slots(), torch.randn(p, n, generator=g).to(DEV)
        kern = lambda: lgssm_ops.predictive(mp, Sp, Cm, R, Y, mask, packed=packed, slots=slots, impl="kernel")
        tor = lambda: lgssm_ops.predictive(mp, Sp, Cm, R, Y, mask, packed=packed, slots=slots, impl="torch")
        k_ms, k_b2b, t_ms = med_ms(kern), b2b_ms(kern), med_ms(tor, max(3, ITERS // 2))
        ker, ref = kern(), lgssm_ops.predictive_torch(mp.double(), Sp.double(), Cm.double(), R.double(), Y.double(), mask.double())
        diff = {k: float(((ker[k].double() - ref[k]).abs() / ref[k].abs().clamp_min(1.0)).max()) for k in ("ll", "nis", "a_pred", "S")}
        items = B * T
        bpi = 4 * (n * n + n + p * n + p + 1) + 4 * (p + p * p + 2) + 4
        emit(dict(shape=name, items=items, kernel_ms=round(k_ms, 4), b2b_ms=round(k_b2b, 4), torch_ms=round(t_ms, 3),
                  speedup=round(t_ms / k_ms, 1), bytes_per_item=bpi, gbytes_per_s_b2b=round(items * bpi / (k_b2b * 1e-3) / 1e9, 1),
                  hbm_fraction=round(items * bpi / (k_b2b * 1e-3) / HBM_BYTES_PER_S, 4), max_ratio_vs_float64=diff))


def model_rows(emit):
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    for name, kind, K, B, T in (("lstm K=3 B=256 T=50", "lstm", 3, 256, 50), ("switching K=7 B=32 T=100", "switching", 7, 32, 100)):
        torch.manual_seed(0)
        model = KVAE(KVAEConfig(dynamics_model=kind, num_modes=K, scheduled_beta=False)).to(DEV).eval()
        x = (torch.rand(B, T, 1, 32, 32) > 0.7).float().to(DEV)
        mask = torch.ones(B, T, device=DEV)
        mask[:, T // 3:T // 2] = 0
        emit(dict(model=name, score_ms=round(med_ms(lambda: model.score(x, mask=mask)), 3),
                  score_decode_ms=round(med_ms(lambda: model.score(x, mask=mask, decode=True)), 3),
                  forward_ms=round(med_ms(lambda: model(x, mask=mask)), 3),
                  log_likelihood_16_ms=round(med_ms(lambda: model.log_likelihood(x, num_samples=16, mask=mask), max(3, ITERS // 2)), 3)))


def main():
    assert torch.cuda.is_available(), "predictive_probe needs a HIP device: nothing here is a CPU measurement"
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    kernel_rows(emit)
    with torch.no_grad():
        model_rows(emit)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text("# tools/predictive_probe.py %d  (%s)\n" % (ITERS, torch.cuda.get_device_name(0)) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
