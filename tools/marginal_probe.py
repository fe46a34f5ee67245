"""python tools/marginal_probe.py: the numbers of DESIGN.md section 13, one JSON line each (needs an MI355X).
1. kvae_lgssm_predictive (both launches) and kvae_lgssm_predictive_bwd alone at (B,T,n) = (256,50,4) and (512,200,16), C_t and gC
   in the product's packed step record: five windows of 300 back-to-back calls under one HIP event pair each, microseconds per call;
   the adjoint's algorithmic bytes (reads + writes per item, from the shapes) over its best window, and that rate over 8 TB/s.
2. The full captured train step (Trainer, hipGraph, side stream) at bench.py's c2 and c4 presets with kf_objective="elbo" and
   "marginal", two trainers on models of the same seed, three windows of 300 steps each, alternating; host clock around a
   synchronise, milliseconds per step."""
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "kalman-vae_amd")):
    sys.path.insert(0, p)
import torch

import bench
from kvae import _native as N
from kvae.train.synthetic import bouncing_ball
from kvae.train.train import Trainer

dev = torch.device("cuda:0")


def kernel(B, T, n, iters=300):
    p, m = 2, n
    g = torch.Generator().manual_seed(1)
    M = torch.randn(B, T, n, n, generator=g)
    Sp = (M @ M.mT / n + 0.5 * torch.eye(n)).to(dev).contiguous()
    mp = torch.randn(B, T, n, generator=g).to(dev)
    E = n * n + n * m + p * n
    rec = torch.randn(B, T, E, generator=g).to(dev)
    off = n * n + n * m
    R = (0.03 ** 2 * torch.eye(p)).to(dev)
    Y = torch.randn(B, T, p, generator=g).to(dev)
    g_ll, g_seq = torch.randn(B, T, generator=g).to(dev), torch.randn(B, generator=g).to(dev)
    pr = N.PredProblem()
    pr.B, pr.T, pr.n, pr.p = B, T, n, p
    pr.mus_pred, pr.Sigmas_pred, pr.R, pr.y = mp.data_ptr(), Sp.data_ptr(), R.data_ptr(), Y.data_ptr()
    pr.C = N.Stack(rec.data_ptr() + 4 * off, T * E, E)
    ll, seq, lv = torch.empty(B, T, device=dev), torch.empty(B, device=dev), torch.empty(B, T, device=dev, dtype=torch.int32)
    pr.ll, pr.seq_ll, pr.levels = ll.data_ptr(), seq.data_ptr(), lv.data_ptr()
    gr = N.PredGrads()
    g_mp, g_Sp, gY, grec = torch.empty_like(mp), torch.empty_like(Sp), torch.empty_like(Y), torch.zeros_like(rec)
    gr.g_ll, gr.g_seq = g_ll.data_ptr(), g_seq.data_ptr()
    gr.g_mus_pred, gr.g_Sigmas_pred, gr.gY = g_mp.data_ptr(), g_Sp.data_ptr(), gY.data_ptr()
    gr.gC = N.Stack(grec.data_ptr() + 4 * off, T * E, E)
    lib = N.hip_lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd = lambda: lib.dll.kvae_lgssm_predictive(C.byref(pr), s)
    bwd = lambda: lib.dll.kvae_lgssm_predictive_bwd(C.byref(pr), C.byref(gr), s)
    out = {"shape": [B, T, n]}
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        for _ in range(20):
            assert fn() == 0
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / iters)
        out[name + "_us"] = [round(t, 2) for t in times]
    assert int(lv.abs().max()) == 0 and bool(torch.isfinite(g_Sp).all())
    items = B * T
    rd = n * n + n + p * n + p + 1
    wr = n * n + n + p * n + p
    out["bwd_bytes"] = 4 * items * (rd + wr)
    out["bwd_bytes_written"] = 4 * items * wr
    best = min(out["bwd_us"])
    out["bwd_GBps"] = round(out["bwd_bytes"] / best / 1e3, 1)
    out["bwd_hbm_fraction"] = round(out["bwd_bytes"] / (best * 1e-6) / (bench.HBM_PEAK_GBS * 1e9), 4)
    return out


def step_ab(preset, steps, windows=3):
    a = bench.parse_args(["--config", preset])
    for k, v in bench.PRESETS[preset].items():
        if getattr(a, k.replace("-", "_"), None) is None:
            setattr(a, k, v)
    x = bouncing_ball(a.batch, a.seq_len, 1234).float().to(dev)
    tr, out = {}, {"preset": preset, "steps_per_window": steps}
    for obj in ("elbo", "marginal"):
        _, model = bench.build_model(a, dev)
        model.to(dev).train()
        tr[obj] = Trainer(model, lr=1e-3, use_graph=True, reference_logging=True, kf_objective=obj)
        for _ in range(5):
            o = tr[obj].step(x)
        torch.cuda.synchronize()
        out[obj + "_loss"] = float(o["loss"])
        out[obj + "_elbo_kf"] = float(o["elbo_kf"])
        out[obj + "_captures"] = tr[obj].captures
        out[obj + "_ms"] = []
    for _ in range(windows):
        for obj in ("elbo", "marginal"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr[obj].step(x)
            torch.cuda.synchronize()
            out[obj + "_ms"].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    return out


assert torch.cuda.is_available(), "marginal_probe needs a HIP device: nothing here is measured without one"
for shp in ((256, 50, 4), (512, 200, 16)):
    r = kernel(*shp)
    print(json.dumps(r), flush=True)
for preset, steps in (("c2", 300), ("c4", 300)):
    r = step_ab(preset, steps)
    print(json.dumps(r), flush=True)
