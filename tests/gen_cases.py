"""Cases of KVAE.generate shared by the CPU tier (tests/test_generate.py: host simulation, the rollout kernel on emulated
wavefronts) and the GPU tier (tests/test_gpu_generate.py): the reference fixtures of the noise-free rollout and the rollout
kernel against a restatement of the recursion written here, in fp64."""
import torch

from golden_util import load, sub


# ---------------------------------------------------------------------------------------------------------------------------
# reference fixtures (tests/golden/make_goldens_generate.py)
# ---------------------------------------------------------------------------------------------------------------------------
def vae_weights(model, seed):
    """The fixture script's seeded frame-VAE weights (make_goldens_generate.py: vae_weights), repeated."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith(("encoder.", "decoder.")):
                fan_in = p[0].numel() if p.dim() > 1 else 64
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / fan_in ** 0.5)


def golden_model(name):
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    g = load(name)
    model = KVAE(KVAEConfig(dynamics_model="lstm", num_modes=int(g["K"]), scheduled_beta=False))
    vae_weights(model, int(g["vae_seed"]))
    sd = model.state_dict()
    for k, v in sub(g, "vae_sum.").items():
        assert abs(float(sd[k].double().sum()) - float(v)) <= 1e-9 * max(1.0, abs(float(v))), k
    res = model.load_state_dict(sub(g, "sd."), strict=False)
    assert not res.unexpected_keys and all(k.startswith(("encoder.", "decoder.")) for k in res.missing_keys)
    return model, g


def golden_generate(name, dev):
    """Noise-free KVAE.generate vs the reference's impute with the tail hidden: a and alpha <= 1e-4, frames <= 1e-3."""
    from kvae import noise
    model, g = golden_model(name)
    model.to(dev).eval()
    T0, H = int(g["T0"]), int(g["H"])
    u = g["u"].to(dev) if "u" in g else None
    with noise.inject(eps_a=g["eps_a"].reshape(-1, g["eps_a"].shape[-1])):
        out = model.generate(g["x"].to(dev), H, num_samples=1, u=u, noise=False)
    assert out["a"].shape == (2, 1, H, 2) and out["x"].shape == (2, 1, H, 1, 32, 32)
    assert (out["a_vae"].cpu() - g["a_vae"]).abs().max() < 1e-5
    assert (out["a"][:, 0].cpu() - g["a_tail"]).abs().max() <= 1e-4
    assert (out["weights"][:, 0].cpu() - g["state_probs_tail"]).abs().max() <= 1e-4
    assert (out["x"][:, 0].cpu() - g["x_tail"]).abs().max() <= 1e-3
    assert not model.training
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the rollout against a restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _spd_chol(*lead, n, g, scale):
    M = torch.randn(*lead, n, n, generator=g, dtype=torch.float64)
    return torch.linalg.cholesky(scale * (M @ M.mT / n + 0.5 * torch.eye(n, dtype=torch.float64))).float()


def random_problem(kind, K, n, m, p, B, S, H, hidden=50, seed=0, with_noise=True, with_u=True, p_stay=0.8):
    """Inputs of lgssm_ops.rollout (host fp32 tensors)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g)
    pr = dict(kind=kind, A=torch.eye(n).repeat(K, 1, 1) + rn(K, n, n, sc=0.15), Bm=rn(K, n, m, sc=0.3), Cm=rn(K, p, n, sc=0.5),
              mu=rn(B, n), L0=_spd_chol(B, n=n, g=g, scale=0.3), U=rn(B, H, m, sc=0.5) if with_u else None,
              LR=_spd_chol(n=p, g=g, scale=0.05), S=S, H=H)
    if kind == "switching":
        pr["LQ"] = _spd_chol(K, n=n, g=g, scale=0.05)
        P = torch.full((K, K), (1 - p_stay) / max(K - 1, 1))
        P.fill_diagonal_(p_stay if K > 1 else 1.0)
        pr["P"] = P
        pr["s0"] = torch.nn.functional.one_hot(torch.randint(0, K, (B,), generator=g), K).float()
    else:
        pr["LQ"] = _spd_chol(n=n, g=g, scale=0.05)
        if K > 1:
            pr["lstm"] = (rn(4 * hidden, p, sc=0.4), rn(4 * hidden, hidden, sc=0.15), rn(4 * hidden, sc=0.1), rn(4 * hidden, sc=0.1),
                          rn(K, hidden, sc=1.0), rn(K, sc=0.5))
            pr.update(h0=torch.tanh(rn(B, hidden)), c0=rn(B, hidden), y0=rn(B, p))
    if with_noise:
        pr.update(eps0=rn(B, S, n), eps_z=rn(B, S, H, n), eps_a=rn(B, S, H, p))
        if kind == "switching":
            pr["gumbel"] = -torch.log(-torch.log(torch.rand(B, S, H, K, generator=g).clamp(1e-9, 1 - 1e-9)))
    return pr


def restate(pr, dtype):
    """The recursion of KVAE.generate (its docstring; include/kvae_lgssm.h), one rollout at a time with the mixed matrices
    formed explicitly, in `dtype`."""
    c = lambda t: None if t is None else t.to(dtype)
    A, Bm, Cm, mu, L0, U, LQ, LR = (c(pr.get(k)) for k in ("A", "Bm", "Cm", "mu", "L0", "U", "LQ", "LR"))
    eps0, eps_z, eps_a, gumbel = (c(pr.get(k)) for k in ("eps0", "eps_z", "eps_a", "gumbel"))
    S, H, kind = pr["S"], pr["H"], pr["kind"]
    K, n, p = A.shape[0], A.shape[1], Cm.shape[1]
    B = mu.shape[0]
    a_out = torch.zeros(B, S, H, p, dtype=dtype)
    z_out = torch.zeros(B, S, H, n, dtype=dtype)
    w_out = torch.zeros(B, S, H, K, dtype=dtype)
    lstm = tuple(c(t) for t in pr["lstm"]) if "lstm" in pr else None
    for b in range(B):
        for s in range(S):
            z = mu[b] + (L0[b] @ eps0[b, s] if eps0 is not None else 0)
            if kind == "switching":
                reg = c(pr["s0"])[b]
            elif lstm is not None:
                h, cc, y = c(pr["h0"])[b], c(pr["c0"])[b], c(pr["y0"])[b]
            for t in range(H):
                if kind == "switching":
                    pi = reg @ c(pr["P"])
                    reg = (torch.nn.functional.one_hot(torch.argmax(torch.log(pi) + gumbel[b, s, t]), K).to(dtype)
                           if gumbel is not None else pi)
                    w = reg
                elif lstm is None:
                    w = torch.ones(1, dtype=dtype)
                else:
                    w_ih, w_hh, b_ih, b_hh, hw, hb = lstm
                    gates = w_ih @ y + w_hh @ h + b_ih + b_hh
                    Hd = h.shape[0]
                    i_, f_, g_, o_ = (gates[q * Hd:(q + 1) * Hd] for q in range(4))
                    cc = torch.sigmoid(f_) * cc + torch.sigmoid(i_) * torch.tanh(g_)
                    h = torch.sigmoid(o_) * torch.tanh(cc)
                    w = torch.softmax(hw @ h + hb, 0)
                At = (w[:, None, None] * A).sum(0)
                Bt = (w[:, None, None] * Bm).sum(0)
                Ct = Cm[0] if kind == "switching" else (w[:, None, None] * Cm).sum(0)
                z = At @ z + (Bt @ U[b, t] if U is not None else 0)
                if eps_z is not None:
                    LQt = (w[:, None, None] * LQ).sum(0) if kind == "switching" else LQ
                    z = z + LQt @ eps_z[b, s, t]
                a = Ct @ z + (LR @ eps_a[b, s, t] if eps_a is not None else 0)
                y = a
                a_out[b, s, t], z_out[b, s, t], w_out[b, s, t] = a, z, w
    return a_out, z_out, w_out


def rollout_vs_restatement(dev, pr, impl="kernel"):
    """lgssm_ops.rollout on `dev` vs the fp64 restatement; bar: max(1e-4, 4 x the distance of the fp32 restatement)."""
    from kvae.kalman import lgssm_ops
    to = lambda t: t.to(dev) if isinstance(t, torch.Tensor) else (tuple(x.to(dev) for x in t) if isinstance(t, tuple) else t)
    args = {k: to(v) for k, v in pr.items()}
    kind, S, H = args.pop("kind"), args.pop("S"), args.pop("H")
    A, Bm, Cm, mu, L0, U, LQ, LR = (args.pop(k) for k in ("A", "Bm", "Cm", "mu", "L0", "U", "LQ", "LR"))
    got = lgssm_ops.rollout(kind, A, Bm, Cm, mu, L0, U, LQ, LR, S, H, impl=impl, **args)
    ref = restate(pr, torch.float64)
    f32 = restate(pr, torch.float32)
    for name, x, r, f in zip(("a", "z", "weights"), got, ref, f32):
        assert x.shape == r.shape, (name, x.shape, r.shape)
        bar = max(1e-4, 4 * float((f.double() - r).abs().max()))
        err = float((x.cpu().double() - r).abs().max())
        assert err <= bar, (name, err, bar)
    return got
