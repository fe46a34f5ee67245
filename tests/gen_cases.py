"""Cases of KVAE.generate shared by the CPU tier (tests/test_generate.py: host simulation, the rollout kernel on emulated
wavefronts) and the GPU tier (tests/test_gpu_generate.py): the reference fixtures of the noise-free rollout and the rollout
kernel against a restatement of the recursion written here, in fp64 - as whole tensors (rollout_vs_restatement) and one
(rollout, step) at a time with guards, sentinels and isolation (rollout_per_step; bars GEN_STEP_TOL = 4 x the float32 yardstick)."""
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


# ---------------------------------------------------------------------------------------------------------------------------
# the rollout kernel (csrc/lgssm_gen.h) one (rollout, step) at a time
# ---------------------------------------------------------------------------------------------------------------------------
# Bars = 4 x YARDSTICK, where the yardstick of a quantity is the largest per-(rollout, step) ratio (parity_cases._per_step_ratio,
# rollouts flattened to [B*S, H, d]) of the FLOAT32 run of the restatement above against its float64 run, over GEN_CASES and
# GEN_LARGE_CASES (rerun: gen_yardstick()).  Families = the kernel's dispatches: lstm4 = (n, m) (4, 4), lstm16 = (16, 16),
# rt = run-time dimensions, sw = switching.  Kernel ratios against the same float64 runs: DESIGN section 2.
GEN_YARDSTICK = {   # float32 restatement against its float64 run, largest per-(rollout, step) ratio over both case lists
    "lstm4.a": 2.35e-06, "lstm4.z": 4.05e-07, "lstm4.weights": 7.22e-07, "lstm16.a": 6.42e-06, "lstm16.z": 1.35e-06, "lstm16.weights": 4.37e-06,
    "rt.a": 6.25e-06, "rt.z": 1.88e-06, "rt.weights": 5.72e-07, "sw.a": 1.06e-05, "sw.z": 6.28e-07, "sw.weights": 4.82e-07,
}
GEN_STEP_TOL = {k: 4.0 * v for k, v in GEN_YARDSTICK.items()}
GEN_GUARD = -7.25e33     # what the guard records and every output element hold before the call
GEN_PAD = 8              # guard records in front of and behind each output: the rollouts of one wavefront
GEN_HARD_GAP = 1e-3      # least top-two gap of log pi + g in the float64 run: a hard draw's regime is then compared exactly
GEN_NOISE = {"none": (), "eps0": ("eps0",), "eps_z": ("eps_z",), "eps_a": ("eps_a",), "gumbel": ("gumbel",),
             "all": ("eps0", "eps_z", "eps_a", "gumbel")}
_PER_SEQ = ("mu", "L0", "U", "h0", "c0", "y0", "s0", "eps0", "eps_z", "eps_a", "gumbel")


def gen_family(kind, n, m):
    return "sw" if kind == "switching" else {(4, 4): "lstm4", (16, 16): "lstm16"}.get((n, m), "rt")


def keep_noise(pr, noise):
    """The problem with only the noise buffers of GEN_NOISE[noise] (the others NULL: their terms drop out)."""
    keep = GEN_NOISE[noise]
    return {k: v for k, v in pr.items() if k not in GEN_NOISE["all"] or k in keep}


def restate_vec(pr, dtype, gaps=False):
    """restate() with the rollouts of a sequence side by side (z [B,S,n]); test_restate_vec_is_restate pins it to the scalar form
    at 1e-12 in float64.  gaps=True: also the smallest top-two gap of log pi + g over every hard draw (inf without one)."""
    c = lambda t: None if t is None else t.to(dtype)
    A, Bm, Cm, mu, L0, U, LQ, LR = (c(pr.get(k)) for k in ("A", "Bm", "Cm", "mu", "L0", "U", "LQ", "LR"))
    eps0, eps_z, eps_a, gumbel = (c(pr.get(k)) for k in ("eps0", "eps_z", "eps_a", "gumbel"))
    S, H, kind = pr["S"], pr["H"], pr["kind"]
    K, B = A.shape[0], mu.shape[0]
    lstm = tuple(c(t) for t in pr["lstm"]) if "lstm" in pr else None
    mv = lambda M, v: torch.einsum("...ij,...j->...i", M, v)
    z = mu[:, None].expand(B, S, -1)
    if eps0 is not None:
        z = z + mv(L0[:, None], eps0)
    if kind == "switching":
        reg = c(pr["s0"])[:, None].expand(B, S, K)
    elif lstm is not None:
        h, cc, y = (c(pr[k])[:, None].expand(B, S, -1) for k in ("h0", "c0", "y0"))
    a_out, z_out, w_out, gap = [], [], [], float("inf")
    for t in range(H):
        if kind == "switching":
            pi = reg @ c(pr["P"])
            if gumbel is not None:
                sc = torch.log(pi) + gumbel[:, :, t]
                if K > 1:
                    top = sc.topk(2, -1).values
                    gap = min(gap, float((top[..., 0] - top[..., 1]).min()))
                reg = torch.nn.functional.one_hot(sc.argmax(-1), K).to(dtype)
            else:
                reg = pi
            w = reg
        elif lstm is None:
            w = torch.ones(B, S, 1, dtype=dtype)
        else:
            w_ih, w_hh, b_ih, b_hh, hw, hb = lstm
            i_, f_, g_, o_ = (y @ w_ih.T + h @ w_hh.T + b_ih + b_hh).chunk(4, -1)
            cc = torch.sigmoid(f_) * cc + torch.sigmoid(i_) * torch.tanh(g_)
            h = torch.sigmoid(o_) * torch.tanh(cc)
            w = torch.softmax(h @ hw.T + hb, -1)
        mix = lambda M: torch.einsum("bsk,kij->bsij", w, M)
        z = mv(mix(A), z)
        if U is not None:
            z = z + mv(mix(Bm), U[:, None, t])
        if eps_z is not None:
            z = z + mv(mix(LQ) if kind == "switching" else LQ, eps_z[:, :, t])
        a = mv(Cm[0] if kind == "switching" else mix(Cm), z)
        if eps_a is not None:
            a = a + mv(LR, eps_a[:, :, t])
        y = a
        a_out.append(a), z_out.append(z), w_out.append(w)
    out = tuple(torch.stack(v, 2) for v in (a_out, z_out, w_out))
    return out + (gap,) if gaps else out


def _gen_reference(pr, dtype):
    """The scalar restatement where it is quick, its side-by-side form (pinned to it) at thousands of rollouts."""
    return restate(pr, dtype) if pr["mu"].shape[0] * pr["S"] <= 64 else restate_vec(pr, dtype)[:3]


def rollout_raw(dev, pr):
    """kvae_lgssm_generate through the loaded library, the problem built as lgssm_ops.rollout builds it, each of a, z, weights
    [R,H,d] with a guard in front and one behind (GEN_PAD records [H,d] each: what one wavefront could store) and every element
    holding GEN_GUARD before the call: afterwards both guards must be untouched (the ragged last wavefront stores nothing for
    r0 + r >= R) and no element may keep the sentinel.  Returns CPU tensors a [B,S,H,p], z [B,S,H,n], weights [B,S,H,K]."""
    import ctypes as C
    from kvae import _native as N
    from kvae.kalman.lgssm_ops import _f32c
    A, Bm, Cm, mu = pr["A"], pr["Bm"], pr["Cm"], pr["mu"]
    K, n, m, p, B, S, H = A.shape[0], A.shape[1], Bm.shape[2], Cm.shape[1], mu.shape[0], pr["S"], pr["H"]
    g = N.GenProblem()
    g.B, g.S, g.H, g.n, g.m, g.p, g.K = B, S, H, n, m, p, K
    g.kind = 1 if pr["kind"] == "switching" else 0
    named = {("C" if k == "Cm" else k): pr.get(k) for k in ("A", "Bm", "Cm", "LQ", "LR", "P") + _PER_SEQ}
    if "lstm" in pr:
        named.update(zip(("w_ih", "w_hh", "b_ih", "b_hh", "head_w", "head_b"), pr["lstm"]))
        g.hidden = pr["lstm"][1].shape[1]
    keep = {k: _f32c(t.detach().to(dev)) for k, t in named.items() if t is not None}
    for k, t in keep.items():
        setattr(g, k, t.data_ptr())
    R = B * S
    flats = {k: torch.full(((R + 2 * GEN_PAD) * H * d,), GEN_GUARD, device=dev, dtype=torch.float32) for k, d in (("a", p), ("z", n), ("weights", K))}
    g.a_out, g.z_out, g.w_out = (flats[k].data_ptr() + 4 * GEN_PAD * H * d for k, d in (("a", p), ("z", n), ("weights", K)))
    lib = N.lib_for(keep["mu"])
    before = lib.dll.kvae_wemu_generate_launches() if dev == "cpu" else None
    lib.check(lib.dll.kvae_lgssm_generate(C.byref(g), N.stream_for(keep["mu"])), "kvae_lgssm_generate")
    if dev == "cpu":
        assert lib.dll.kvae_wemu_generate_launches() == before + 1, "the emulated rollout kernel is not what ran"
    out = []
    for k, d in (("a", p), ("z", n), ("weights", K)):
        flat, rec = flats[k].cpu(), H * d
        assert bool((flat[:GEN_PAD * rec] == GEN_GUARD).all()), (k, "the guard in front was written")
        assert bool((flat[-GEN_PAD * rec:] == GEN_GUARD).all()), (k, "the guard behind was written")
        body = flat[GEN_PAD * rec:-GEN_PAD * rec].view(R, rec)
        left = (body == GEN_GUARD).any(-1).nonzero().flatten().tolist()
        assert not left, (k, "not overwritten at rollout", left[:4])
        out.append(body.reshape(B, S, H, d).clone())
    return tuple(out)


def redraw_sequence(pr, b, seed=977):
    """The problem with everything that belongs to sequence b alone drawn again (hand-over state, controls, noise)."""
    g = torch.Generator().manual_seed(seed + b)
    out = dict(pr)
    for k in _PER_SEQ:
        if pr.get(k) is None:
            continue
        t = pr[k].clone()
        if k == "L0":
            t[b] = _spd_chol(n=t.shape[-1], g=g, scale=0.3)
        elif k == "s0":
            t[b] = t[b].roll(1, -1)   # another one-hot start (the same one at K = 1)
        elif k == "gumbel":
            t[b] = -torch.log(-torch.log(torch.rand(t[b].shape, generator=g).clamp(1e-9, 1 - 1e-9)))
        else:
            t[b] = torch.randn(t[b].shape, generator=g)
        out[k] = t
    return out


def rollout_per_step(dev, pr, isolate=(), yardstick=False):
    """The rollout kernel on `dev` (rollout_raw: guards and sentinels) against the float64 restatement of exactly the float32
    operand values, one (rollout, step) at a time: a, z, weights under GEN_STEP_TOL.  Hard Gumbel draws: the float64 run must
    keep a top-two gap of log pi + g above GEN_HARD_GAP at every (rollout, step) - then the regimes are equal and the weights
    exactly one-hot.  K = 1 (lstm): weights exactly 1.  Soft switching: the rows of weights sum to 1 within the bar.
    isolate: sequences whose own inputs are drawn again in turn - every output of every other sequence must keep its bits.
    yardstick=True: no kernel, the float32 restatement's ratios instead.  Returns {family.quantity: largest ratio}."""
    from parity_cases import _per_step_ratio
    kind, S, H = pr["kind"], pr["S"], pr["H"]
    K, n, m, B = pr["A"].shape[0], pr["A"].shape[1], pr["Bm"].shape[2], pr["mu"].shape[0]
    fam = gen_family(kind, n, m)
    hard = kind == "switching" and pr.get("gumbel") is not None
    ref = _gen_reference(pr, torch.float64)
    if hard:
        gap = restate_vec(pr, torch.float64, gaps=True)[3]
        assert gap > GEN_HARD_GAP, ("a hard draw of the float64 run is too close to call: another seed", gap)
        w = ref[2]
        assert bool(((w == 0) | (w == 1)).all()) and bool((w.sum(-1) == 1).all())
    got = _gen_reference(pr, torch.float32) if yardstick else rollout_raw(dev, pr)
    out = {}
    for name, x, r in zip(("a", "z", "weights"), got, ref):
        assert x.shape == r.shape and x.dtype == torch.float32, (name, x.shape, r.shape)
        assert bool(torch.isfinite(x).all()), name
        key = "%s.%s" % (fam, name)
        if name == "weights" and (hard or K == 1):
            assert yardstick or torch.equal(x.double(), r), (key, "regimes differ" if hard else "weights of K = 1 are not 1")
            continue
        ratio, where = _per_step_ratio(x.reshape(B * S, H, -1), r.reshape(B * S, H, -1))
        out[key] = ratio
        assert yardstick or ratio < GEN_STEP_TOL[key], (key, ratio, where, GEN_STEP_TOL[key])
    if kind == "switching" and not hard and not yardstick:
        off = float((got[2].double().sum(-1) - 1).abs().max())
        assert off < GEN_STEP_TOL["sw.weights"], ("rows of soft weights do not sum to 1", off)
    if not yardstick:
        for b in isolate:
            other = rollout_raw(dev, redraw_sequence(pr, b))
            rest = [q for q in range(B) if q != b]
            for name, x, y in zip(("a", "z", "weights"), got, other):
                assert torch.equal(x[rest], y[rest]), (name, "another sequence changed with sequence", b)
            assert not torch.equal(got[1][b], other[1][b]), ("the redraw of sequence %d changed nothing" % b)
    return out


def _gen_case(i, kind, n, m, K, B, S, H=None, seed=None):
    """Options rotate with the index: p (2 for the cell; 1, 3, 16 else), H, controls, noise subset.  Isolation: the first, the
    middle and the last sequence of a small case; the middle one of the 7 x 439 (both its boundaries lie inside a wavefront)."""
    cell = kind == "lstm" and K > 1
    isolate = sorted({0, B // 2, B - 1}) if 1 < B and B * S <= 64 else ([B // 2] if B * S == 3073 else [])
    noises = ("none", "eps0", "eps_z", "eps_a", "all") if kind == "lstm" else ("none", "eps0", "gumbel", "eps_a", "all")
    return dict(kind=kind, n=n, m=m, K=K, p=2 if cell else (1, 3, 16)[i % 3], B=B, S=S, H=(1, 2, 3, 8)[(i // 2) % 4] if H is None else H,
                with_u=i % 2 == 0, noise=noises[i % 5], isolate=isolate, seed=100 + i if seed is None else seed)


GEN_DISPATCHES = [("lstm", 4, 4), ("lstm", 16, 16), ("lstm", 5, 3), ("lstm", 4, 2), ("lstm", 16, 3), ("lstm", 3, 16), ("lstm", 1, 1),
                  ("switching", 4, 4), ("switching", 4, 2), ("switching", 16, 16), ("switching", 7, 5)]
GEN_BS = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (3, 3), (5, 1), (3, 7)]
GEN_CASES = [_gen_case(11 * j + d, kind, n, m, (1, 2, 3, 16)[(j + d) % 4], *GEN_BS[(11 * j + d) % 9])
             for j in range(4) for d, (kind, n, m) in enumerate(GEN_DISPATCHES)]
# R = 3072: the last size with 4 rollouts per wavefront; R = 3073 = 7 x 439: 8 per wavefront, ragged, sequence boundaries inside.
# (Seed 246: the one hard-draw case of this size, 6146 draws over 16 regimes - of the seeds 200 ... 259 it is the one whose
# smallest float64 gap, 1.8e-3, clears GEN_HARD_GAP with the most room; the case asserts the gap, so another seed fails, not skips.)
GEN_LARGE_CASES = [_gen_case(7 * d + e, kind, n, m, K, B, S, H=2, seed=246 if (kind, B) == ("switching", 7) else None)
                   for d, (kind, n, m, K) in enumerate([("lstm", 4, 4, 3), ("lstm", 16, 16, 2), ("lstm", 5, 3, 3), ("switching", 4, 2, 16)])
                   for e, (B, S) in enumerate([(4, 768), (7, 439)])] + [_gen_case(4, "lstm", 3, 16, 1, 7, 439, H=2)]


def gen_case_id(c):
    return "%s_n%dm%dp%d_K%d_B%dS%dH%d_%s_%s" % (c["kind"][:2], c["n"], c["m"], c["p"], c["K"], c["B"], c["S"], c["H"],
                                                  "u" if c["with_u"] else "nou", c["noise"])


def gen_case_problem(c):
    pr = random_problem(c["kind"], c["K"], c["n"], c["m"], c["p"], c["B"], c["S"], c["H"], seed=c["seed"], with_u=c["with_u"])
    return keep_noise(pr, c["noise"])


def run_gen_case(dev, c, **kw):
    return rollout_per_step(dev, gen_case_problem(c), isolate=c["isolate"], **kw)


def gen_yardstick():
    """GEN_YARDSTICK, measured again: the float32 restatement over both case lists."""
    out = {}
    for c in GEN_CASES + GEN_LARGE_CASES:
        for k, v in run_gen_case("cpu", c, yardstick=True).items():
            out[k] = max(out.get(k, 0.0), v)
    return out
