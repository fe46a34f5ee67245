"""Cases of KalmanFilter.sample_posterior / KVAE.sample_imputations shared by the CPU tier (tests/test_posterior_sample.py: host
simulation, both kernels of csrc/lgssm_post.h on emulated wavefronts) and the GPU tier (tests/test_gpu_posterior_sample.py):
the reference's masked fixtures (noise-free paths = its smoother's means; moments of sampled paths = its smoother's covariances
and the lag-one cross-covariance J_t Sigma_{t+1|T}), the kernels against a restatement of the recursion written here in fp64,
the per-item Cholesky ladder, and the same kernels one gains item / one (path, step) at a time over guarded buffers
(gains_per_item, paths_per_step, ladder_per_item; bars POST_STEP_TOL = 4 x the float32 yardstick)."""
import torch

from golden_util import load, rel_err, sub

FIXTURES = [("masked_lstm_K7_B2_T100", "lstm"), ("masked_switch_K7_B2_T100", "switching")]
RUNGS = [1e-6 * 10 ** k for k in range(5)]


def make_filter(g, kind, device="cpu"):
    """Product KalmanFilter + dynamics module carrying the fixture's parameters."""
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    dyn = sub(g, "dyn.")
    K, n = dyn["A"].shape[0], dyn["A"].shape[1]
    model = KVAE(KVAEConfig(dynamics_model=kind, num_modes=K, z_dim=n))
    kf = model.kalman_filter
    res = kf.dyn_params.load_state_dict(dyn, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    kf.load_state_dict({"Q": g["Qbuf"], "R": g["R"], "mu0": g["mu0"], "Sigma0": g["Sigma0"]}, strict=False)
    if "tau" in g and hasattr(kf.dyn_params, "tau"):
        kf.dyn_params.tau = float(g["tau"])
    kf.train(bool(g["train"]))
    return kf.to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# pinned to the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------------
def golden_noise_free(name, kind, dev, S=3):
    """sample_posterior(noise=False): z = the fixture's mus_smooth and a = its a_imputed on every path (<= 1e-4, rel_err), and z =
    KalmanFilter.smooth's mus_smooth on the same device (<= 1e-4); every ladder level 0."""
    from kvae import noise
    g = load(name)
    kf = make_filter(g, kind, dev)
    a, u, mask = g["a"].to(dev), g["u"].to(dev), g["mask"].to(dev)
    kf.dyn_params.reset_state()
    with noise.inject(gumbel=g.get("gumbel")):
        out = kf.sample_posterior(a, u, mask, num_samples=S, noise=False)
        kf.dyn_params.reset_state()
        with torch.no_grad():
            ms = kf.smooth(a, u, mask=mask)[0]
    B, T, n = g["mus_smooth"].shape[:3]
    assert out["z"].shape == (B, S, T, n) and out["a"].shape == (B, S, T, 2) and out["levels"].shape == (B, T)
    assert out["levels"].dtype == torch.int32 and int(out["levels"].abs().max()) == 0
    figs = {}
    for s in range(S):
        figs["z_vs_fixture"] = rel_err(out["z"][:, s].cpu(), g["mus_smooth"].squeeze(-1))
        figs["a_vs_fixture"] = rel_err(out["a"][:, s].cpu(), g["a_imputed"])
        figs["z_vs_smooth"] = rel_err(out["z"][:, s].cpu(), ms.squeeze(-1).cpu())
        print(name, dev, s, figs)
        assert figs["z_vs_fixture"] <= 1e-4 and figs["a_vs_fixture"] <= 1e-4 and figs["z_vs_smooth"] <= 1e-4, figs
    assert len(out["filter"]) == 7 and rel_err(out["filter"][0].cpu(), g["mus_filt"]) < 1e-4
    return out


def fixture_stacks(g):
    """The fixture's own filter stacks as the arguments of lgssm_ops.posterior_paths."""
    return dict(mus_filt=g["mus_filt"].squeeze(-1), Sigmas_filt=g["Sigmas_filt"], mus_pred=g["mus_pred"].squeeze(-1),
                Sigmas_pred=g["Sigmas_pred"], A=g["A_list"], Cm=g["C_list"], Q=g["Q_seq"] if "Q_seq" in g else g["Qbuf"])


def moment_errors(z, g):
    """Largest deviation, in standard errors, of the sample mean / covariance / lag-one cross-covariance of the paths z [B,S,T,n]
    from the reference smoother's mus_smooth / Sigmas_smooth / J_t Sigma_{t+1|T} (J_t recomputed in fp64 from the fixture).
    s.e. of a mean: sqrt(Sigma_ii / S); of a second moment: sqrt((C_ij^2 + V_ii V'_jj) / (S - 1))."""
    z = z.double().cpu()
    S = z.shape[1]
    mu, Sig = g["mus_smooth"].squeeze(-1).double(), g["Sigmas_smooth"].double()
    Sf, Sp, A = g["Sigmas_filt"].double(), g["Sigmas_pred"].double(), g["A_list"].double()
    J = Sf[:, :-1] @ A[:, 1:].mT @ torch.linalg.inv(Sp[:, 1:])
    lag = J @ Sig[:, 1:]
    var = Sig.diagonal(dim1=-2, dim2=-1)
    mean = z.mean(1)
    d = z - mean[:, None]
    cov = torch.einsum("bsti,bstj->btij", d, d) / (S - 1)
    lagc = torch.einsum("bsti,bstj->btij", d[:, :, :-1], d[:, :, 1:]) / (S - 1)
    e_mean = ((mean - mu).abs() / (var / S).sqrt()).max()
    e_cov = ((cov - Sig).abs() / ((Sig ** 2 + var[..., :, None] * var[..., None, :]) / (S - 1)).sqrt()).max()
    e_lag = ((lagc - lag).abs() / ((lag ** 2 + var[:, :-1, :, None] * var[:, 1:, None, :]) / (S - 1)).sqrt()).max()
    return float(e_mean), float(e_cov), float(e_lag)


def golden_moments(name, dev, S=8192, seed=1, impl="kernel"):
    """Paths sampled over the fixture's own filter stacks with draws from a CPU generator: every moment within 5 s.e."""
    from kvae.kalman import lgssm_ops
    g = load(name)
    B, T, n = g["mus_smooth"].shape[:3]
    eps = torch.randn(B, S, T, n, generator=torch.Generator().manual_seed(seed))
    st = {k: v.to(dev) for k, v in fixture_stacks(g).items()}
    z, a, levels = lgssm_ops.posterior_paths(S=S, eps=eps.to(dev), impl=impl, **st)
    assert int(levels.abs().max()) == 0
    errs = moment_errors(z, g)
    print(name, dev, impl, "mean / cov / lag (s.e.):", errs)
    return errs


# ---------------------------------------------------------------------------------------------------------------------------
# against a restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _spd(*lead, n, g, scale):
    M = torch.randn(*lead, n, n, generator=g, dtype=torch.float64)
    return scale * (M @ M.mT / n + 0.5 * torch.eye(n, dtype=torch.float64))


def random_problem(n, p, B, S, T, seed=0, per_step_Q=True, with_noise=True, emission_noise=False, shared_ac=False, rescaled=False):
    """Inputs of lgssm_ops.posterior_paths (host fp32 tensors): SPD filter stacks from a plain fp64 filter over random
    time-varying A, C with the middle third of the steps hidden.  shared_ac: one [n,n] A and one [p,n] C for every step.
    rescaled: the same filter in the coordinates z' = D z, D = diag(logspace(-1, 1, n)) in seeded random order (Sigma' =
    D Sigma D for both covariance stacks and Q, A' = D A D^-1, C' = C D^-1, mu' = D mu) - still the output of a consistent
    filter, with rows of Sigma_{t+1|t} a factor 100 apart: the solve exchanges rows."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    A = 0.9 * eye + rn(B, T, n, n, sc=0.15)
    C = rn(B, T, p, n, sc=0.5)
    if shared_ac:
        A, C = A[0, 0].expand(B, T, n, n), C[0, 0].expand(B, T, p, n)
    Q = _spd(B, T, n=n, g=g, scale=0.05) if per_step_Q else _spd(n=n, g=g, scale=0.05)
    R = _spd(n=p, g=g, scale=0.05)
    Y = rn(B, T, p)
    hidden = [T // 3 <= t < max(2 * T // 3, T // 3 + (T > 2)) for t in range(T)]
    mu, Sig = rn(B, n, sc=0.5), _spd(B, n=n, g=g, scale=0.5)
    mf, Sf, mp, Sp = [], [], [], []
    for t in range(T):
        Qt = Q[:, t] if per_step_Q else Q
        mu_p = (A[:, t] @ mu.unsqueeze(-1)).squeeze(-1)
        Sig_p = A[:, t] @ Sig @ A[:, t].mT + Qt
        if hidden[t]:
            mu, Sig = mu_p, Sig_p
        else:
            Ct = C[:, t]
            Kt = Sig_p @ Ct.mT @ torch.linalg.inv(Ct @ Sig_p @ Ct.mT + R)
            mu = mu_p + (Kt @ (Y[:, t] - (Ct @ mu_p.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1)).squeeze(-1)
            G = eye - Kt @ Ct
            Sig = G @ Sig_p @ G.mT + Kt @ R @ Kt.mT
        Sig = 0.5 * (Sig + Sig.mT)
        mf.append(mu), Sf.append(Sig), mp.append(mu_p), Sp.append(0.5 * (Sig_p + Sig_p.mT))
    st = lambda v: torch.stack(v, 1)
    mf, Sf, mp, Sp = st(mf), st(Sf), st(mp), st(Sp)
    if rescaled:
        d = torch.logspace(-1, 1, n, dtype=torch.float64)[torch.randperm(n, generator=torch.Generator().manual_seed(seed + 7919))]
        two = lambda M: d[:, None] * M * d[None, :]
        mf, mp, Sf, Sp, Q, A, C = mf * d, mp * d, two(Sf), two(Sp), two(Q), d[:, None] * A / d[None, :], C / d[None, :]
    if shared_ac:
        A, C = A[0, 0], C[0, 0]
    pr = dict(mus_filt=mf.float(), Sigmas_filt=Sf.float(), mus_pred=mp.float(), Sigmas_pred=Sp.float(), A=A.float().contiguous(),
              Cm=C.float().contiguous(), Q=Q.float(), S=S)
    if with_noise:
        pr["eps"] = torch.randn(B, S, T, n, generator=g)
    if emission_noise:
        pr["eta"] = torch.randn(B, S, T, p, generator=g)
        pr["LR"] = torch.linalg.cholesky(R).float()
    return pr


def item_ladder(P):
    """(L, level, smallest eigenvalue) of one symmetrised P: the per-item _safe_cholesky ladder."""
    P = 0.5 * (P + P.mT)
    eye = torch.eye(P.shape[-1], dtype=P.dtype)
    lam = float(torch.linalg.eigvalsh(P.double())[0])
    jitter = 1e-6
    for lv in range(5):
        L, info = torch.linalg.cholesky_ex(P + (jitter * eye.float()).to(P.dtype))   # the jitter enters through an fp32 eye()
        if int(info) == 0:
            return L, lv, lam
        jitter *= 10.0
    return torch.diag(P.diagonal().clamp(min=1e-6).sqrt()), 5, lam


def restate_gains(pr, dtype):
    """The gains of every (b, t), written plainly in `dtype`: J [B,T,n,n] (0 at T-1), L = the ladder's factor of P_t, c = mu_{t|t} -
    J_t mu_{t+1|t} (mu_{T-1|T-1} at T-1), the levels and the smallest eigenvalue of every P_t."""
    c = lambda t: None if t is None else t.to(dtype)
    mf, Sf, mp, Sp, A, Q = (c(pr[k]) for k in ("mus_filt", "Sigmas_filt", "mus_pred", "Sigmas_pred", "A", "Q"))
    B, T, n = mf.shape
    at = lambda M, b, t: M if M.dim() == 2 else M[b, t]
    eye = torch.eye(n, dtype=dtype)
    J, L, cc = torch.zeros(B, T, n, n, dtype=dtype), torch.zeros(B, T, n, n, dtype=dtype), torch.zeros(B, T, n, dtype=dtype)
    levels, lam = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, T, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            if t == T - 1:
                P = Sf[b, t]
                cc[b, t] = mf[b, t]
            else:
                An = at(A, b, t + 1)
                J[b, t] = torch.linalg.solve(Sp[b, t + 1].T, (Sf[b, t] @ An.T).T).T
                G = eye - J[b, t] @ An
                P = G @ Sf[b, t] @ G.T + J[b, t] @ at(Q, b, t + 1) @ J[b, t].T
                cc[b, t] = mf[b, t] - J[b, t] @ mp[b, t + 1]
            L[b, t], lv, lam[b, t] = item_ladder(P)
            levels[b, t] = lv
    return J, L, cc, levels, lam


def restate(pr, dtype):
    """The recursion of KVAE.sample_imputations (its docstring; include/kvae_lgssm.h), written plainly: the gains of every (b, t),
    then one path at a time, in `dtype`.  Returns z, a, levels and the smallest eigenvalue of every P_t."""
    c = lambda t: None if t is None else t.to(dtype)
    mf, mp, C = (c(pr[k]) for k in ("mus_filt", "mus_pred", "Cm"))
    eps, eta, LR = c(pr.get("eps")), c(pr.get("eta")), c(pr.get("LR"))
    S = pr["S"]
    B, T, n = mf.shape
    p = C.shape[-2]
    at = lambda M, b, t: M if M.dim() == 2 else M[b, t]
    z_out, a_out = torch.zeros(B, S, T, n, dtype=dtype), torch.zeros(B, S, T, p, dtype=dtype)
    J, L, _, levels, lam = restate_gains(pr, dtype)
    for b in range(B):
        for s in range(S):
            z = None
            for t in range(T - 1, -1, -1):
                z = mf[b, t] if t == T - 1 else mf[b, t] + J[b, t] @ (z - mp[b, t + 1])
                if eps is not None:
                    z = z + L[b, t] @ eps[b, s, t]
                a = at(C, b, t) @ z
                if eta is not None:
                    a = a + LR @ eta[b, s, t]
                z_out[b, s, t], a_out[b, s, t] = z, a
    return z_out, a_out, levels, lam


def restate_paths_vec(pr, dtype, gains=None):
    """restate() with every path side by side (z [B,S,n]), over restate_gains; test_restate_paths_vec_is_restate pins it to the
    scalar form at 1e-12 in float64.  Returns z, a."""
    c = lambda t: None if t is None else t.to(dtype)
    mf, mp, C = (c(pr[k]) for k in ("mus_filt", "mus_pred", "Cm"))
    eps, eta, LR = c(pr.get("eps")), c(pr.get("eta")), c(pr.get("LR"))
    B, T, n = mf.shape
    J, L = (restate_gains(pr, dtype) if gains is None else gains)[:2]
    mv = lambda M, v: torch.einsum("b...ij,b...j->b...i", M, v)
    zs, z = [None] * T, None
    for t in range(T - 1, -1, -1):
        z = mf[:, None, t].expand(B, pr["S"], n) if t == T - 1 else mf[:, None, t] + mv(J[:, None, t], z - mp[:, None, t + 1])
        if eps is not None:
            z = z + mv(L[:, None, t], eps[:, :, t])
        zs[t] = z
    z = torch.stack(zs, 2)
    return z, emit(pr, z, dtype)


def emit(pr, z, dtype):
    """a = C_t z + L_R eta in `dtype` for given paths z [B,S,T,n]: the emission as a function of z alone."""
    C = pr["Cm"].to(dtype)
    a = torch.einsum("pn,bstn->bstp", C, z.to(dtype)) if C.dim() == 2 else torch.einsum("btpn,bstn->bstp", C, z.to(dtype))
    if pr.get("eta") is not None:
        a = a + torch.einsum("pq,bstq->bstp", pr["LR"].to(dtype), pr["eta"].to(dtype))
    return a


def run_paths(dev, pr, impl="kernel", **kw):
    from kvae.kalman import lgssm_ops
    args = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in pr.items()}
    return lgssm_ops.posterior_paths(impl=impl, **args, **kw)


def paths_vs_restatement(dev, pr, impl="kernel", got=None, want_levels=None):
    """lgssm_ops.posterior_paths on `dev` vs the fp64 restatement; bar per output: max(1e-4, 4 x the distance of the fp32
    restatement); ladder levels equal to the restatement's."""
    got = run_paths(dev, pr, impl) if got is None else got
    ref = restate(pr, torch.float64)
    f32 = restate(pr, torch.float32)
    for name, x, r, f in zip(("z", "a"), got[:2], ref[:2], f32[:2]):
        assert x.shape == r.shape, (name, x.shape, r.shape)
        assert bool(torch.isfinite(x).all()), name
        bar = max(1e-4, 4 * float((f.double() - r).abs().max()))
        err = float((x.cpu().double() - r).abs().max())
        assert err <= bar, (name, err, bar)
    assert got[2].dtype == torch.int32 and torch.equal(got[2].cpu(), ref[2]), (got[2].cpu(), ref[2])
    if want_levels is not None:
        assert sorted(set(ref[2].flatten().tolist())) == sorted(want_levels), ref[2]
    return got, ref


def pack_record(pr, pad=3):
    """The same problem with A | C | Q of every step in ONE packed record [B,T,E] (E padded): (record, Slots)."""
    from kvae.kalman.lgssm_ops import Slots
    B, T, n = pr["mus_filt"].shape
    p = pr["Cm"].shape[-2]
    Q = pr["Q"] if pr["Q"].dim() == 4 else pr["Q"].expand(B, T, n, n)
    rec = torch.cat([torch.zeros(B, T, pad), pr["A"].flatten(2), pr["Cm"].flatten(2), Q.flatten(2), torch.zeros(B, T, 1)], -1).contiguous()
    return rec, Slots(A=pad, C=pad + n * n, Q=pad + n * n + p * n)


# ---------------------------------------------------------------------------------------------------------------------------
# the ladder
# ---------------------------------------------------------------------------------------------------------------------------
def ladder_problem(n=4, B=4, T=5, seed=5, targets=((0, 4, -3.16e-5), (1, 4, -3.16e-4), (2, 1, -3.16e-3), (3, 2, -1.0), (1, 0, -3.16e-5))):
    """A random problem whose Sigma_{t|t} at the steps (b, t) of `targets` gets one negative eigenvalue, tuned (a secant iteration
    on the fp64 restatement) so that the smallest eigenvalue of P_t is the target: -3.16e-5, -3.16e-4, -3.16e-3 -> levels 2, 3, 4; -1 ->
    the clamped diagonal (5).  Q > 0 and Sigma_{t+1|t} are untouched, so every solve stays regular."""
    pr = random_problem(n, 2, B, 3, T, seed=seed, per_step_Q=True)

    def lam_of(b, t, Sf):
        Sf = Sf.double()
        if t == T - 1:
            P = Sf
        else:
            An, Sp, Q = pr["A"][b, t + 1].double(), pr["Sigmas_pred"][b, t + 1].double(), pr["Q"][b, t + 1].double()
            J = torch.linalg.solve(Sp.T, (Sf @ An.T).T).T
            G = torch.eye(n, dtype=torch.float64) - J @ An
            P = G @ Sf @ G.T + J @ Q @ J.T
        return float(torch.linalg.eigvalsh(0.5 * (P + P.T))[0])

    for b, t, target in targets:
        base = pr["Sigmas_filt"][b, t].double()
        w, V = torch.linalg.eigh(base)
        v = V[:, 0]
        shifted = lambda d: (base - (w[0] + d) * torch.outer(v, v)).float()   # smallest eigenvalue of Sigma_{t|t} becomes -d
        d = -target
        for _ in range(30):
            lam = lam_of(b, t, shifted(d))
            if abs(lam - target) <= 0.02 * abs(target):
                break
            d = d * target / lam if lam < 0 else d * 2.0
        pr["Sigmas_filt"][b, t] = shifted(d)
    return pr, targets


def check_ladder(dev, impl="kernel"):
    pr, targets = ladder_problem()
    got, ref = paths_vs_restatement(dev, pr, impl, want_levels=[0, 2, 3, 4, 5])
    lam = ref[3]
    want = {-3.16e-5: 2, -3.16e-4: 3, -3.16e-3: 4, -1.0: 5}
    for b, t, target in targets:
        assert int(ref[2][b, t]) == want[target], (b, t, target, int(ref[2][b, t]), float(lam[b, t]))
    for b in range(lam.shape[0]):      # every item a factor 3 away from every rung: fp32 rounding cannot move it to a neighbour
        for t in range(lam.shape[1]):
            if lam[b, t] < 0:
                assert all(-lam[b, t] >= 3 * r or -lam[b, t] <= r / 3 for r in RUNGS), (b, t, float(lam[b, t]))
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
def small_model(kind="lstm", K=3, **kw):
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    torch.manual_seed(0)
    m = KVAE(KVAEConfig(dynamics_model=kind, num_modes=K, scheduled_beta=False, **kw))
    with torch.no_grad():
        m.kalman_filter.dyn_params.A.add_(0.05 * torch.randn_like(m.kalman_filter.dyn_params.A))
    return m


def model_vs_impute(dev, kind, B=2, T=12):
    """sample_imputations(noise=False) path 0 vs KVAE.impute: frames <= 1e-3, a <= 1e-4 apart."""
    from kvae import noise
    model = small_model(kind).to(dev).eval()
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, T, 1, 32, 32, generator=g) > 0.7).float().to(dev)
    mask = torch.ones(B, T)
    mask[:, 3:8] = 0
    mask = mask.to(dev)
    nz = dict(eps_a=torch.randn(B * T, 2, generator=g).to(dev), gumbel=(-torch.empty(B, T, 3).exponential_(generator=g).log()).to(dev))
    with noise.inject(**nz):
        imp = model.impute(x, mask)
    with noise.inject(**nz):
        out = model.sample_imputations(x, mask, num_samples=1, noise=False)
    assert out["x"].shape == (B, 1, T, 1, 32, 32) and out["a"].shape == (B, 1, T, 2) and out["z"].shape == (B, 1, T, 4)
    da = float((out["a"][:, 0] - imp["a_imputed"]).abs().max())
    dx = float((out["x"][:, 0] - imp["x_imputed"]).abs().max())
    print(kind, dev, "a", da, "frames", dx)
    assert da <= 1e-4 and dx <= 1e-3, (da, dx)
    assert torch.equal(out["a_vae"], imp["a_vae"])
    if kind == "switching":
        assert torch.equal(out["state_probs"], imp["state_probs"])


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels of csrc/lgssm_post.h one item / one (path, step) at a time
# ---------------------------------------------------------------------------------------------------------------------------
# Bars = 4 x YARDSTICK, where the yardstick of a quantity is the largest per-slice ratio (parity_cases._per_step_ratio; J, L, c per
# (b, t), z and a per (path, step) with the paths flattened to [B*S, T, d]) of the FLOAT32 run of the restatement above against
# its float64 run, over the case lists below (rerun: post_yardstick()).  Families = the gains kernels: n4, n16, rt (run-time n).
# "emit": a against C_t z + L_R eta evaluated on the SAME z (the kernel's own z_out; the float32 restatement's for the yardstick).
# ".lv": the items whose ladder level is raised (L) and the (path, step)s downstream of one (z, a), where the yardstick differs
# from level 0 by more than 2 x.  Kernel ratios against the same float64 runs: DESIGN section 2.
# (a ".lv" yardstick within 2 x of its level-0 one is folded into it: n16.z, rt.z.)
POST_YARDSTICK = {   # float32 restatement against its float64 run, largest per-slice ratio over every case list
    "n4.J": 8.31e-06, "n4.L": 2.20e-07, "n4.L.lv": 2.68e-06, "n4.c": 5.42e-06, "n4.z": 2.41e-05, "n4.z.lv": 1.25e-06, "n4.a": 1.58e-05,
    "n4.a.lv": 2.72e-06, "n4.emit": 1.06e-06,
    "n16.J": 2.83e-05, "n16.L": 9.71e-07, "n16.L.lv": 1.10e-05, "n16.c": 2.28e-05, "n16.z": 1.72e-05, "n16.a": 8.49e-05, "n16.a.lv": 6.88e-06,
    "n16.emit": 7.32e-06,
    "rt.J": 1.97e-05, "rt.L": 2.56e-07, "rt.L.lv": 3.65e-05, "rt.c": 1.36e-05, "rt.z": 6.89e-06, "rt.a": 1.89e-05, "rt.a.lv": 8.30e-06,
    "rt.emit": 1.96e-06,
}
POST_STEP_TOL = {k: 4.0 * v for k, v in POST_YARDSTICK.items()}
POST_GUARD = -7.25e33    # what the guard records and every output element hold before the call
POST_LEVEL_GUARD = -77   # ... and every level


def post_family(n):
    return {4: "n4", 16: "n16"}.get(n, "rt")


def _post_bar(key, raised):
    return POST_STEP_TOL[key + ".lv"] if raised and key + ".lv" in POST_STEP_TOL else POST_STEP_TOL[key]


def _off16(t, floats):
    """First index of a flat float32 buffer whose address is `floats` floats past a 16-byte boundary."""
    return ((16 - t.data_ptr() % 16) % 16) // 4 + floats


def _misaligned(t, dev):
    """A copy of t on `dev` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=dev, dtype=t.dtype)
    o = _off16(buf, 1)
    v = buf[o:o + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


class GuardedCall:
    """lgssm_ops.PosteriorCall over `pr` on `dev` with ws, levels, z and a in buffers of the test: one guard record in front of
    each and one behind (ws: one item's J | L | c; z, a: one path's [T,d]; levels: 4), everything filled with a sentinel.
    misalign: "ws" puts the workspace, "eps" the draws 4 bytes past a 16-byte boundary (the paths then take the scalar-load
    kernel).  check(written) asserts the guards untouched, every element of the buffers named overwritten, the others untouched."""

    def __init__(self, dev, pr, misalign=None):
        from kvae.kalman import lgssm_ops
        args = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in pr.items()}
        if misalign == "eps":
            args["eps"] = _misaligned(args["eps"], dev)
        self.call = call = lgssm_ops.PosteriorCall(**args)
        assert misalign != "eps" or call.noise["eps"].data_ptr() % 16 == 4
        B, T, n = pr["mus_filt"].shape
        S, p = pr["S"], pr["Cm"].shape[-2]
        self.dims = (B, S, T, n, p)
        self.recs = dict(ws=(B * T, 2 * n * n + n), z=(B * S, T * n), a=(B * S, T * p))
        self.flat, self.view = {}, {}
        for k, (rows, rec) in self.recs.items():
            flat = torch.full(((rows + 2) * rec + 8,), POST_GUARD, device=dev, dtype=torch.float32)
            o = _off16(flat, 1 if misalign == k else 0) + rec
            self.flat[k], self.view[k] = flat, flat[o:o + rows * rec]
        self.lv_flat = torch.full((B * T + 8,), POST_LEVEL_GUARD, device=dev, dtype=torch.int32)
        call.ws, call.z, call.a = self.view["ws"], self.view["z"].view(B, S, T, n), self.view["a"].view(B, S, T, p)
        call.levels = self.lv_flat[4:4 + B * T].view(B, T)
        call.pr.ws, call.pr.z_out, call.pr.a_out, call.pr.levels_out = (t.data_ptr() for t in (call.ws, call.z, call.a, call.levels))
        assert call.ws.data_ptr() % 16 == (4 if misalign == "ws" else 0) or (n not in (4, 16) and misalign is None)

    def run(self, stages=0):
        lib = self.call.lib
        before = lib.dll.kvae_wemu_posterior_launches() if not self.call.ws.is_cuda else None
        self.call.run(stages)
        if before is not None:
            assert lib.dll.kvae_wemu_posterior_launches() == before + 1, "the emulated kernels are not what ran"
        return self

    def check(self, written):
        """Guards untouched; the buffers named in `written` hold no sentinel any more, the others nothing else."""
        for k, (rows, rec) in self.recs.items():
            flat, view = self.flat[k].cpu(), self.view[k].cpu()
            o = (self.view[k].data_ptr() - self.flat[k].data_ptr()) // 4
            assert bool((flat[:o] == POST_GUARD).all()), (k, "the guard record in front was written")
            assert bool((flat[o + rows * rec:] == POST_GUARD).all()), (k, "the guard record behind was written")
            if k in written:
                left = (view.view(rows, rec) == POST_GUARD).any(-1).nonzero().flatten().tolist()
                assert not left, (k, "not overwritten at record", left[:4])
            else:
                assert bool((view == POST_GUARD).all()), (k, "written by a stage that does not own it")
        lv = self.lv_flat.cpu()
        assert bool((lv[:4] == POST_LEVEL_GUARD).all()) and bool((lv[-4:] == POST_LEVEL_GUARD).all()), "a level guard was written"
        keeps = lv[4:-4] == POST_LEVEL_GUARD
        assert not bool(keeps.any()) if "levels" in written else bool(keeps.all()), "levels"

    def gains(self):
        B, S, T, n, p = self.dims
        rec = self.call.ws.cpu().view(B, T, 2 * n * n + n)
        return rec[..., :n * n].reshape(B, T, n, n), rec[..., n * n:2 * n * n].reshape(B, T, n, n), rec[..., 2 * n * n:], self.call.levels.cpu()


def _ratios(got, ref):
    """The per-slice ratios of parity_cases._per_step_ratio as a [B,T] tensor (asserted to have its maximum)."""
    from parity_cases import _per_step_ratio
    B, T = ref.shape[:2]
    err = (got.double() - ref).abs().reshape(B, T, -1).amax(-1)
    scale = ref.abs().reshape(B, T, -1).amax(-1).clamp_min(1e-2 * float(ref.abs().max())).clamp_min(1e-30)
    r = err / scale
    assert float(r.max()) == _per_step_ratio(got, ref)[0]
    return r


def _compare(key, got, ref, raised, out, yardstick):
    """Per-slice ratios of one stack, the slices of `raised` ([B,T] bool) under the key's .lv bar and recorded under it."""
    r = _ratios(got, ref)
    for name, mask in ((key, ~raised), (key + ".lv", raised)):
        if bool(mask.any()):
            v = float(r[mask].max())
            out[name] = max(out.get(name, 0.0), v)
            if not yardstick:
                bar = _post_bar(key, name.endswith(".lv"))
                k = int(torch.where(mask, r, torch.full_like(r, -1.0)).argmax())
                assert v < bar, (name, v, divmod(k, r.shape[1]), bar)


def pivot_exchanges(M):
    """Columns at which Gauss-Jordan with first-maximum partial pivoting exchanges rows of M (float64 replay of the kernel's rule)."""
    M = M.double().clone()
    n = M.shape[0]
    cols = []
    for c in range(n):
        piv = c + int(M[c:, c].abs().argmax())   # argmax returns the first maximum
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
            cols.append(c)
        f = M[:, c] / M[c, c]
        f[c] = 0.0
        M = M - f[:, None] * M[c][None, :]
    return cols


def _assert_inputs(pr, spd_filt=True):
    """What the cases rely on, on the float64 view of the operands alone: Sigma_{t+1|t} and Q positive definite (every solve
    regular), and Sigma_{t|t} too unless the problem poisons it on purpose."""
    lam = lambda M: float(torch.linalg.eigvalsh(0.5 * (M.double() + M.double().mT)).min())
    assert lam(pr["Sigmas_pred"]) > 0 and lam(pr["Q"]) > 0, "Sigma_{t+1|t} or Q is not positive definite"
    assert not spd_filt or lam(pr["Sigmas_filt"]) > 0, "Sigma_{t|t} is not positive definite"


def _assert_pivots(pr):
    """The float64 replay of the solve's pivoting exchanges rows at EVERY item with t < T-1, at n = 16 somewhere at >= 8 columns."""
    B, T, n = pr["mus_filt"].shape
    counts = [[len(pivot_exchanges(pr["Sigmas_pred"][b, t + 1].T)) for t in range(T - 1)] for b in range(B)]
    assert all(k > 0 for row in counts for k in row), ("an item's solve exchanges no rows: another seed", counts)
    assert n != 16 or max(k for row in counts for k in row) >= 8, counts


def gains_per_item(dev, pr, want_levels=(0,), pivots=None, spd_filt=True, yardstick=False):
    """The gains launch alone (PosteriorCall.GAINS over guarded buffers) against restate_gains in float64, one (b, t) at a time:
    J, L, c under POST_STEP_TOL; levels equal; L lower triangular to the bit; J of item T-1 exactly 0; z and a untouched.
    pivots="every": a float64 replay of the solve's pivoting over Sigma_{t+1|t}^T must exchange rows at EVERY item with
    t < T-1 (and, at n = 16, at 8 or more columns of some item).  Returns {family.quantity: largest ratio}, levels of the float64 run."""
    B, T, n = pr["mus_filt"].shape
    fam = post_family(n)
    _assert_inputs(pr, spd_filt)
    J, L, c, levels, lam = restate_gains(pr, torch.float64)
    assert sorted(set(levels.flatten().tolist())) == sorted(want_levels), levels
    if pivots == "every":
        _assert_pivots(pr)
    if yardstick:
        gJ, gL, gc, glv = restate_gains(pr, torch.float32)[:4]
    else:
        call = GuardedCall(dev, pr)
        call.run(call.call.GAINS)
        call.check(("ws", "levels"))
        gJ, gL, gc, glv = call.gains()
        assert bool((gL.triu(1) == 0).all()), "L has a non-zero above its diagonal"
        assert bool((gJ[:, -1] == 0).all()), "J of item T-1 is not exactly 0"
    assert glv.dtype == torch.int32 and torch.equal(glv, levels), (glv, levels)
    out, raised, none = {}, levels > 0, torch.zeros_like(levels, dtype=torch.bool)
    _compare(fam + ".J", gJ, J, none, out, yardstick)
    _compare(fam + ".c", gc, c, none, out, yardstick)
    _compare(fam + ".L", gL, L, raised, out, yardstick)
    return out, levels, lam


def paths_per_step(dev, pr, misalign=None, isolate=False, want_levels=(0,), pivots=None, spd_filt=True, yardstick=False):
    """The whole call over guarded buffers against the float64 restatement, one (path, step) at a time: z and a under
    POST_STEP_TOL, and a against C_t z + L_R eta evaluated in float64 on the kernel's own z ("emit").  isolate: other draws for
    ONE path leave every other path's bits alone; another Sigma_{t|t} at one (b, t) leaves every other sequence's bits alone,
    and sequence b's at the steps after t.  Returns {family.quantity: largest ratio}."""
    B, T, n = pr["mus_filt"].shape
    S, p, fam = pr["S"], pr["Cm"].shape[-2], post_family(n)
    _assert_inputs(pr, spd_filt)
    if pivots == "every":
        _assert_pivots(pr)
    gains = restate_gains(pr, torch.float64)
    levels = gains[3]
    assert sorted(set(levels.flatten().tolist())) == sorted(want_levels), levels
    z64, a64 = restate_paths_vec(pr, torch.float64, gains)
    if yardstick:
        z, a = restate_paths_vec(pr, torch.float32)
    else:
        call = GuardedCall(dev, pr, misalign).run()
        call.check(("ws", "levels", "z", "a"))
        z, a = call.call.z.cpu().clone(), call.call.a.cpu().clone()
        assert torch.equal(call.call.levels.cpu(), levels)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(a).all())
    down = (levels > 0).flip(1).cummax(1).values.flip(1) if pr.get("eps") is not None else torch.zeros(B, T, dtype=torch.bool)
    down = down[:, None].expand(B, S, T).reshape(B * S, T)   # (path, step)s that a raised item's L has reached
    out = {}
    flat = lambda t: t.reshape(B * S, T, -1)
    _compare(fam + ".z", flat(z), flat(z64), down, out, yardstick)
    _compare(fam + ".a", flat(a), flat(a64), down, out, yardstick)
    _compare(fam + ".emit", flat(a), flat(emit(pr, z, torch.float64)), torch.zeros_like(down), out, yardstick)
    if isolate and not yardstick:
        g = torch.Generator().manual_seed(4242)
        for r in sorted({0, (B * S) // 2, B * S - 1}):
            other = dict(pr, eps=pr["eps"].clone())
            other["eps"].view(B * S, T, n)[r] = torch.randn(T, n, generator=g)
            c2 = GuardedCall(dev, other, misalign).run()
            rest = [q for q in range(B * S) if q != r]
            assert torch.equal(c2.call.z.cpu().view(B * S, T, n)[rest], z.view(B * S, T, n)[rest]), ("z: another path changed with path", r)
            assert torch.equal(c2.call.a.cpu().view(B * S, T, p)[rest], a.view(B * S, T, p)[rest]), ("a: another path changed with path", r)
            assert not torch.equal(c2.call.z.cpu().view(B * S, T, n)[r], z.view(B * S, T, n)[r])
        for b, t in sorted({(0, 0), (B // 2, T // 2), (B - 1, T - 1)}):
            other = dict(pr, Sigmas_filt=pr["Sigmas_filt"].clone())
            other["Sigmas_filt"][b, t] *= 1.25
            c2 = GuardedCall(dev, other, misalign).run()
            z2, a2 = c2.call.z.cpu(), c2.call.a.cpu()
            rest = [q for q in range(B) if q != b]
            assert torch.equal(z2[rest], z[rest]) and torch.equal(a2[rest], a[rest]), ("another sequence changed with Sigma_f of", b, t)
            assert torch.equal(z2[b, :, t + 1:], z[b, :, t + 1:]) and torch.equal(a2[b, :, t + 1:], a[b, :, t + 1:]), ("later steps changed", b, t)
            assert not torch.equal(z2[b, :, t], z[b, :, t])
    return out


# ---- ladder -----------------------------------------------------------------------------------------------------------------
LADDER_WANT = {-3.16e-6: 1, -3.16e-5: 2, -3.16e-4: 3, -3.16e-3: 4, -1.0: 5}
# n = 4, items 4 ... 7 of (B, T) = (4, 5) - ONE wavefront of the gains kernel - at four different raised levels
LADDER_ONE_WAVE = dict(n=4, B=4, T=5, targets=((0, 4, -3.16e-6), (1, 0, -3.16e-4), (1, 1, -3.16e-3), (1, 2, -1.0)))
# n = 4, 15 items: the raised item is the last one, and the dead slot of the last wavefront repeats it
LADDER_LAST_ITEM = dict(n=4, B=3, T=5, targets=((2, 4, -3.16e-4),))
LADDER_CASES = {"n4": dict(n=4), "n16": dict(n=16), "rt5": dict(n=5), "one_wave": LADDER_ONE_WAVE, "last_item": LADDER_LAST_ITEM}


def ladder_per_item(dev, name, yardstick=False):
    """ladder_problem(**LADDER_CASES[name]) through gains_per_item and paths_per_step: every target at its level in the float64
    run, every item a factor 3 from every rung, L per item under the .lv bar."""
    kw = LADDER_CASES[name]
    pr, targets = ladder_problem(**kw)
    want = sorted({0} | {LADDER_WANT[tg] for _, _, tg in targets})
    out, levels, lam = gains_per_item(dev, pr, want_levels=want, spd_filt=False, yardstick=yardstick)
    for b, t, target in targets:
        assert int(levels[b, t]) == LADDER_WANT[target], (b, t, target, int(levels[b, t]), float(lam[b, t]))
    assert int((levels > 0).sum()) == len(targets)
    if name == "one_wave":
        assert [divmod(4 + k, kw["T"]) for k in range(4)] == [tg[:2] for tg in targets] and len(set(levels.flatten()[4:8].tolist())) == 4
    if name == "last_item":
        assert (kw["B"] * kw["T"]) % 4 != 0 and targets[0][:2] == (kw["B"] - 1, kw["T"] - 1)
    for b in range(lam.shape[0]):      # every item a factor 3 away from every rung: fp32 rounding cannot move it to a neighbour
        for t in range(lam.shape[1]):
            if lam[b, t] < 0:
                assert all(-lam[b, t] >= 3 * r or -lam[b, t] <= r / 3 for r in RUNGS), (b, t, float(lam[b, t]))
    for k, v in paths_per_step(dev, pr, want_levels=want, spd_filt=False, yardstick=yardstick).items():
        out[k] = max(out.get(k, 0.0), v)
    return out


# ---- case lists -------------------------------------------------------------------------------------------------------------
def _post_case(i, n, p, B, S, T, **kw):
    """Options rotate with the index: per-step / shared Q, shared A and C (stride 0), emission noise."""
    c = dict(n=n, p=p, B=B, S=S, T=T, seed=300 + i, per_step_Q=i % 2 == 0, shared_ac=i % 3 == 1, emission_noise=i % 4 < 2,
             with_noise=True, rescaled=False, misalign=None, isolate=False, pivots=None)
    c.update(kw)
    return c


# (seeds of the rescaled problems: the first from 300 + index on at which EVERY item's solve exchanges rows - asserted by the case)
POST_GAIN_CASES = ([_post_case(i, n, 2, 3, 1, 6, rescaled=True, pivots="every", seed=sd) for i, (n, sd) in enumerate([(4, 301), (16, 301), (5, 302)])] +
                   [_post_case(3 + i, n, 2, B, 1, T) for i, (n, B, T) in enumerate([(4, 1, 1), (4, 1, 2), (4, 1, 3), (4, 3, 3), (4, 5, 1),
                                                                                  (16, 1, 1), (16, 3, 2), (5, 3, 3), (1, 2, 3), (7, 1, 4), (12, 2, 2)])])
# T = 1 ... 9 on each of the three path kernels: every residue of the ring of four, twice; misaligned consumers take the LDS kernel
POST_RING_CASES = [_post_case(5 * T + j, n, 2, 2, 3, T, misalign=mis)
                   for T in range(1, 10) for j, (n, mis) in enumerate([(4, None), (16, None), (5, None), (4, "eps"), (16, "ws")])]
POST_SHAPE_CASES = ([_post_case(60 + i, n, 2, B, S, 5, isolate=(B, S) == (5, 13)) for i, (n, B, S) in enumerate(
                        [(4, 1, 63), (4, 1, 64), (4, 5, 13), (5, 1, 63), (5, 2, 32), (5, 5, 13)])] +   # R = 63, 64, 65: one wavefront and a lane more
                    [_post_case(70 + i, 16, 2, B, S, 5, isolate=(B, S) == (3, 3)) for i, (B, S) in enumerate([(1, 3), (2, 2), (5, 1), (3, 3)])] +
                    [_post_case(80 + i, n, 2, 3, 1, 4) for i, n in enumerate((4, 16, 5))] +                  # S = 1
                    [_post_case(84 + i, n, 2, 2, 70, 3) for i, n in enumerate((4, 16, 5))] +                 # S = 70
                    [_post_case(90 + 2 * i + e, n, p, 2, 3, 4, emission_noise=bool(e)) for i, (n, p) in enumerate(
                        [(4, 1), (16, 2), (5, 3), (4, 16), (16, 16), (3, 1), (16, 3)]) for e in range(2)] +   # p = 1, 2, 3, 16 with and without eta
                    [_post_case(110 + i, n, 2, 2, 3, 6, with_noise=False) for i, n in enumerate((4, 16, 5))] +   # eps = None
                    [_post_case(120 + i, n, 3, 3, 4, 6, rescaled=True, pivots="every", isolate=True) for i, n in enumerate((4, 16, 5))])
POST_EMIT_CASE = _post_case(0, 4, 2, 1, 65, 1009)   # 65585 rows > 1024 wavefronts of rows: the emission strides over its grid


def post_case_id(c):
    return "n%dp%d_B%dS%dT%d_%s%s%s%s%s%s" % (c["n"], c["p"], c["B"], c["S"], c["T"], "Qt" if c["per_step_Q"] else "Q1", "_AC1" if c["shared_ac"] else "",
                                               "_eta" if c["emission_noise"] else "", "" if c["with_noise"] else "_noeps",
                                               "_rescaled" if c["rescaled"] else "", "_off_" + c["misalign"] if c["misalign"] else "")


def post_case_problem(c):
    return random_problem(c["n"], c["p"], c["B"], c["S"], c["T"], seed=c["seed"], per_step_Q=c["per_step_Q"], with_noise=c["with_noise"],
                          emission_noise=c["emission_noise"], shared_ac=c["shared_ac"], rescaled=c["rescaled"])


def run_gain_case(dev, c, **kw):
    return gains_per_item(dev, post_case_problem(c), pivots=c["pivots"], **kw)[0]


def run_path_case(dev, c, **kw):
    return paths_per_step(dev, post_case_problem(c), misalign=c["misalign"], isolate=c["isolate"], pivots=c["pivots"], **kw)


def post_yardstick():
    """POST_YARDSTICK, measured again: the float32 restatement over every case list."""
    out = {}
    runs = ([run_gain_case("cpu", c, yardstick=True) for c in POST_GAIN_CASES] + [ladder_per_item("cpu", k, yardstick=True) for k in LADDER_CASES] +
            [run_path_case("cpu", c, yardstick=True) for c in POST_RING_CASES + POST_SHAPE_CASES + [POST_EMIT_CASE]])
    for r in runs:
        for k, v in r.items():
            out[k] = max(out.get(k, 0.0), v)
    return out
