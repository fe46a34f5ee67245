"""Cases of KalmanFilter.sample_posterior / KVAE.sample_imputations shared by the CPU tier (tests/test_posterior_sample.py: host
simulation, both kernels of csrc/lgssm_post.h on emulated wavefronts) and the GPU tier (tests/test_gpu_posterior_sample.py):
the reference's masked fixtures (noise-free paths = its smoother's means; moments of sampled paths = its smoother's covariances
and the lag-one cross-covariance J_t Sigma_{t+1|T}), the kernels against a restatement of the recursion written here in fp64,
and the per-item Cholesky ladder."""
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


def random_problem(n, p, B, S, T, seed=0, per_step_Q=True, with_noise=True, emission_noise=False):
    """Inputs of lgssm_ops.posterior_paths (host fp32 tensors): SPD filter stacks from a plain fp64 filter over random
    time-varying A, C with the middle third of the steps hidden."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: sc * torch.randn(*s, generator=g, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    A = 0.9 * eye + rn(B, T, n, n, sc=0.15)
    C = rn(B, T, p, n, sc=0.5)
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
    st = lambda v: torch.stack(v, 1).float()
    pr = dict(mus_filt=st(mf), Sigmas_filt=st(Sf), mus_pred=st(mp), Sigmas_pred=st(Sp), A=A.float(), Cm=C.float(), Q=Q.float(), S=S)
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


def restate(pr, dtype):
    """The recursion of KVAE.sample_imputations (its docstring; include/kvae_lgssm.h), written plainly: the gains of every (b, t),
    then one path at a time, in `dtype`.  Returns z, a, levels and the smallest eigenvalue of every P_t."""
    c = lambda t: None if t is None else t.to(dtype)
    mf, Sf, mp, Sp, A, C, Q = (c(pr[k]) for k in ("mus_filt", "Sigmas_filt", "mus_pred", "Sigmas_pred", "A", "Cm", "Q"))
    eps, eta, LR = c(pr.get("eps")), c(pr.get("eta")), c(pr.get("LR"))
    S = pr["S"]
    B, T, n = mf.shape
    p = C.shape[-2]
    at = lambda M, b, t: M if M.dim() == 2 else M[b, t]
    eye = torch.eye(n, dtype=dtype)
    z_out, a_out = torch.zeros(B, S, T, n, dtype=dtype), torch.zeros(B, S, T, p, dtype=dtype)
    levels, lam = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, T, dtype=torch.float64)
    for b in range(B):
        J, L = [None] * T, [None] * T
        for t in range(T):
            if t == T - 1:
                P = Sf[b, t]
            else:
                An = at(A, b, t + 1)
                J[t] = torch.linalg.solve(Sp[b, t + 1].T, (Sf[b, t] @ An.T).T).T
                G = eye - J[t] @ An
                P = G @ Sf[b, t] @ G.T + J[t] @ at(Q, b, t + 1) @ J[t].T
            L[t], lv, lam[b, t] = item_ladder(P)
            levels[b, t] = lv
        for s in range(S):
            z = None
            for t in range(T - 1, -1, -1):
                z = mf[b, t] if t == T - 1 else mf[b, t] + J[t] @ (z - mp[b, t + 1])
                if eps is not None:
                    z = z + L[t] @ eps[b, s, t]
                a = at(C, b, t) @ z
                if eta is not None:
                    a = a + LR @ eta[b, s, t]
                z_out[b, s, t], a_out[b, s, t] = z, a
    return z_out, a_out, levels, lam


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
