"""Device-agnostic cases of kvae_lgssm_switching_pf / lgssm_ops.switching_pf / KalmanFilter.particle_filter_regimes /
KVAE.particle_filter_regimes: run against the host simulation (tests/test_particle_filter.py: the kernel bodies of
csrc/lgssm_spf.h on emulated workgroups) and against the gfx950 library (tests/test_gpu_particle_filter.py).  The reference is
lgssm_ops.switching_pf_torch in FLOAT64 on the same float32-rounded numbers and the same draws, REPLAYING the decisions (regimes,
resampled, ancestors) of the run it is compared with: once one boundary decision differs two free-running particle filters have
nothing to do with each other.  The decisions themselves are compared with the free-running float64 run wherever its margins say
they are not toss-ups.  The exactness and unbiasedness cases are independent of the restatement (every regime path enumerated)."""
import ctypes as C
import math

import torch

from golden_util import rel_err
from swf_cases import _kalman_filter, _kalman_step, _model_case, dynamics, enumerate_paths, inputs, prior, small_model  # noqa: F401
import swf_cases

# (B, G, T, K, n, m, masked, N, ess_threshold): every K whose table padding differs, T = 1, run-time dims below the padded 4,
# one / two / four wavefronts per workgroup, never / sometimes / always resampling
LONG_CASE = (1, 2, 70, 7, 4, 2, True, 128, 0.5)   # the only long one: the prefetch over many steps, T past the 64-lane stride of the sums
CASES = [
    (1, 1, 1, 1, 4, 2, False, 64, 0.5),
    (2, 2, 3, 2, 4, 2, False, 64, 1.0),
    (3, 3, 5, 3, 4, 2, False, 64, 0.5),
    (2, 1, 6, 3, 3, 2, True, 128, 1.0),
    (2, 2, 9, 5, 3, 2, True, 256, 0.5),
    (2, 4, 12, 7, 4, 2, True, 64, 1.0),
    (1, 1, 6, 8, 4, 1, False, 64, 0.0),
]
OUTPUTS = ("log_lik", "log_lik_seq", "regime_filt", "mus_filt", "Sigmas_filt", "ess", "path_log_w")
DECISIONS = ("regimes", "resampled", "ancestors")
STATE = ("log_w", "mu", "Sigma")
# Yardsticks, by the project's standing rule (swf_cases.YARDSTICK): the largest ABSOLUTE distance of switching_pf_torch in FLOAT32
# from its float64 run on the same inputs and draws, both replaying the float64 run's own decisions, over CASES + [LONG_CASE] with
# seed 0, measured on the CPU by yardsticks() (rerun: python tests/spf_cases.py).  Bars = 4 x: the margin covers another
# summation order.  (ess is of size N: its distance is absolute all the same.)
YARDSTICK = {"log_lik": 8.47e-7, "log_lik_seq": 4.82e-6, "regime_filt": 1.11e-6, "mus_filt": 7.47e-7, "Sigmas_filt": 5.25e-7, "ess": 3.94e-5,
             "path_log_w": 1.5e-6, "state_log_w": 1.5e-6, "state_mu": 3.47e-7, "state_Sigma": 5.95e-8}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
# the model-level case (model_level below: the small switching KVAE's own parameters), measured the same way by model_yardsticks()
MODEL_YARDSTICK = {"log_lik": 4.02e-7, "log_lik_seq": 1.4e-6, "regime_filt": 1.49e-7, "mus_filt": 2.22e-7, "Sigmas_filt": 6.08e-6, "ess": 2.48e-5,
                   "path_log_w": 1.95e-6, "state_log_w": 1.95e-6, "state_mu": 9.45e-7, "state_Sigma": 2.58e-5}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}
# the identity-prior case (identity_prior below): the log weights of the particles whose regime the data rule out fall to -50, where
# one float32 rounding is as large as the bar measured on CASES (whose log weights stay above -15); the same rule on that case's own
# inputs, by identity_yardstick().  Its other outputs keep the bars above.
IDENTITY_LOG_W = 8.05e-6
IDENTITY_TOL = dict(TOL, path_log_w=4.0 * IDENTITY_LOG_W, state_log_w=4.0 * IDENTITY_LOG_W)
MODEL_PF = dict(num_particles=64, replicates=2, ess_threshold=0.5)
# float64 margins above which float32 must take the same decision, and the share of decisions that may fall under them
MARGIN = {"regimes": 1e-4, "ancestors": 1e-5, "resampled": 1e-3}
EXCUSED = 0.05


def draws(case, seed=0):
    """(pf_regime [B,G,T,N], pf_resample [B,G,T]) in float32, uniform on [0, 1)."""
    B, G, T, K, n, m, masked, N, thr = case
    g = torch.Generator().manual_seed(7000000 + 100000 * seed + 1000 * B + 100 * G + 10 * T + K + N)
    return torch.rand(B, G, T, N, generator=g), torch.rand(B, G, T, generator=g)


def restate(args, th, ph, mask, thr, dtype=torch.float64, **kw):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_pf_torch(*(a.to(dtype) for a in args), th.to(dtype), ph.to(dtype), mask=mask, ess_threshold=thr, **kw)


_REF = {}


def reference(case, seed=0):
    """(args32, mask, pf_regime, pf_resample, the free-running float64 restatement with its margins), computed once per case and
    shared among the tests; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        B, G, T, K, n, m, masked, N, thr = case
        args, mask = inputs(B, T, K, n, m, masked, seed=seed)
        th, ph = draws(case, seed)
        _REF[key] = (args, mask, th, ph, restate(args, th, ph, mask, thr, margins=True))
    return _REF[key]


def decisions_of(got):
    return {k: got[k].detach().cpu() for k in DECISIONS}


def distances(got, ref):
    """Largest absolute distance of every float output from the float64 run."""
    c = lambda t: t.detach().cpu().double()
    out = {k: float((c(got[k]) - ref[k]).abs().max()) for k in OUTPUTS}
    for k in STATE:
        out["state_" + k] = float((c(got["state"][k]) - ref["state"][k]).abs().max())
    return out


def check_outputs(got, ref, mask, tol=None, what=""):
    """Every output of one call against the float64 run that replayed its decisions, under the bars; the integer outputs exactly;
    on hidden steps log_lik = 0; the lineages are the host-side walk."""
    from kvae.kalman import lgssm_ops
    tol = TOL if tol is None else tol
    c = lambda t: t.detach().cpu()
    dist = distances(got, ref)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in OUTPUTS:
        assert got[k].shape == ref[k].shape, k
        assert bool(torch.isfinite(c(got[k]).double()).all()), k
    for k in ("regimes", "ancestors", "levels", "paths"):
        assert got[k].dtype == torch.int32 and torch.equal(c(got[k]), ref[k]), k
    assert got["resampled"].dtype == torch.bool and torch.equal(c(got["resampled"]), ref["resampled"])
    assert got["state"]["regime"].dtype == torch.int32 and torch.equal(c(got["state"]["regime"]), ref["state"]["regime"])
    assert torch.equal(c(got["paths"]), lgssm_ops.lineages(c(got["regimes"]), c(got["ancestors"])))
    assert torch.equal(c(got["path_log_w"]), c(got["state"]["log_w"]))
    K = got["regime_filt"].shape[-1]
    assert int(c(got["regimes"]).min()) >= 0 and int(c(got["regimes"]).max()) < K
    if mask is not None:
        hidden = (mask == 0)[:, None, :].expand_as(c(got["log_lik"]))
        assert bool(hidden.any())
        assert bool((c(got["log_lik"])[hidden] == 0).all())
    return dist


def check_decisions(got, free, thr, what=""):
    """The run's own decisions against the free-running float64 restatement, per replicate up to (and at) its first step with a
    decision under its margin: equal wherever the float64 margin says the decision is not a toss-up.  Past that step the two
    runs may be different particle systems."""
    c = lambda t: t.detach().cpu()
    rg, an, rs = c(got["regimes"]), c(got["ancestors"]), c(got["resampled"])
    ok_r = free["margin_regime"] >= MARGIN["regimes"]                                       # [B,G,T,N]
    ok_a = (free["margin_ancestor"] >= MARGIN["ancestors"]) | ~free["resampled"].unsqueeze(-1)
    compare_rs = 0.0 < thr < 1.0
    ok_s = (free["margin_ess"] >= MARGIN["resampled"]) if compare_rs else torch.ones_like(free["resampled"])
    clean = ok_r.all(-1) & ok_a.all(-1) & ok_s                                              # [B,G,T]
    before = torch.cat([torch.ones_like(clean[..., :1]), clean[..., :-1]], -1).long().cumprod(-1).bool()   # every earlier step clean
    compared = int(before.sum())
    print(what, "decisions: steps compared", compared, "of", before.numel())
    assert bool(before[..., 0].all())
    m = before.unsqueeze(-1) & ok_r
    assert torch.equal(rg[m], free["regimes"][m]), what
    if compare_rs:
        m = before & ok_s
        assert torch.equal(rs[m], free["resampled"][m]), what
    same_rs = before & (rs == free["resampled"])
    m = same_rs.unsqueeze(-1) & ok_a
    assert torch.equal(an[m], free["ancestors"][m]), what


def excused_shares(free, thr):
    """The share of the float64 run's own decisions that fall under their margins: (regimes, ancestors, resampled)."""
    r = float((free["margin_regime"] < MARGIN["regimes"]).double().mean())
    did = free["resampled"].unsqueeze(-1).expand_as(free["margin_ancestor"])
    a = float((free["margin_ancestor"][did] < MARGIN["ancestors"]).double().mean()) if bool(did.any()) else 0.0
    s = float((free["margin_ess"] < MARGIN["resampled"]).double().mean()) if 0.0 < thr < 1.0 else 0.0
    return r, a, s


def run(DEV, args, th, ph, mask=None, thr=0.5, **kw):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_pf(*(a.to(DEV) for a in args), th.to(DEV), ph.to(DEV), mask=None if mask is None else mask.to(DEV),
                                  ess_threshold=thr, **kw)


def per_step(DEV, case):
    args, mask, th, ph, free = reference(case)
    thr = case[-1]
    got = run(DEV, args, th, ph, mask, thr)
    ref = restate(args, th, ph, mask, thr, force=decisions_of(got))
    dist = check_outputs(got, ref, mask, what=str(case))
    check_decisions(got, free, thr, what=str(case))
    first_step_is_exact(case, got, TOL)
    return dist


def yardsticks():
    """The float32 torch restatement against the float64 one, both replaying the float64 run's decisions, over CASES +
    [LONG_CASE]: the numbers YARDSTICK holds."""
    worst = {}
    for case in CASES + [LONG_CASE]:
        args, mask, th, ph, free = reference(case)
        force = decisions_of(free)
        f32 = restate(args, th, ph, mask, case[-1], dtype=torch.float32, force=force)
        f64 = restate(args, th, ph, mask, case[-1], force=force)
        for k, v in distances(f32, f64).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def margins_hold(case):
    """At most EXCUSED of the float64 reference's own decisions of each kind fall under their margin."""
    free = reference(case)[4]
    shares = excused_shares(free, case[-1])
    print(case, "share of (regimes, ancestors, resampled) under their margins", shares)
    assert all(s <= EXCUSED for s in shares), shares
    return shares


# ---- exactness ----------------------------------------------------------------------------------------------------------------
def _first_step_exact(case):
    """Exact log p(a_0) [B] and p(s_0 | a_0) [B,K] of a case by enumeration; a hidden first step has log_lik 0 and the prior."""
    B, G, T, K, n, m, masked, N, thr = case
    args, mask, *_ = reference(case)
    a64 = tuple(a.double() for a in args)
    ll, rf = enumerate_paths(a64[:8] + (a64[8][:, :1], a64[9][:, :1]))
    ll, rf = ll[:, 0], rf[:, 0]
    if mask is not None:
        hid = mask[:, 0] == 0
        ll = torch.where(hid, torch.zeros_like(ll), ll)
        rf = torch.where(hid[:, None], torch.full_like(rf, 1.0 / K), rf)
    return ll, rf


def first_step_is_exact(case, got=None, tol=None):
    """Before step 0 every particle is the same particle and the proposal is fully adapted: log_lik and regime_filt of step 0 are
    exact whatever the draws.  got None: the float64 restatement at 1e-9 relative; else a run under the bars."""
    ll, rf = _first_step_exact(case)
    if got is None:
        free = reference(case)[4]
        for g in range(case[1]):
            e_ll = float((free["log_lik"][:, g, 0] - ll).abs().max() / ll.abs().max().clamp_min(1.0))
            e_rf = float((free["regime_filt"][:, g, 0] - rf).abs().max())
            assert e_ll < 1e-9 and e_rf < 1e-9, (case, g, e_ll, e_rf)
        return
    c = lambda t: t.detach().cpu().double()
    assert float((c(got["log_lik"])[:, :, 0] - ll[:, None]).abs().max()) < tol["log_lik"]
    assert float((c(got["regime_filt"])[:, :, 0] - rf[:, None]).abs().max()) < tol["regime_filt"]


def exact_shared_dynamics(K=3, T=6, B=2, G=2, N=64):
    """All regimes share A, B, Q: every particle carries the single filter's belief whatever its regime history - exact at every
    step, under all three resampling rules and any draws (float64 restatement, 1e-9)."""
    args, _ = inputs(B, T, K, seed=5, shared=True)
    args = tuple(a.double() for a in args)
    args = args[:5] + (args[5] / args[5].sum(-1, keepdim=True),) + args[6:]   # rows of the float32 prior sum to 1 + 1.5e-8
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    ll = torch.zeros(B, T, dtype=torch.float64)
    mus = torch.zeros(B, T, A.shape[1], dtype=torch.float64)
    mu, Sig = mu0.expand(B, -1), Sigma0.expand(B, -1, -1)
    for t in range(T):
        mu, Sig, ll[:, t] = _kalman_step(mu, Sig, Y[:, t], U[:, t], A[0], Bm[0], Q[0], Cm, R)
        mus[:, t] = mu
    th, ph = draws((B, G, T, K, 4, 2, False, N, 0.5), seed=5)
    for thr in (0.0, 0.5, 1.0):
        got = restate(args, th, ph, None, thr)
        e_ll = rel_err(got["log_lik"], ll[:, None].expand_as(got["log_lik"]))
        e_mu = rel_err(got["mus_filt"], mus[:, None].expand_as(got["mus_filt"]))
        e_S = rel_err(got["Sigmas_filt"][:, :, -1], Sig[:, None].expand_as(got["Sigmas_filt"][:, :, -1]))
        print("shared dynamics", thr, e_ll, e_mu, e_S)
        assert e_ll < 1e-9 and e_mu < 1e-9 and e_S < 1e-9, (thr, e_ll, e_mu, e_S)
        assert float((got["regime_filt"].sum(-1) - 1).abs().max()) < 1e-12


def vs_existing_filter(DEV, K, thr, B=3, T=9, G=2, N=64):
    """K identical regimes (K = 1: the one regime): every replicate of the particle filter is the existing filter.  log_lik
    against KalmanFilter.predictive and mus_filt / Sigmas_filt against KalmanFilter.filter over the single regime, under the bars."""
    from kvae import noise
    args, mask = inputs(B, T, K, masked=True, seed=7, shared=True)
    one = tuple(a[:1] if i < 3 else a for i, a in enumerate(args[:5])) + (prior(1),) + args[6:]
    kf1, kfK = _kalman_filter(one, DEV), _kalman_filter(args, DEV)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    th, ph = draws((B, G, T, K, 4, 2, True, N, thr), seed=7)
    with noise.inject(pf_regime=th, pf_resample=ph):
        got = kfK.particle_filter_regimes(Y, U, mk, num_particles=N, replicates=G, ess_threshold=thr)
    pred = kf1.predictive(Y, U, mk)
    mf, Sf = pred["filter"][0].squeeze(-1), pred["filter"][1]
    c = lambda t: t.detach().cpu().double()
    for name, g, w in (("log_lik", got["log_lik"], pred["ll"]), ("log_lik_seq", got["log_lik_seq"], pred["seq_ll"]),
                       ("mus_filt", got["mus_filt"], mf), ("Sigmas_filt", got["Sigmas_filt"], Sf)):
        d = float((c(g) - c(w).unsqueeze(1)).abs().max())
        print("vs the existing filter", K, thr, name, d, TOL[name])
        assert d < TOL[name], (name, d)
    assert torch.equal(got["levels"].cpu(), pred["levels"].cpu().unsqueeze(1).expand_as(got["levels"]))
    assert float((c(got["regime_filt"]).sum(-1) - 1.0).abs().max()) < 4 * TOL["regime_filt"]


def exact_single_regime(B=3, T=9, G=2, N=64):
    """K = 1 in float64 over T masked steps, under all three thresholds: every replicate of the restatement equals the existing
    filter at 1e-9 relative.  KalmanFilter.filter / predictive themselves run in float32 only (their kernels are the only
    implementation), so their float64 statements stand in: the oracle's filter_step - the reference's KalmanFilter.filter step,
    which the filter kernels are tested against - and lgssm_ops.predictive_torch over its one-step-ahead beliefs."""
    from kvae.kalman import lgssm_ops
    from oracle import torch_oracle as O
    args, mask = inputs(B, T, 1, masked=True, seed=7)
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = (a.double() for a in args)
    mu, Sig = mu0.expand(B, -1).unsqueeze(-1), Sigma0.expand(B, -1, -1)
    mf, Sf, mp, Sp = [], [], [], []
    for t in range(T):
        mu, Sig, m_p, S_p = O.filter_step(mu, Sig, Y[:, t], U[:, t], A[0], Bm[0], Cm, Q[0], R, mask[:, t].double())
        mf.append(mu.squeeze(-1)), Sf.append(Sig), mp.append(m_p.squeeze(-1)), Sp.append(S_p)
    mf, Sf, mp, Sp = (torch.stack(v, 1) for v in (mf, Sf, mp, Sp))
    pred = lgssm_ops.predictive_torch(mp, Sp, Cm, R, Y, mask)
    th, ph = draws((B, G, T, 1, 4, 2, True, N, 0.5), seed=7)
    for thr in (0.0, 0.5, 1.0):
        got = restate(args, th, ph, mask, thr)
        e = {"log_lik": rel_err(got["log_lik"], pred["ll"][:, None].expand_as(got["log_lik"])),
             "log_lik_seq": rel_err(got["log_lik_seq"], pred["seq_ll"][:, None].expand_as(got["log_lik_seq"])),
             "mus_filt": rel_err(got["mus_filt"], mf[:, None].expand_as(got["mus_filt"])),
             "Sigmas_filt": rel_err(got["Sigmas_filt"], Sf[:, None].expand_as(got["Sigmas_filt"]))}
        print("K = 1 in float64 against the single filter", thr, e)
        assert all(v < 1e-9 for v in e.values()), (thr, e)
        assert torch.equal(got["levels"], pred["levels"][:, None].expand_as(got["levels"]))
        assert bool((got["regime_filt"] == 1.0).all()) and bool((got["regimes"] == 0).all())


def _identity_inputs(K=3, T=6, B=2, G=2, N=64):
    args, _ = inputs(B, T, K, seed=4, p_stay=1.0)
    assert bool((args[5] == torch.eye(K)).all())
    return args, draws((B, G, T, K, 4, 2, False, N, 1.0), seed=4)


def identity_yardstick():
    """The float32 restatement against the float64 one on the identity-prior inputs, as yardsticks(): the number IDENTITY_LOG_W holds."""
    args, (th, ph) = _identity_inputs()
    worst = 0.0
    for thr in (0.5, 1.0):
        force = decisions_of(restate(args, th, ph, None, thr))
        d = distances(restate(args, th, ph, None, thr, dtype=torch.float32, force=force), restate(args, th, ph, None, thr, force=force))
        worst = max(worst, d["state_log_w"])
    return worst


def identity_prior(DEV=None, K=3, T=6, B=2, G=2, N=64):
    """P = I (StickyRegimePrior(K, 1.0): zeros in P, log P = -inf): no NaN or inf anywhere, and no particle ever draws a regime
    of zero probability - every lineage keeps the regime it drew at step 0.  DEV None: the float64 restatement."""
    args, (th, ph) = _identity_inputs(K, T, B, G, N)
    for thr in (0.5, 1.0):
        got = restate(args, th, ph, None, thr) if DEV is None else run(DEV, args, th, ph, None, thr)
        for k in OUTPUTS:
            assert bool(torch.isfinite(got[k].double()).all()), k
        for k in STATE:
            assert bool(torch.isfinite(got["state"][k].double()).all()), k
        paths = got["paths"].cpu()
        assert bool((paths == paths[..., :1]).all())
        rg, an = got["regimes"].cpu().long(), got["ancestors"].cpu().long()
        for t in range(1, T):   # the draw of slot i at step t is the regime that slot carried in
            carried = rg[:, :, t - 1].gather(-1, an[:, :, t - 1])
            assert torch.equal(rg[:, :, t], carried), t
        if DEV is not None:
            ref = restate(args, th, ph, None, thr, force=decisions_of(got))
            check_outputs(got, ref, None, tol=IDENTITY_TOL, what="P = I on the kernel")


# ---- the ladder above level 0 ------------------------------------------------------------------------------------------------
def ladder_levels(DEV):
    """Every level of the density's jitter ladder, through a carried state: in replicate g one particle holds Sigma = -s_g I, with
    s_g found by bisection in float64 so that the smallest eigenvalue of its forecast covariance under regime 0 is 0 (healthy: level
    0), -3e-6, -3e-5, -3e-4, -3e-3, -3e-2 - a factor 3 inside the jitters 1e-5 .. 1e-2 that first repair them, and past the last.
    `levels` of step 0 are 0 .. 5 over the replicates, on the float64 restatement and on the kernel, and the kernel's equal the
    restatement's at both steps; every float output stays finite."""
    B, T, K, N, thr = 1, 2, 2, 64, 0.0
    targets = (None, 3e-6, 3e-5, 3e-4, 3e-3, 3e-2)
    G = len(targets)
    args, _ = inputs(B, T, K, seed=9)
    A, Bm, Q, Cm, R, P, mu0, Sigma0 = (a.double() for a in args[:8])
    M0, M1 = Cm @ Q[0] @ Cm.T + R, Cm @ A[0] @ A[0].T @ Cm.T
    low = lambda sc: float(torch.linalg.eigvalsh(M0 - sc * M1)[0])
    Sig = Sigma0.expand(B, G, N, 4, 4).clone()
    for g, target in enumerate(targets):
        if target is None:
            continue
        lo, hi = 0.0, 1.0
        assert low(lo) > 0 > low(hi) + target
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if low(mid) > -target else (lo, mid)
        Sig[0, g, 5] = -hi * torch.eye(4, dtype=torch.float64)
    state = {"log_w": torch.full((B, G, N), -math.log(N)), "regime": torch.zeros(B, G, N, dtype=torch.int32),
             "mu": mu0.float().expand(B, G, N, 4).contiguous(), "Sigma": Sig.float()}
    th, ph = draws((B, G, T, K, 4, 2, False, N, thr), seed=9)
    ref = restate(args, th, ph, None, thr, state={k: (v if k == "regime" else v.double()) for k, v in state.items()})
    assert ref["levels"][0, :, 0].tolist() == [0, 1, 2, 3, 4, 5], ref["levels"]
    if DEV is None:
        return
    got = run(DEV, args, th, ph, None, thr, state={k: v.to(DEV) for k, v in state.items()})
    assert got["levels"].dtype == torch.int32 and torch.equal(got["levels"].cpu(), ref["levels"]), (got["levels"], ref["levels"])
    for k in OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), k


# ---- unbiasedness ----------------------------------------------------------------------------------------------------------------
def measure_spread(K, T, thr, chunks=32, per_chunk=1024, B=4, N=64):
    """The spread (standard deviation over replicates) of the two unbiased estimators of `unbiased`, from chunks * per_chunk
    replicates of the float32 restatement with seeds of their own: (sigma of exp(cumulative log_lik - exact) regime_filt_t(j)
    [B,T,K], sigma of exp(log_lik_seq - exact) [B], their means).  What tests/golden/spf_unbiased_spread.npz holds
    (python tests/spf_cases.py spread: a few minutes per case)."""
    args, _ = inputs(B, T, K, seed=6)
    ll, _ = enumerate_paths(tuple(a.double() for a in args))
    exact = ll.cumsum(-1)
    s1, s2 = torch.zeros(B, T, K, dtype=torch.float64), torch.zeros(B, T, K, dtype=torch.float64)
    l1, l2 = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for ch in range(chunks):
        g = torch.Generator().manual_seed(990000 + ch)
        th, ph = torch.rand(B, per_chunk, T, N, generator=g), torch.rand(B, per_chunk, T, generator=g)
        got = restate(args, th, ph, None, thr, dtype=torch.float32, want=("log_lik", "regime_filt"))
        w = (got["log_lik"].double().cumsum(-1) - exact[:, None]).exp()
        est = w.unsqueeze(-1) * got["regime_filt"].double()
        s1 += est.sum(1)
        s2 += (est * est).sum(1)
        l1 += w[..., -1].sum(1)
        l2 += (w[..., -1] ** 2).sum(1)
    n = chunks * per_chunk
    sd = lambda a, b: ((b / n - (a / n) ** 2) * n / (n - 1)).clamp_min(0).sqrt()
    return sd(s1, s2), sd(l1, l2), s1 / n, l1 / n


def spread_key(K, T, thr):
    return f"K{K}_T{T}_thr{thr}"


_EXACT, _SPREAD = {}, {}


def unbiased(DEV, K, T, thr, G=512, B=4, N=64, impl=None):
    """The mean over G replicates of exp(log_lik_seq - exact) lies within 5 standard errors of 1, and the mean of
    exp(cumulative log_lik - exact) regime_filt_t(j) within 5 standard errors of the exact filtered marginal for EVERY t >= 1 and
    j; both exact values by enumeration of all K^T regime paths.  Fixed seeds.
    The standard error is the sample's own, spread / sqrt(G), wherever the sample's spread is of the order of the estimator's
    (at least half of it).  Where it is not, the sample has not seen the estimator's tail and its spread is no standard error:
    the estimator's spread itself is used, as the float32 restatement measured it over 32768 replicates with other seeds
    (measure_spread, tests/golden/spf_unbiased_spread.npz).  In float64 at (K,T) = (3,8), threshold 1, sequence 3, t = 2, j = 2
    (exact 1.542e-6), 512 replicates give 1.439e-6 with a sample spread of 6.8e-8 and a largest term of 1.8e-6 - 44 sample standard
    errors away - while 65536 replicates give 1.526e-6 +- 2.2e-8 with a largest term of 3.3e-4: one replicate in a few thousand
    carries the rest of the mass."""
    import golden_util
    if (K, T) not in _EXACT:
        args, _ = inputs(B, T, K, seed=6)
        _EXACT[(K, T)] = (args, *enumerate_paths(tuple(a.double() for a in args)))
    if not _SPREAD:
        _SPREAD.update(golden_util.load("spf_unbiased_spread"))
    args, ll, rf = _EXACT[(K, T)]
    spread = _SPREAD["regime_" + spread_key(K, T, thr)].double()[:, 1:]
    spread_ll = _SPREAD["lik_" + spread_key(K, T, thr)].double()
    th, ph = draws((B, G, T, K, 4, 2, False, N, thr), seed=6)
    got = run(DEV, args, th, ph, None, thr, want=("log_lik", "log_lik_seq", "regime_filt"), impl=impl)
    lik = got["log_lik"].detach().cpu().double()
    cum, exact = lik.cumsum(-1), ll.cumsum(-1)
    w = (cum - exact[:, None]).exp()                                         # [B,G,T]

    def errors(sample, ref_spread):
        """(standard error per entry, where the sample's own spread was used)"""
        own = sample.std(1)
        seen = own >= 0.5 * ref_spread
        return torch.where(seen, own, ref_spread) / math.sqrt(G), seen

    se_ll, seen_ll = errors(w[..., -1], spread_ll)
    z_ll = (w[..., -1].mean(1) - 1.0).abs() / se_ll
    print("unbiased", (K, T, thr, G), "log_lik_seq: |z| max", float(z_ll.max()), "own spread used for", int(seen_ll.sum()), "of", seen_ll.numel(),
          "; spread of log_lik_seq", float(got["log_lik_seq"].detach().cpu().double().std(1).max()))
    assert float(z_ll.max()) <= 5.0, z_ll
    est = w.unsqueeze(-1) * got["regime_filt"].detach().cpu().double()      # [B,G,T,K]
    diff = (est.mean(1) - rf)[:, 1:].abs()
    se, seen = errors(est[:, :, 1:], spread)
    z = diff / se.clamp_min(1e-300)
    print("unbiased", (K, T, thr, G), "regime_filt: max of |diff| / se", float(z.max()), "; own spread used for", int(seen.sum()), "of", seen.numel(),
          "; max over the others", float(z[~seen].max()) if bool((~seen).any()) else 0.0)
    assert float(z.max()) <= 5.0, (float(z.max()), (z > 5.0).nonzero().tolist())
    return float(z_ll.max())


# ---- lineages ------------------------------------------------------------------------------------------------------------------
def lineage_rules(DEV):
    """paths is the host-side walk (check_outputs asserts that for every case); without resampling slot n's lineage is slot n's
    own draws; after an always-resample run the lineages coalesce backwards in time: the number of distinct ancestor slots never
    grows going back, and at t = 0 there are at most N."""
    args, mask, th, ph, _ = reference(CASES[-1])
    assert CASES[-1][-1] == 0.0
    got = run(DEV, args, th, ph, mask, 0.0)
    assert torch.equal(got["paths"].cpu(), got["regimes"].cpu().transpose(2, 3))
    assert not bool(got["resampled"].any())
    N = CASES[-1][7]
    assert torch.equal(got["ancestors"].cpu(), torch.arange(N, dtype=torch.int32).expand_as(got["ancestors"]))
    case = CASES[5]
    assert case[-1] == 1.0
    args, mask, th, ph, _ = reference(case)
    got = run(DEV, args, th, ph, mask, 1.0)
    assert bool(got["resampled"].all())
    an = got["ancestors"].cpu().long()
    B, G, T, N = an.shape
    i = torch.arange(N).expand(B, G, N)
    prev = None
    for t in range(T - 1, -1, -1):
        i = an[:, :, t].gather(-1, i)
        distinct = torch.tensor([[len(set(i[b, g].tolist())) for g in range(G)] for b in range(B)])
        assert bool((distinct >= 1).all()) and bool((distinct <= N).all())
        assert prev is None or bool((distinct <= prev).all())
        prev = distinct
    print("distinct ancestors at t = 0 after", T, "always-resampled steps:", prev.tolist())


# ---- streaming, partial outputs, repeatability -----------------------------------------------------------------------------------
PER_STEP = ("log_lik", "regime_filt", "mus_filt", "Sigmas_filt", "ess", "resampled", "regimes", "ancestors", "levels")


def _same_state(a, b, what):
    for k in STATE + ("regime",):
        assert torch.equal(a["state"][k], b["state"][k]), (what, "state", k)
    assert torch.equal(a["path_log_w"], b["path_log_w"]), what


def streaming(DEV, case):
    """Chunks of (1, T - 1) and of (3, 4, rest), each continuing from the state of the one before with its slice of the draws:
    the per-step outputs, concatenated, and the final state are the bits of the single call."""
    args, mask, th, ph, _ = reference(case)
    assert mask is not None
    T, thr = case[2], case[-1]
    whole = run(DEV, args, th, ph, mask, thr)
    for sizes in ((1, T - 1), (3, 4, T - 7)):
        assert sum(sizes) == T and all(s > 0 for s in sizes)
        parts, state, t0 = [], None, 0
        for s in sizes:
            sl = slice(t0, t0 + s)
            parts.append(run(DEV, args[:8] + (args[8][:, sl], args[9][:, sl]), th[:, :, sl], ph[:, :, sl], mask[:, sl], thr, state=state))
            state, t0 = parts[-1]["state"], t0 + s
        for k in PER_STEP:
            assert torch.equal(torch.cat([p[k] for p in parts], 2), whole[k]), (sizes, k)
        _same_state(parts[-1], whole, sizes)


def partial_outputs(DEV, case):
    """Each output alone gives the bits of the full call, nothing else is returned; two full calls give the same bits."""
    from kvae.kalman import lgssm_ops
    args, mask, th, ph, _ = reference(case)
    thr = case[-1]
    full, again = run(DEV, args, th, ph, mask, thr), run(DEV, args, th, ph, mask, thr)
    for k in PER_STEP + ("log_lik_seq", "paths"):
        assert torch.equal(full[k], again[k]), k
    _same_state(full, again, "second call")
    for k in lgssm_ops._SPF_OUTPUTS:
        one = run(DEV, args, th, ph, mask, thr, want=(k,))
        assert [n for n, v in one.items() if v is not None] == [k], k
        if k == "state":
            for s in STATE + ("regime",):
                assert torch.equal(one["state"][s], full["state"][s]), s
        else:
            assert torch.equal(one[k], full[k]), k


# ---- routing ------------------------------------------------------------------------------------------------------------------
def routing(DEV):
    """K = 9, n = 5 and N = 96 are outside the kernel: the Python layer takes switching_pf_torch (float32 there), impl="hip" raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    ok = torch.zeros(1, device=DEV)
    S = lgssm_ops.switching_pf_supported
    assert S(8, 4, 4, 2, 64, ok) and S(1, 1, 1, 2, 256, ok) and S(3, 4, 2, 2, 128, ok)
    assert not S(9, 4, 4, 2, 64, ok) and not S(3, 5, 2, 2, 64, ok) and not S(3, 4, 5, 2, 64, ok) and not S(3, 4, 2, 3, 64, ok)
    assert not S(3, 4, 2, 2, 96, ok) and not S(3, 4, 2, 2, 512, ok) and not S(3, 4, 2, 2, 32, ok)
    assert not S(3, 4, 2, 2, 64, ok.double())
    for case in ((2, 2, 4, 9, 4, 2, False, 64, 0.5), (2, 1, 4, 3, 5, 2, True, 64, 1.0), (1, 2, 4, 3, 4, 2, True, 96, 0.5)):
        B, G, T, K, n, m, masked, N, thr = case
        args, mask = inputs(B, T, K, n, m, masked, seed=8)
        th, ph = draws(case, seed=8)
        got = run(DEV, args, th, ph, mask, thr)
        f32 = restate(args, th, ph, mask, thr, dtype=torch.float32)
        ref = restate(args, th, ph, mask, thr, force=decisions_of(got))
        for k in OUTPUTS:
            assert got[k].dtype == torch.float32
            assert rel_err(got[k].cpu(), ref[k]) < 1e-4, k
            if DEV == "cpu":
                assert torch.equal(got[k], f32[k]), k                      # the restatement itself
        with pytest.raises(ValueError, match="impl='hip'"):
            run(DEV, args, th, ph, mask, thr, impl="hip")
    case = (2, 2, 3, 2, 4, 2, True, 64, 0.5)
    args, mask = inputs(2, 3, 2, masked=True)
    th, ph = draws(case)
    with pytest.raises(ValueError):
        run(DEV, args, th, ph, mask, want=("regime_pred",))
    with pytest.raises(ValueError):
        run(DEV, args, th, ph, mask, impl="kernel")
    with pytest.raises(ValueError, match="ess_threshold"):
        run(DEV, args, th, ph, mask, thr=1.5)
    with pytest.raises(ValueError, match="pf_resample"):
        run(DEV, args, th, ph[:, :1], mask)
    with pytest.raises(ValueError, match="state"):
        run(DEV, args, th, ph, mask, state={"log_w": torch.zeros(2, 2, 32), "regime": torch.zeros(2, 2, 64, dtype=torch.int32),
                                            "mu": torch.zeros(2, 2, 64, 4), "Sigma": torch.zeros(2, 2, 64, 4, 4)})
    forced = run(DEV, args, th, ph, mask, impl="torch")
    assert rel_err(forced["log_lik"].cpu(), run(DEV, args, th, ph, mask)["log_lik"].cpu()) < 1e-4


# ---- the C ABI through raw pointers ------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """Error codes of include/kvae_lgssm.h, and not a byte of any output written on error."""
    from kvae import _native as N
    B, G, T, K, n, m, Np = 2, 2, 3, 3, 4, 2, 64
    args, mask = inputs(B, T, K, n, m, masked=True)
    th, ph = draws((B, G, T, K, n, m, True, Np, 0.5))
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), mask=mask.to(DEV), pf_regime=th.to(DEV), pf_resample=ph.to(DEV))
    # buffers large enough for the shapes the failing calls claim (K = 9, n = 5, N = 256) too
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    i32 = torch.int32
    outs = dict(ll=big(B, G, T), seq_ll=big(B, G), regime_filt=big(B, G, T, 9), mus_filt=big(B, G, T, 5), Sigmas_filt=big(B, G, T, 5, 5),
                ess=big(B, G, T), resampled=big(B, G, T, dt=i32), regimes=big(B, G, T, 256, dt=i32), ancestors=big(B, G, T, 256, dt=i32),
                levels=big(B, G, T, dt=i32), paths=big(B, G, 256, T, dt=i32), out_log_w=big(B, G, 256), out_regime=big(B, G, 256, dt=i32),
                out_mu=big(B, G, 256, 5), out_Sigma=big(B, G, 256, 5, 5))
    st = dict(state_log_w=torch.full((B, G, 256), -math.log(Np), device=DEV), state_regime=torch.zeros(B, G, 256, device=DEV, dtype=i32),
              state_mu=torch.zeros(B, G, 256, 5, device=DEV), state_Sigma=torch.eye(5, device=DEV).repeat(B, G, 256, 1, 1))

    def call(drop=(), **kw):
        pr = N.SpfProblem()
        pr.B, pr.G, pr.T, pr.K, pr.N, pr.n, pr.m, pr.p, pr.ess_threshold = B, G, T, K, Np, n, m, 2, 0.5
        for k, v in list(ins.items()) + list(outs.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in kw.items():
            setattr(pr, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        rc = lib.dll.kvae_lgssm_switching_pf(C.byref(pr), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool((v == 7).all()) for v in outs.values())
    assert lib.dll.kvae_lgssm_switching_pf(None, None) == 2
    for k in names + ("pf_regime", "pf_resample"):
        assert call(drop=(k,)) == 2, k                                      # KVAE_ERR_NULL
    assert call(drop=("ll",)) == 2                                          # seq_ll reads ll
    assert call(drop=("regimes",)) == 2 and call(drop=("ancestors",)) == 2  # the lineage walk reads both
    for kw in (dict(B=0), dict(T=0), dict(G=0), dict(B=-1)):
        assert call(**kw) == 1, kw                                          # KVAE_ERR_DIMS
    for kw in (dict(K=9), dict(K=0), dict(n=5), dict(n=0), dict(m=5), dict(p=3), dict(p=1), dict(N=96), dict(N=32), dict(N=512), dict(N=0),
               dict(ess_threshold=1.5), dict(ess_threshold=-0.1), dict(ess_threshold=float("nan"))):
        assert call(**kw) == 4, kw                                          # KVAE_ERR_ARG
    assert call(state_log_w=st["state_log_w"]) == 4
    assert call(state_log_w=st["state_log_w"], state_mu=st["state_mu"], state_Sigma=st["state_Sigma"]) == 4
    assert untouched()
    assert call(drop=("mu0", "Sigma0"), **st) == 0                          # a carried state replaces (mu0, Sigma0)
    assert call(drop=("mask",)) == 0 and call(drop=tuple(outs)) == 0 and call(drop=("seq_ll", "ll")) == 0
    assert call(drop=("paths", "regimes", "ancestors")) == 0
    assert call() == 0
    assert not any(bool((v.reshape(-1)[:2] == 7).all()) for v in outs.values())


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _model_draws(B, T, dev, seed=31):
    g = torch.Generator().manual_seed(seed)
    N, G = MODEL_PF["num_particles"], MODEL_PF["replicates"]
    return torch.rand(B, G, T, N, generator=g).to(dev), torch.rand(B, G, T, generator=g).to(dev)


def _model_reference(model, a_vae, u, mask, th, ph, dtype=torch.float64, **kw):
    from kvae.kalman import lgssm_ops
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().to(dtype)
    return lgssm_ops.switching_pf_torch(d(dyn.A), d(dyn.B), d(dyn.Q), d(dyn.C[0]), d(kf.R), dyn.prior.transition_matrix.to(dtype),
                                        d(kf.mu0), d(kf.Sigma0), d(a_vae), d(u), d(th), d(ph), mask=mask,
                                        ess_threshold=MODEL_PF["ess_threshold"], **kw)


def model_yardsticks(DEV="cpu"):
    """The float32 restatement against the float64 one on the model-level case, both replaying the float64 run's decisions: the
    numbers MODEL_YARDSTICK holds (the encoder needs the host simulation injected on the CPU)."""
    model, x, mask, u, _ = _model_case(DEV)
    model.eval()
    with torch.no_grad():
        a = model.encode_sequence(x, sample=False)[0]
    th, ph = _model_draws(x.shape[0], x.shape[1], DEV)
    force = decisions_of(_model_reference(model, a, u, mask, th, ph))
    return distances(_model_reference(model, a, u, mask, th, ph, torch.float32, force=force), _model_reference(model, a, u, mask, th, ph, force=force))


def model_level(DEV, K=3, B=3, T=12):
    from kvae import noise
    model, x, mask, u, g = _model_case(DEV, K, B, T)
    model.train()
    dyn = model.kalman_filter.dyn_params
    dyn.tau = 0.37
    before = {k: v.clone() for k, v in model.state_dict().items()}
    nz = dict(eps_a=torch.randn(B * T, model.a_dim, generator=g).to(DEV), eps_z=torch.randn(B, T, model.z_dim, generator=g).to(DEV),
              gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV))
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_before = model(x, u=u)
    th, ph = _model_draws(B, T, DEV)
    with noise.inject(pf_regime=th, pf_resample=ph):
        out = model.particle_filter_regimes(x, u=u, mask=mask.to(DEV), decode=True, **MODEL_PF)
        again = model.particle_filter_regimes(x, u=u, mask=mask.to(DEV), decode=True, **MODEL_PF)
    keys = PER_STEP + ("log_lik_seq", "paths", "path_log_w", "log_lik_seq_mean", "regime_filt_mean", "regimes_map", "a_filt", "a_vae",
                       "n_obs", "x_filt")
    for k in keys:
        assert torch.equal(out[k], again[k]), k
    with noise.inject(**dict(zip(("pf_regime", "pf_resample"), _model_draws(B, T, DEV, seed=32)))):   # other draws: another particle system
        other = model.particle_filter_regimes(x, u=u, mask=mask.to(DEV), **MODEL_PF)
    assert not torch.equal(other["regimes"], out["regimes"]) and "x_filt" not in other
    assert model.training and dyn.tau == 0.37                               # left as they were
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_after = model(x, u=u)
    for k in ("state_probs", "mus_smooth", "Sigmas_smooth", "a_samples", "x_logits"):
        assert torch.equal(fwd_before[k], fwd_after[k]), k
    n, p, N, G = model.z_dim, model.a_dim, MODEL_PF["num_particles"], MODEL_PF["replicates"]
    shapes = dict(log_lik=(B, G, T), log_lik_seq=(B, G), regime_filt=(B, G, T, K), mus_filt=(B, G, T, n), Sigmas_filt=(B, G, T, n, n),
                  ess=(B, G, T), resampled=(B, G, T), regimes=(B, G, T, N), ancestors=(B, G, T, N), levels=(B, G, T), paths=(B, G, N, T),
                  path_log_w=(B, G, N), log_lik_seq_mean=(B,), regime_filt_mean=(B, T, K), regimes_map=(B, T), a_filt=(B, T, p),
                  a_vae=(B, T, p), n_obs=(B,), x_filt=x.shape)
    for k, s in shapes.items():
        assert tuple(out[k].shape) == tuple(s), k
    assert out["regimes_map"].dtype == torch.int64 and torch.equal(out["n_obs"].cpu(), mask.sum(1))
    assert set(out["state"]) == set(STATE + ("regime",))
    c = lambda t: t.detach().cpu().double()
    lse = torch.logsumexp(c(out["log_lik_seq"]), 1) - math.log(G)
    assert float((c(out["log_lik_seq_mean"]) - lse).abs().max()) < 1e-4
    assert float((c(out["regime_filt_mean"]).sum(-1) - 1).abs().max()) < 1e-5
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.encode_sequence(x, sample=False)[0], out["a_vae"])
    model.train()
    ref = _model_reference(model, out["a_vae"], u, mask, th, ph, force=decisions_of(out))
    check_outputs(out, ref, mask, tol=MODEL_TOL, what="model")
    # a stream: two chunks are the bits of the whole
    with noise.inject(pf_regime=th[:, :, :5], pf_resample=ph[:, :, :5]):
        first = model.particle_filter_regimes(x[:, :5], u=u[:, :5], mask=mask[:, :5].to(DEV), **MODEL_PF)
    with noise.inject(pf_regime=th[:, :, 5:], pf_resample=ph[:, :, 5:]):
        rest = model.particle_filter_regimes(x[:, 5:], u=u[:, 5:], mask=mask[:, 5:].to(DEV), state=first["state"], **MODEL_PF)
    for k in ("regime_filt", "log_lik", "regimes", "ancestors", "mus_filt"):
        assert torch.equal(torch.cat([first[k], rest[k]], 2), out[k]), k
    for k in STATE + ("regime",):
        assert torch.equal(rest["state"][k], out["state"][k]), k


def model_errors(DEV):
    import pytest
    lstm = small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.particle_filter_regimes(x)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.particle_filter_regimes(torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 3, 4, device=DEV))
    model = small_model("switching").to(DEV)
    for bad in (dict(mask=torch.ones(2, 4)), dict(u=torch.zeros(2, 4, 4)), dict(num_particles=0), dict(replicates=0), dict(ess_threshold=2.0)):
        with pytest.raises(ValueError):
            model.particle_filter_regimes(x, **bad)


def pf_scores(DEV):
    """particle_filter_scores returns finite floats; with one regime the particle filter and GPB2 are the same exact filter, so
    the gap is zero within the two kernels' bars on log_lik_seq.  The draws are injected from a seeded generator."""
    from kvae import noise
    from kvae.train.prediction import particle_filter_scores
    keys = {"log_lik_per_step_pf", "log_lik_per_step_gpb2", "gpb2_gap_per_step", "pf_std", "regime_tv", "ess_mean"}

    def seeded(G, seed):
        g = torch.Generator().manual_seed(seed)
        return noise.inject(pf_regime=torch.rand(2, G, 6, 64, generator=g), pf_resample=torch.rand(2, G, 6, generator=g))

    model, x, mask, u, _ = _model_case(DEV, B=2, T=6)
    for kw in (dict(), dict(mask=mask[:2, :6].to(DEV), u=u[:2, :6])):
        with seeded(3, 41):
            sc = particle_filter_scores(model, {"images": x[:2, :6]}, num_particles=64, replicates=3, **kw)
        assert set(sc) == keys
        assert all(isinstance(v, float) and math.isfinite(v) for v in sc.values()), sc
        assert 0.0 <= sc["regime_tv"] <= 1.0 and 1.0 <= sc["ess_mean"] <= 64.0 + 1e-3 and sc["pf_std"] >= 0.0
    one, x, mask, u, _ = _model_case(DEV, K=1, B=2, T=6)
    with seeded(2, 42):
        sc = particle_filter_scores(one, x, mask=mask.to(DEV), u=u, num_particles=64, replicates=2)
    n_obs = float(mask.sum())
    bar = x.shape[0] * (MODEL_TOL["log_lik_seq"] + swf_cases.MODEL_TOL["log_lik_seq"]) / n_obs
    print("K = 1: gpb2_gap_per_step", sc["gpb2_gap_per_step"], "bar", bar)
    assert abs(sc["gpb2_gap_per_step"]) <= bar, (sc, bar)
    assert sc["pf_std"] <= 2 * MODEL_TOL["log_lik_seq"] and sc["regime_tv"] == 0.0


def spread_and_gpb2_error(DEV="cpu", G=64, N=64):
    """Reported, not asserted: the spread of log_lik_seq over the replicates next to the GPB2 error of
    log_lik_seq, at the enumerable sizes."""
    rows = []
    for K, T in ((2, 10), (3, 8)):
        args, _ = inputs(4, T, K, seed=6)
        exact = enumerate_paths(tuple(a.double() for a in args))[0].sum(1)
        for thr in (0.5, 1.0):
            th, ph = draws((4, G, T, K, 4, 2, False, N, thr), seed=6)
            seq = restate(args, th, ph, None, thr, dtype=torch.float32, want=("log_lik_seq",))["log_lik_seq"].double()
            rows.append(((K, T, thr), float(seq.std(1).min()), float(seq.std(1).max()), float((seq.mean(1) - exact).abs().max())))
        rows.append(((K, T, "gpb2"),) + swf_cases.gpb2_error(K, T))
    return rows


if __name__ == "__main__":
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "kalman-vae_amd"), str(root), str(root / "tests")]
    torch.set_num_threads(4)
    if sys.argv[1:] == ["spread"]:   # the fixture of `unbiased`: tests/golden/spf_unbiased_spread.npz
        import numpy as np
        out = {}
        for K, T in ((2, 10), (3, 8)):
            for thr in (0.5, 1.0):
                sd, sd_ll, _, _ = measure_spread(K, T, thr)
                out["regime_" + spread_key(K, T, thr)], out["lik_" + spread_key(K, T, thr)] = sd.numpy(), sd_ll.numpy()
        np.savez(root / "tests" / "golden" / "spf_unbiased_spread.npz", **out)
        sys.exit(0)
    print("YARDSTICK", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print("IDENTITY_LOG_W", float(f"{identity_yardstick():.3g}"))
    for case in CASES + [LONG_CASE]:
        margins_hold(case)
    from hostsim.build import build
    from kvae import _native
    _native._set_test_backend(_native.LgssmLib(build()))
    print("MODEL_YARDSTICK", {k: float(f"{v:.3g}") for k, v in model_yardsticks().items()})
    for row in spread_and_gpb2_error():
        print("spread of log_lik_seq (min, max over sequences; |mean - exact|) / GPB2 error", row)
