"""Device-agnostic cases of kvae_lgssm_switching_forecast / lgssm_ops.switching_forecast / KalmanFilter.forecast_regimes /
KVAE.forecast_regimes: run against the host simulation (tests/test_switching_forecast.py: the kernel body of csrc/lgssm_swh.h on
emulated wavefronts) and against the gfx950 library (tests/test_gpu_switching_forecast.py).  The reference is
lgssm_ops.switching_forecast_torch in FLOAT64 on the same float32-rounded numbers; the exactness cases are independent of it
(every regime path enumerated, or the closed-form h-step prediction of a Kalman filter per regime, all in float64)."""
import ctypes as C
import math

import torch

import swf_cases
from golden_util import rel_err

# (B, T, K, n, m, masked, H): swf_cases' shapes with a horizon each - H = 1, H > T (most targets past the end), a medium horizon
# under a mask, n = m = 4, run-time n below the padded 4, a full grid of 8 regimes, hidden origins and a sequence that starts
# hidden, more blocks than a few, and the only long one (the prefetch, origins past 64)
LONG_CASE = (2, 70, 7, 4, 2, True, 9)
CASES = [
    (1, 1, 1, 4, 2, False, 1),
    (3, 2, 2, 4, 2, False, 3),
    (3, 5, 3, 4, 2, True, 4),
    (5, 7, 4, 4, 4, False, 2),
    (2, 9, 5, 3, 2, True, 2),
    (2, 6, 8, 4, 1, False, 5),
    (3, 12, 7, 4, 2, True, 6),
    (17, 3, 3, 4, 2, False, 2),
]
FORE = ("regime_fore", "a_fore", "S_fore", "mus_fore", "Sigmas_fore", "log_lik_fore")   # and levels_fore, which must be equal
# Yardsticks, by the project's standing rule (swf_cases.YARDSTICK): the largest ABSOLUTE distance of switching_forecast_torch in
# FLOAT32 from its float64 run on the same inputs over CASES + [LONG_CASE] with seed 0, per output, measured on the CPU by
# yardsticks() (rerun: python tests/swh_cases.py).  Bars = 4 x: the margin covers another summation order.
YARDSTICK = {"regime_fore": 4.39e-07, "a_fore": 1.41e-06, "S_fore": 7.14e-06, "mus_fore": 8.05e-07, "Sigmas_fore": 1.41e-06,
             "log_lik_fore": 2.26e-06}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
# the model-level case (model_level below: the small switching KVAE's own parameters, Sigma0 = 20 I, R = 0.03^2 I, H = 5),
# measured the same way by model_yardsticks() with the host simulation injected
MODEL_YARDSTICK = {"regime_fore": 1.0e-07, "a_fore": 2.52e-08, "S_fore": 5.53e-08, "mus_fore": 3.77e-07, "Sigmas_fore": 1.59e-05,
                   "log_lik_fore": 3.71e-07}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}
MODEL_H = 5
# what a horizon step shares with the filter's hidden step: the forecast output and the filter output it must agree with
HIDDEN_STEP = (("regime_fore", "regime_pred"), ("a_fore", "a_pred"), ("S_fore", "S"), ("mus_fore", "mus_filt"), ("Sigmas_fore", "Sigmas_filt"))


def inputs(B, T, K, n=4, m=2, masked=False, H=1, seed=0, **kw):
    """swf_cases.inputs with U drawn for T + H steps: ((A, Bm, Q, Cm, R, P, mu0, Sigma0, Y), U_all [B,T+H,m], mask or None), float32."""
    args, mask = swf_cases.inputs(B, T, K, n, m, masked, seed=seed, **kw)
    g = torch.Generator().manual_seed(900000 + 100000 * seed + 1000 * B + 10 * T + K + H)
    tail = torch.randn(B, H, m, generator=g, dtype=torch.float64).float()
    return args[:9], torch.cat([args[9], tail], 1), mask


_REF = {}


def reference(case, seed=0):
    """(args32, U_all, mask, the float64 restatement), computed once per case and shared among the tests; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        from kvae.kalman import lgssm_ops
        args, U, mask = inputs(*case, seed=seed)
        _REF[key] = (args, U, mask, lgssm_ops.switching_forecast_torch(*(a.double() for a in args), U.double(), case[6], mask=mask))
    return _REF[key]


def run(DEV, args, U, H, mask=None, **kw):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_forecast(*(a.to(DEV) for a in args), None if U is None else U.to(DEV), H,
                                        mask=None if mask is None else mask.to(DEV), **kw)


def valid_of(T, H, mask, B, t0=0):
    """[B,T_o,H] bool: the target t + h lies inside the sequence and is observed."""
    step = torch.arange(t0, T)[:, None] + torch.arange(1, H + 1)[None, :]
    inside = (step < T).expand(B, -1, -1)
    return inside if mask is None else inside & (mask[:, step.clamp(max=T - 1)] != 0)


def distances(got, ref):
    c = lambda t: t.detach().cpu().double()
    return {k: float((c(got[k]) - c(ref[k])).abs().max()) for k in FORE}


def check_forecast(got, ref, valid, tol=None, what=""):
    """The forecast outputs of one call against the float64 values under the bars; levels_fore equal; log_lik_fore exactly 0
    wherever there is nothing to score; every output finite."""
    tol = TOL if tol is None else tol
    c = lambda t: t.detach().cpu()
    dist = distances(got, ref)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in FORE + ("levels_fore",):
        assert got[k].shape == ref[k].shape, k
        assert bool(torch.isfinite(c(got[k]).double()).all()), k
    assert got["levels_fore"].dtype == torch.int32 and torch.equal(c(got["levels_fore"]), c(ref["levels_fore"]))
    assert bool((c(got["log_lik_fore"])[~valid] == 0).all())
    return dist


def per_step(DEV, case):
    """1. every (b, t, h) against float64; the filter outputs of the call are the bits of switching_filter's."""
    args, U, mask, ref = reference(case)
    B, T, H = case[0], case[1], case[6]
    got = run(DEV, args, U, H, mask)
    valid = valid_of(T, H, mask, B)
    if mask is not None or H > 1 or T == 1:
        assert bool((~valid).any())
    dist = check_forecast(got, ref, valid, what=str(case))
    flt = swf_cases.run(DEV, args + (U[:, :T],), mask)
    for k in swf_cases.OUTPUTS + ("levels",):
        assert torch.equal(got[k], flt[k]), k
    for k in swf_cases.STATE:
        assert torch.equal(got["state"][k], flt["state"][k]), k
    return dist


def yardsticks():
    """The float32 torch restatement against the float64 one over CASES + [LONG_CASE]: the numbers YARDSTICK holds."""
    from kvae.kalman import lgssm_ops
    worst = {}
    for case in CASES + [LONG_CASE]:
        args, U, mask, ref = reference(case)
        f32 = lgssm_ops.switching_forecast_torch(*args, U, case[6], mask=mask)
        for k, v in distances(f32, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ---- 2. a horizon step is the filter's hidden step ---------------------------------------------------------------------------
def horizon_one_is_the_next_step(DEV, case):
    """Horizon 1 from origin t against step t + 1 of the same call's filter outputs, under the sum of the two bars.  Returns
    whether every compared value was bit-equal (reported in DESIGN.md; regime_pred, a_pred and S do not depend on the
    measurement of step t + 1, log_lik does not on a step that is observed)."""
    args, U, mask, _ = reference(case)
    B, T, H = case[0], case[1], case[6]
    if T < 2:
        return True
    got = run(DEV, args, U, H, mask)
    c = lambda t: t.detach().cpu().double()
    same = True
    for f, s in HIDDEN_STEP[:3] + (("log_lik_fore", "log_lik"),):
        a, b = c(got[f])[:, :T - 1, 0], c(got[s])[:, 1:]
        d = float((a - b).abs().max())
        print("h = 1", case, f, d)
        assert d < TOL[f] + swf_cases.TOL[s], (f, d)
        same = same and torch.equal(a, b)
    return same


def every_horizon_is_a_masked_filter(DEV, case):
    """Every horizon: each origin t against ONE switching_filter call over T + H steps whose mask hides everything after t (the
    frames past the end are zeros): regime_pred, a_pred, S, mus_filt, Sigmas_filt of step t + h, under the sum of the two bars.
    Returns whether every compared value was bit-equal."""
    args, U, mask, _ = reference(case)
    B, T, H = case[0], case[1], case[6]
    assert T <= 12
    got = run(DEV, args, U, H, mask)
    Y = torch.cat([args[8], torch.zeros(B, H, 2)], 1)
    mk = torch.ones(B, T) if mask is None else mask
    c = lambda t: t.detach().cpu().double()
    same, worst = True, {}
    for t in range(T):
        hide = torch.cat([mk[:, :t + 1], torch.zeros(B, T + H - t - 1)], 1)
        flt = swf_cases.run(DEV, args[:8] + (Y, U), hide, want=tuple(s for _, s in HIDDEN_STEP))
        for f, s in HIDDEN_STEP:
            a, b = c(got[f])[:, t], c(flt[s])[:, t + 1:t + 1 + H]
            worst[f] = max(worst.get(f, 0.0), float((a - b).abs().max()))
            same = same and torch.equal(a, b)
    for f, s in HIDDEN_STEP:
        print("masked filter", case, f, worst[f])
        assert worst[f] < TOL[f] + swf_cases.TOL[s], (f, worst[f])
    return same


# ---- 3. exactness, independent of the restatement ------------------------------------------------------------------------------
def _log_density(y, a, S):
    """log N(y; a, S + 1e-6 I): level 0 of the project's Cholesky ladder, as swf_cases._kalman_step."""
    Sj = S + 1e-6 * torch.eye(2, dtype=S.dtype)
    r = y - a
    return -0.5 * ((r.unsqueeze(-2) @ torch.linalg.inv(Sj) @ r.unsqueeze(-1)).reshape(r.shape[:-1]) + torch.logdet(Sj) + 2 * math.log(2 * math.pi))


def _mixture(w, mean, cov):
    """(mean, covariance) of the mixture of the Gaussians (mean [N,d], cov [N,d,d]) under w [N]."""
    m_ = (w[:, None] * mean).sum(0)
    d = mean - m_
    return m_, (w[:, None, None] * (cov + d.unsqueeze(-1) * d.unsqueeze(-2))).sum(0)


def _forecast_of(comp_w, comp_mu, comp_Sig, comp_reg, K, Cm, R, y):
    """The read-outs of one (origin, horizon) from the exact mixture of predicted components (weights, z-mean, z-covariance, the
    regime each is in): the six outputs of FORE; log_lik_fore None without a target frame y."""
    a, S = comp_mu @ Cm.T, Cm @ comp_Sig @ Cm.T + R
    S = 0.5 * (S + S.mT)
    out = {"regime_fore": torch.stack([comp_w[comp_reg == j].sum() for j in range(K)])}
    out["mus_fore"], out["Sigmas_fore"] = _mixture(comp_w, comp_mu, comp_Sig)
    out["a_fore"], out["S_fore"] = _mixture(comp_w, a, S)
    out["log_lik_fore"] = None if y is None else torch.logsumexp(comp_w.log() + _log_density(y, a, S), 0)
    return out


def enumerate_forecast(args, U, H):
    """Origin 0, no mask: the exact forecast of every horizon h = 1 .. H by enumerating all K^(h+1) regime paths of float64
    `args` - s_0 uniform, one Kalman update on a_0 per regime, then one Kalman prediction per path.  {output: [B,H,...]};
    log_lik_fore where the target lies inside the sequence, else 0."""
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y = args
    B, T, _ = Y.shape
    K, n = A.shape[0], A.shape[1]
    rows = {k: [] for k in FORE}
    for b in range(B):
        mus, Sigs, lls = zip(*(swf_cases._kalman_step(mu0[None], Sigma0[None], Y[b, :1], U[b, :1], A[j], Bm[j], Q[j], Cm, R) for j in range(K)))
        mu, Sig, reg = torch.cat(mus), torch.cat(Sigs), torch.arange(K)
        w = torch.softmax(torch.cat(lls) - math.log(K), 0)
        per_h = {k: [] for k in FORE}
        for h in range(1, H + 1):
            w = torch.cat([w * P[reg, j] for j in range(K)])
            mu, Sig = (torch.cat([mu @ A[j].T + U[b, h] @ Bm[j].T for j in range(K)]), torch.cat([A[j] @ Sig @ A[j].T + Q[j] for j in range(K)]))
            reg = torch.arange(K).repeat_interleave(reg.shape[0])
            f = _forecast_of(w, mu, Sig, reg, K, Cm, R, Y[b, h] if h < T else None)
            if f["log_lik_fore"] is None:
                f["log_lik_fore"] = torch.zeros((), dtype=torch.float64)
            for k in FORE:
                per_h[k].append(f[k])
        for k in FORE:
            rows[k].append(torch.stack(per_h[k]))
    return {k: torch.stack(v) for k, v in rows.items()}


def _stochastic(a64):
    """float64 args with the rows of P renormalised: the rows of the float32 prior sum to 1 + 1.5e-8, which an exact computation -
    whose weights are not renormalised at every step - knows nothing of (swf_cases.exact_shared_dynamics)."""
    return a64[:5] + (a64[5] / a64[5].sum(-1, keepdim=True),) + a64[6:]


def _exact_case(K, H, seed, B=2, **kw):
    """(args32, U_all, args64, U64) with T = H + 1: every target of origin 0 lies inside the sequence."""
    args, U, _ = inputs(B, H + 1, K, H=H, seed=seed, **kw)
    return args, U, _stochastic(tuple(a.double() for a in args)), U.double()


def exact_from_origin_zero(DEV, K, H):
    """3a. origin 0, no mask: regime_fore, a_fore, S_fore, mus_fore, Sigmas_fore at every h, and log_lik_fore at h = 1, equal the
    enumeration of all K^(h+1) regime paths - the restatement in float64 at 1e-9 relative, the kernel under the bars of 1.  At
    h >= 2 the distance of log_lik_fore is the GPB2 error of the forecast density: returned, not asserted."""
    from kvae.kalman import lgssm_ops
    args, U, a64, U64 = _exact_case(K, H, seed=3)
    exact = enumerate_forecast(a64, U64, H)
    ref = lgssm_ops.switching_forecast_torch(*a64, U64, H)
    for k in FORE:
        r, e = (ref[k][:, 0], exact[k]) if k != "log_lik_fore" else (ref[k][:, 0, :1], exact[k][:, :1])
        err = rel_err(r, e)
        print("exact from origin 0", (K, H), k, err)
        assert err < 1e-9, (k, err)
    if DEV is not None:
        got = run(DEV, args, U, H)
        for k in FORE:
            g, e = (got[k][:, 0], exact[k]) if k != "log_lik_fore" else (got[k][:, 0, :1], exact[k][:, :1])
            d = float((g.detach().cpu().double() - e).abs().max())
            print("exact from origin 0 on the kernel", (K, H), k, d, TOL[k])
            assert d < TOL[k], (k, d)
    return float((ref["log_lik_fore"][:, 0, 1:] - exact["log_lik_fore"][:, 1:]).abs().max())


def gpb2_forecast_error(K, H):
    """The largest distance of log_lik_fore at h >= 2 from the enumeration: the size of the GPB2 approximation of the forecast
    density (reported, not asserted)."""
    return exact_from_origin_zero(None, K, H)


def regime_forecast_is_the_chain(DEV, case):
    """3b. every origin and horizon: regime_fore[t, h] = regime_filt[t] P^h in float64."""
    from kvae.kalman import lgssm_ops
    args, U, mask, _ = reference(case)
    a64 = _stochastic(tuple(a.double() for a in args))
    H, P = case[6], a64[5]
    ref = lgssm_ops.switching_forecast_torch(*a64, U.double(), H, mask=mask, want=("regime_filt", "regime_fore"))
    chain = torch.stack([ref["regime_filt"] @ torch.linalg.matrix_power(P, h) for h in range(1, H + 1)], 2)
    err = rel_err(ref["regime_fore"], chain)
    print("regime_filt P^h", case, err)
    assert err < 1e-9, err
    d = float((run(DEV, args, U, H, mask, want=("regime_fore",))["regime_fore"].cpu().double() - chain).abs().max())
    print("regime_filt P^h on the kernel", case, d, TOL["regime_fore"])
    assert d < TOL["regime_fore"], d


def fixed_regime_forecast(args, U, H, regimes, uniform_over=None):
    """The exact forecast at every origin and horizon when no regime ever changes (P = I: `regimes` = all of them, each a Kalman
    filter of its own weighted by its likelihood so far) or when it does not matter (shared A, B, Q and K = 1: `regimes` = [0]):
    the closed-form h-step prediction of each filter, float64, no mask.  uniform_over: K where regime_fore is uniform (shared
    dynamics under a doubly stochastic prior)."""
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y = args
    B, T, _ = Y.shape
    K, n = A.shape[0], A.shape[1]
    reg = torch.tensor(regimes)
    out = {k: [] for k in FORE}
    for b in range(B):
        mu, Sig = mu0.expand(len(regimes), n), Sigma0.expand(len(regimes), n, n)
        lj = torch.full((len(regimes),), -math.log(len(regimes)), dtype=torch.float64)
        per_t = {k: [] for k in FORE}
        for t in range(T):
            step = [swf_cases._kalman_step(mu[i:i + 1], Sig[i:i + 1], Y[b, t:t + 1], U[b, t:t + 1], A[k], Bm[k], Q[k], Cm, R) for i, k in enumerate(regimes)]
            mu, Sig, lj = torch.cat([s[0] for s in step]), torch.cat([s[1] for s in step]), lj + torch.cat([s[2] for s in step])
            w, pm, pS = torch.softmax(lj, 0), mu, Sig
            per_h = {k: [] for k in FORE}
            for h in range(1, H + 1):
                pm = torch.stack([A[k] @ pm[i] + Bm[k] @ U[b, t + h] for i, k in enumerate(regimes)])
                pS = torch.stack([A[k] @ pS[i] @ A[k].T + Q[k] for i, k in enumerate(regimes)])
                f = _forecast_of(w, pm, pS, reg, K, Cm, R, Y[b, t + h] if t + h < T else None)
                if uniform_over:
                    f["regime_fore"] = torch.full((K,), 1.0 / K, dtype=torch.float64)
                if f["log_lik_fore"] is None:
                    f["log_lik_fore"] = torch.zeros((), dtype=torch.float64)
                for k in FORE:
                    per_h[k].append(f[k])
            for k in FORE:
                per_t[k].append(torch.stack(per_h[k]))
        for k in FORE:
            out[k].append(torch.stack(per_t[k]))
    return {k: torch.stack(v) for k, v in out.items()}


def exact_fixed_regimes(DEV, what, K=3, T=6, H=4, B=2):
    """3c / 3d. P = I ("identity"), shared A, B, Q ("shared") and K = 1 ("single"): every output, log_lik_fore included, equals
    fixed_regime_forecast at every origin and horizon - the restatement in float64 at 1e-9 relative, the kernel under the bars
    of 1 - and with P = I no NaN or inf appears on the kernel."""
    from kvae.kalman import lgssm_ops
    kw = {"identity": dict(p_stay=1.0), "shared": dict(shared=True), "single": dict()}[what]
    K = 1 if what == "single" else K
    args, U, _ = inputs(B, T, K, H=H, seed={"identity": 4, "shared": 5, "single": 6}[what], **kw)
    a64, U64 = tuple(a.double() for a in args), U.double()
    if what == "identity":
        assert bool((a64[5] == torch.eye(K, dtype=torch.float64)).all())
    if what == "shared":
        a64 = _stochastic(a64)
    exact = fixed_regime_forecast(a64, U64, H, list(range(K)) if what == "identity" else [0], uniform_over=K if what == "shared" else None)
    ref = lgssm_ops.switching_forecast_torch(*a64, U64, H)
    for k in FORE:
        err = rel_err(ref[k], exact[k])
        print("exact,", what, k, err)
        assert err < 1e-9, (k, err)
    if DEV is None:
        return
    got = run(DEV, args, U, H)
    for k in FORE + ("levels_fore",):
        assert bool(torch.isfinite(got[k].cpu().double()).all()), k
    for k in FORE:
        d = float((got[k].cpu().double() - exact[k]).abs().max())
        print("exact,", what, "on the kernel", k, d, TOL[k])
        assert d < TOL[k], (k, d)


# ---- 4. streaming and origins --------------------------------------------------------------------------------------------------
def streaming(DEV, case):
    """Chunks of (1, T - 1) and of (3, 4, rest), each continuing from the state of the one before with its slice [chunk + H] of
    U: every forecast output but log_lik_fore is the bits of the whole-sequence call at every origin, log_lik_fore wherever the
    target lies inside the chunk, and the final state is the bits of the whole call's."""
    args, U, mask, _ = reference(case)
    assert mask is not None
    T, H = case[1], case[6]
    whole = run(DEV, args, U, H, mask)
    for sizes in ((1, T - 1), (3, 4, T - 7)):
        assert sum(sizes) == T and all(s > 0 for s in sizes)
        state, t0 = None, 0
        for s in sizes:
            part = run(DEV, args[:8] + (args[8][:, t0:t0 + s],), U[:, t0:t0 + s + H], H, mask[:, t0:t0 + s], state=state)
            for k in FORE + ("levels_fore",):
                a, b = part[k], whole[k][:, t0:t0 + s]
                if k == "log_lik_fore":
                    inside = (torch.arange(s)[:, None] + torch.arange(1, H + 1)[None, :] < s).to(a.device).expand_as(a)
                    assert bool(inside.any()) or s == 1
                    a, b = a[inside], b[inside]
                assert torch.equal(a, b), (sizes, t0, k)
            state, t0 = part["state"], t0 + s
        for k in swf_cases.STATE:
            assert torch.equal(state[k], whole["state"][k]), (sizes, "state", k)


def last_origin(DEV, case):
    """origins="last" gives the bits of the last origin of "all"."""
    args, U, mask, _ = reference(case)
    H = case[6]
    whole, last = run(DEV, args, U, H, mask), run(DEV, args, U, H, mask, origins="last")
    for k in FORE + ("levels_fore",):
        assert last[k].shape[1] == 1 and torch.equal(last[k][:, 0], whole[k][:, -1]), k
    for k in swf_cases.OUTPUTS:
        assert torch.equal(last[k], whole[k]), k


# ---- 5. routing and the C ABI ----------------------------------------------------------------------------------------------------
def partial_outputs(DEV, case):
    """Each output alone gives the bits of the full call, nothing else is returned; two full calls give the same bits."""
    from kvae.kalman import lgssm_ops
    args, U, mask, _ = reference(case)
    H = case[6]
    full, again = run(DEV, args, U, H, mask), run(DEV, args, U, H, mask)
    for k in lgssm_ops._SWH_OUTPUTS:
        one = run(DEV, args, U, H, mask, want=(k,))
        assert [n for n, v in one.items() if v is not None] == [k], k
        for a, b, c in ((one, full, k), (again, full, k)):
            if k == "state":
                assert all(torch.equal(a["state"][s], b["state"][s]) for s in swf_cases.STATE)
            else:
                assert torch.equal(a[c], b[c]), k


def routing(DEV):
    """K = 9 and n = 5 are outside the kernel: the Python layer takes switching_forecast_torch (float32 there), impl="hip" raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    ok = torch.zeros(1, device=DEV)
    S = lgssm_ops.switching_forecast_supported
    assert S(8, 4, 4, 2, ok) and S(1, 1, 1, 2, ok)
    assert not S(9, 4, 4, 2, ok) and not S(3, 5, 2, 2, ok) and not S(3, 4, 5, 2, ok) and not S(3, 4, 2, 3, ok) and not S(3, 4, 2, 2, ok.double())
    for case in ((2, 4, 9, 4, 2, False, 3), (2, 4, 3, 5, 2, True, 2)):
        args, U, mask = inputs(*case, seed=8)
        got = run(DEV, args, U, case[6], mask)
        ref = lgssm_ops.switching_forecast_torch(*(a.double() for a in args), U.double(), case[6], mask=mask)
        f32 = lgssm_ops.switching_forecast_torch(*args, U, case[6], mask=mask)
        for k in FORE:
            assert got[k].dtype == torch.float32
            assert rel_err(got[k].cpu(), ref[k]) < 1e-4, k
            if DEV == "cpu":
                assert torch.equal(got[k], f32[k]), k                      # the restatement itself
        with pytest.raises(ValueError, match="impl='hip'"):
            run(DEV, args, U, case[6], mask, impl="hip")
    args, U, mask = inputs(2, 3, 2, H=2)
    for bad in (dict(want=("regimes",)), dict(impl="kernel"), dict(origins="first")):
        with pytest.raises(ValueError):
            run(DEV, args, U, 2, mask, **bad)
    for U_bad, H_bad in ((U, 0), (U[:, :-1], 2), (U, 3)):
        with pytest.raises(ValueError):
            run(DEV, args, U_bad, H_bad, mask)
    forced, zeros = run(DEV, args, U, 2, mask, impl="torch"), run(DEV, args, None, 2, mask, want=("a_fore",))
    assert rel_err(forced["a_fore"].cpu(), run(DEV, args, U, 2, mask)["a_fore"].cpu()) < 1e-4
    assert zeros["a_fore"].shape == forced["a_fore"].shape


def c_abi(lib, DEV):
    """Error codes of include/kvae_lgssm.h, and not a byte of any output written on error."""
    from kvae import _native as N
    B, T, K, n, m, H = 2, 3, 3, 4, 2, 2
    args, U, mask = inputs(B, T, K, n, m, True, H)
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), u=U[:, :T].contiguous().to(DEV), mask=mask.to(DEV))
    top = dict(u_all=U.contiguous().to(DEV))
    # buffers large enough for the shapes the failing calls claim (K = 9, n = 5, H = 3) too
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    outs = dict(regime_filt=big(B, T, 9), ll=big(B, T), seq_ll=big(B), a_pred=big(B, T, 3), out_log_w=big(B, 9))
    fore = dict(hist_lw=big(B, T, 9), hist_mu=big(B, T, 9, 5), hist_Sigma=big(B, T, 9, 5, 5), regime_fore=big(B, T, 3, 9), a_fore=big(B, T, 3, 3),
                S_fore=big(B, T, 3, 3, 3), mus_fore=big(B, T, 3, 5), Sigmas_fore=big(B, T, 3, 5, 5), ll_fore=big(B, T, 3),
                levels_fore=big(B, T, 3, dt=torch.int32))

    def call(drop=(), H=H, t0=0, **kw):
        fp = N.SwhProblem()
        pr = fp.filt
        pr.B, pr.T, pr.K, pr.n, pr.m, pr.p = B, T, K, n, m, 2
        fp.H, fp.t0 = H, t0
        for k, v in list(ins.items()) + list(outs.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in list(top.items()) + list(fore.items()):
            if k not in drop:
                setattr(fp, k, v.data_ptr())
        for k, v in kw.items():
            setattr(pr, k, v)
        rc = lib.dll.kvae_lgssm_switching_forecast(C.byref(fp), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool((v == 7).all()) for v in list(outs.values()) + list(fore.values()))
    assert lib.dll.kvae_lgssm_switching_forecast(None, None) == 2
    for k in names + ("u", "u_all", "hist_lw", "hist_mu", "hist_Sigma"):
        assert call(drop=(k,)) == 2, k                                      # KVAE_ERR_NULL
    assert call(drop=("ll",)) == 2                                          # seq_ll reads ll
    for kw in (dict(B=0), dict(T=0), dict(H=0), dict(H=-1)):
        assert call(**kw) == 1, kw                                          # KVAE_ERR_DIMS
    for kw in (dict(K=9), dict(K=0), dict(n=5), dict(m=5), dict(p=3), dict(t0=-1), dict(t0=T)):
        assert call(**kw) == 4, kw                                          # KVAE_ERR_ARG
    assert untouched()
    assert call(drop=("mask",)) == 0 and call(t0=T - 1) == 0 and call(drop=tuple(outs) + tuple(k for k in fore if not k.startswith("hist"))) == 0
    assert call() == 0
    assert not any(bool((v.reshape(-1)[:2] == 7).all()) for v in list(outs.values()) + list(fore.values()))


# ---- 6. model level -----------------------------------------------------------------------------------------------------------------
def _model_case(DEV, B=3, T=12, H=MODEL_H):
    model, x, mask, u, g = swf_cases._model_case(DEV, 3, B, T)
    u_all = torch.cat([u, (0.3 * torch.randn(B, H, model.u_dim, generator=g)).to(DEV)], 1)
    return model, x, mask, u_all, g


def _model_reference(model, a_vae, u_all, mask, H, dtype=torch.float64):
    from kvae.kalman import lgssm_ops
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().to(dtype)
    return lgssm_ops.switching_forecast_torch(d(dyn.A), d(dyn.B), d(dyn.Q), d(dyn.C[0]), d(kf.R), dyn.prior.transition_matrix.to(dtype),
                                              d(kf.mu0), d(kf.Sigma0), d(a_vae), d(u_all), H, mask=mask)


def model_yardsticks(DEV="cpu"):
    """The float32 restatement against the float64 one on the model-level case: the numbers MODEL_YARDSTICK holds (the encoder
    needs the host simulation injected on the CPU)."""
    model, x, mask, u_all, _ = _model_case(DEV)
    model.eval()
    with torch.no_grad():
        a = model.encode_sequence(x, sample=False)[0]
    return distances(_model_reference(model, a, u_all, mask, MODEL_H, torch.float32), _model_reference(model, a, u_all, mask, MODEL_H))


def model_level(DEV, B=3, T=12, H=MODEL_H):
    from kvae import noise
    model, x, mask, u_all, g = _model_case(DEV, B, T, H)
    K = model.K
    model.train()
    dyn = model.kalman_filter.dyn_params
    dyn.tau = 0.37
    before = {k: v.clone() for k, v in model.state_dict().items()}
    nz = dict(eps_a=torch.randn(B * T, model.a_dim, generator=g).to(DEV), eps_z=torch.randn(B, T, model.z_dim, generator=g).to(DEV),
              gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV))
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_before = model(x, u=u_all[:, :T])
    out = model.forecast_regimes(x, H, u=u_all, mask=mask.to(DEV), decode=True)
    again = model.forecast_regimes(x, H, u=u_all, mask=mask.to(DEV), decode=True)
    for k in FORE + ("levels_fore", "regimes_fore", "valid", "a_vae", "n_obs", "x_fore") + swf_cases.OUTPUTS:
        assert torch.equal(out[k], again[k]), k
    assert model.training and dyn.tau == 0.37                               # left as they were
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_after = model(x, u=u_all[:, :T])
    for k in ("state_probs", "mus_smooth", "Sigmas_smooth", "a_samples", "x_logits"):
        assert torch.equal(fwd_before[k], fwd_after[k]), k
    n, p = model.z_dim, model.a_dim
    shapes = dict(regime_fore=(B, T, H, K), regimes_fore=(B, T, H), a_fore=(B, T, H, p), S_fore=(B, T, H, p, p), mus_fore=(B, T, H, n),
                  Sigmas_fore=(B, T, H, n, n), log_lik_fore=(B, T, H), levels_fore=(B, T, H), valid=(B, T, H), a_vae=(B, T, p), n_obs=(B,),
                  x_fore=(B, H) + tuple(x.shape[2:]), regime_filt=(B, T, K), log_lik=(B, T))
    for k, s in shapes.items():
        assert tuple(out[k].shape) == tuple(s), k
    rf = out["regime_fore"]
    assert out["regimes_fore"].dtype == torch.int64
    assert torch.equal(out["regimes_fore"], (rf == rf.max(-1, keepdim=True).values).to(torch.int8).argmax(-1))
    valid = valid_of(T, H, mask, B)
    assert out["valid"].dtype == torch.bool and torch.equal(out["valid"].cpu(), valid) and bool(valid.any()) and bool((~valid).any())
    flt = model.filter_regimes(x, u=u_all[:, :T], mask=mask.to(DEV))
    for k in swf_cases.OUTPUTS + ("levels",):
        assert torch.equal(out[k], flt[k]), k
    ref = _model_reference(model, out["a_vae"], u_all, mask, H)
    check_forecast(out, ref, valid, tol=MODEL_TOL, what="model")
    # the online case: the last origin after a carried state, and no u at all
    first = model.forecast_regimes(x[:, :5], H, u=u_all[:, :5 + H], mask=mask[:, :5].to(DEV))
    rest = model.forecast_regimes(x[:, 5:], H, u=u_all[:, 5:], mask=mask[:, 5:].to(DEV), state=first["state"], origins="last")
    for k in ("regime_fore", "a_fore", "S_fore", "mus_fore", "regimes_fore"):
        assert rest[k].shape[1] == 1 and torch.equal(rest[k][:, 0], out[k][:, -1]), k
    free = model.forecast_regimes(x, 2)
    assert free["a_fore"].shape == (B, T, 2, p) and "x_fore" not in free and bool(free["valid"][:, :T - 2].all())


def model_errors(DEV):
    import pytest
    lstm = swf_cases.small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.forecast_regimes(x, 2)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.forecast_regimes(torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 5, 4, device=DEV), 2)
    model = swf_cases.small_model("switching").to(DEV)
    for bad in (dict(mask=torch.ones(2, 4)), dict(u=torch.zeros(2, 3, 4)), dict(u=torch.zeros(2, 5, 3)), dict(origins="first")):
        with pytest.raises(ValueError):
            model.forecast_regimes(x, 2, **bad)
    with pytest.raises(ValueError):
        model.forecast_regimes(x, 0)


def forecast_scores(DEV):
    from kvae.train.prediction import forecast_scores as scores
    model, x, mask, u_all, _ = _model_case(DEV)
    T, H = x.shape[1], MODEL_H
    for kw, mk in ((dict(), None), (dict(mask=mask.to(DEV), u=u_all), mask)):
        sc = scores(model, {"images": x}, H, **kw)
        assert set(sc) == {"mse", "mse_naive", "log_lik", "nis_mean", "count"}
        for k, v in sc.items():
            assert isinstance(v, list) and len(v) == H, k
            assert all(math.isfinite(f) for f in v), (k, v)
        assert sc["count"] == valid_of(T, H, mk, x.shape[0]).sum((0, 1)).tolist()
        assert all(isinstance(f, float) for k in ("mse", "mse_naive", "log_lik", "nis_mean") for f in sc[k])
        assert all(f >= 0 for f in sc["mse"] + sc["mse_naive"] + sc["nis_mean"])


if __name__ == "__main__":
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "kalman-vae_amd"), str(root), str(root / "tests")]
    torch.set_num_threads(4)
    print("YARDSTICK", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    from hostsim.build import build
    from kvae import _native
    lib = _native.LgssmLib(build())
    _native._set_test_backend(lib)
    print("MODEL_YARDSTICK", {k: float(f"{v:.3g}") for k, v in model_yardsticks().items()})
    for K, H in ((2, 6), (3, 4)):
        print("GPB2 error of log_lik_fore at h >= 2 (abs)", (K, H), gpb2_forecast_error(K, H))
    lib.dll.kvae_hostsim_wave_emu(1)
    worst = {}
    for case in CASES + [LONG_CASE]:
        for k, v in per_step("cpu", case).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("emulated kernel", {k: float(f"{v:.3g}") for k, v in worst.items()})
    print("h = 1 bit-equal to the filter's next step:", all(horizon_one_is_the_next_step("cpu", c) for c in CASES + [LONG_CASE]))
    print("every horizon bit-equal to a masked filter:", all(every_horizon_is_a_masked_filter("cpu", c) for c in CASES))
