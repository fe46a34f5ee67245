"""Device-agnostic cases of kvae_lgssm_switching_filter / lgssm_ops.switching_filter / KalmanFilter.filter_regimes /
KVAE.filter_regimes: run against the host simulation (tests/test_switching_filter.py: the kernel body of csrc/lgssm_swf.h on
emulated wavefronts) and against the gfx950 library (tests/test_gpu_switching_filter.py).  The reference is
lgssm_ops.switching_filter_torch in FLOAT64 on the same float32-rounded numbers; the exactness cases are independent of it (every
regime path enumerated, each a float64 Kalman filter of its own)."""
import ctypes as C
import math

import torch

from golden_util import rel_err

# (B, T, K, n, m, masked) of the per-step parity, both tiers: every K whose padding differs (1, 2, 3, 4, 5, 7, a full grid of 8),
# T = 1, run-time dims below the padded 4 (n = 3, m = 2, m = 1) and at it (n = m = 4), more sequences than a wavefront packs
LONG_CASE = (2, 70, 7, 4, 2, True)   # the only long one: the prefetch over many steps, T past the 64-lane stride of the sequence sums
CASES = [
    (1, 1, 1, 4, 2, False),
    (3, 2, 2, 4, 2, False),
    (3, 5, 3, 4, 2, True),
    (5, 7, 4, 4, 4, False),
    (2, 9, 5, 3, 2, True),
    (3, 12, 7, 4, 2, True),
    (2, 6, 8, 4, 1, False),
    (17, 3, 3, 4, 2, False),
]
OUTPUTS = ("regime_filt", "regime_pred", "log_lik", "log_lik_seq", "a_pred", "S", "mus_filt", "Sigmas_filt")
STATE = ("log_w", "mu", "Sigma")
# Yardsticks, by the project's standing rule (parity_cases.RNN_YARDSTICK, regime_decode_cases.YARDSTICK): the largest ABSOLUTE
# distance of switching_filter_torch in FLOAT32 from its float64 run on the same inputs - per (b, t) slice for the per-step
# outputs, per sequence for log_lik_seq and the state - over CASES + [LONG_CASE] with seed 0, measured on the CPU by yardsticks()
# (rerun: python tests/swf_cases.py).  Bars = 4 x: the margin covers another summation order.
YARDSTICK = {"regime_filt": 5.64e-7, "regime_pred": 4.39e-7, "log_lik": 2.26e-6, "log_lik_seq": 1.84e-5, "a_pred": 1.35e-6, "S": 3.17e-6,
             "mus_filt": 8.28e-7, "Sigmas_filt": 2.34e-6, "state_log_w": 6.51e-6, "state_mu": 9.81e-7, "state_Sigma": 3.36e-7}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
# the model-level case (model_level below: the small switching KVAE's own parameters, Sigma0 = 20 I, R = 0.03^2 I), measured the
# same way by model_yardsticks() with the host simulation injected
MODEL_YARDSTICK = {"regime_filt": 1.3e-7, "regime_pred": 1.0e-7, "log_lik": 2.32e-7, "log_lik_seq": 1.24e-6, "a_pred": 1.94e-8, "S": 2.17e-8,
                   "mus_filt": 1.97e-7, "Sigmas_filt": 8.93e-6, "state_log_w": 3.8e-7, "state_mu": 3.42e-7, "state_Sigma": 6.71e-6}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}
GAP = 1e-4   # a float64 decision gap (best minus runner-up regime_filt) above which float32 must take the same decision
             # (regime_decode_cases.GAP)
EXCUSED = 0.05   # at most this share of (b, t) may fall under GAP


def prior(K, p_stay=0.8):
    from kvae.kalman.switch_dyn_param import StickyRegimePrior
    return StickyRegimePrior(K, p_stay).transition_matrix


def dynamics(K, n, m, g):
    """Stable, regime-distinct dynamics in float64: A_k a rotation of its own angle and sign in the (0, 1) plane scaled by
    0.97 - 0.03 k, a slower counter-rotation in the (2, 3) plane; Q_k of its own size; a dense C; moderate observation noise."""
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    A = torch.zeros(K, n, n, dtype=torch.float64)
    for k in range(K):
        th = (0.15 + 0.25 * k) * (1.0 if k % 2 == 0 else -1.0)
        sc = 0.97 - 0.03 * k
        A[k] = 0.9 * sc * torch.eye(n, dtype=torch.float64)
        c, s = math.cos(th), math.sin(th)
        A[k, :2, :2] = sc * torch.tensor([[c, -s], [s, c]], dtype=torch.float64)
        if n >= 4:
            c, s = math.cos(-0.7 * th), math.sin(-0.7 * th)
            A[k, 2:4, 2:4] = 0.9 * sc * torch.tensor([[c, -s], [s, c]], dtype=torch.float64)
    Bm = 0.3 * r(K, n, m)
    Q = torch.stack([(0.02 + 0.015 * k) * torch.eye(n, dtype=torch.float64) + 0.004 * (lambda M: M @ M.T)(r(n, n)) for k in range(K)])
    Cm = 0.8 * r(2, n)
    R = 0.05 * torch.eye(2, dtype=torch.float64)
    mu0 = 0.1 * r(n)
    Sigma0 = 0.5 * torch.eye(n, dtype=torch.float64)
    return A, Bm, Q, Cm, R, mu0, Sigma0


def inputs(B, T, K, n=4, m=2, masked=False, seed=0, p_stay=0.8, shared=False):
    """(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U) drawn in float64 and rounded through float32 (the float64 reference starts from the
    same numbers), and mask [B,T] or None.  Y is a draw from the model itself with a regime change every few steps, so that the
    regimes can be told apart.  shared: every regime gets regime 0's A, B, Q."""
    g = torch.Generator().manual_seed(100000 * seed + 1000 * B + 10 * T + K)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    A, Bm, Q, Cm, R, mu0, Sigma0 = dynamics(K, n, m, g)
    if shared:
        A, Bm, Q = (M[:1].expand_as(M).clone() for M in (A, Bm, Q))
    U = r(B, T, m)
    LQ, L0, LR = torch.linalg.cholesky(Q), torch.linalg.cholesky(Sigma0), torch.linalg.cholesky(R)
    Y = torch.zeros(B, T, 2, dtype=torch.float64)
    for b in range(B):
        s = int(torch.randint(K, (1,), generator=g))
        z = mu0 + L0 @ r(n)
        for t in range(T):
            if t > 0 and float(torch.rand(1, generator=g)) > 0.8:
                s = int(torch.randint(K, (1,), generator=g))
            z = A[s] @ z + Bm[s] @ U[b, t] + LQ[s] @ r(n)
            Y[b, t] = Cm @ z + LR @ r(2)
    mask = None
    if masked:
        bt = torch.arange(B)[:, None] + torch.arange(T)[None, :]
        mask = (bt % 3 != 1).float()   # sequence 1 starts hidden; no sequence is hidden throughout
        if B * T <= 20:                # a hidden first step leaves regime_filt exactly uniform: a tie, which the gap rule has to
            mask[:, 0] = 1.0           # excuse - one such step is more than 5 % of a case this small
    return tuple(t.float() for t in (A, Bm, Q, Cm, R, prior(K, p_stay).double(), mu0, Sigma0, Y, U)), mask


_REF = {}


def reference(case, seed=0):
    """(args32, mask, the float64 restatement), computed once per case and shared among the tests; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        from kvae.kalman import lgssm_ops
        args, mask = inputs(*case, seed=seed)
        _REF[key] = (args, mask, lgssm_ops.switching_filter_torch(*(a.double() for a in args), mask=mask))
    return _REF[key]


def distances(got, ref):
    """Largest absolute distance of every output from the float64 run: the per-step outputs per (b, t), log_lik_seq and the
    state per sequence (the maximum over slices of a max-norm is the max-norm)."""
    c = lambda t: t.detach().cpu().double()
    out = {k: float((c(got[k]) - ref[k]).abs().max()) for k in OUTPUTS}
    for k in STATE:
        out["state_" + k] = float((c(got["state"][k]) - ref["state"][k]).abs().max())
    return out


def check_outputs(got, ref, mask, tol=None, what=""):
    """Every output of one call against the float64 run under the bars; levels exactly; regimes wherever the float64 gap says the
    decision is not a toss-up, which must be nearly everywhere; on hidden steps log_lik = 0 and regime_filt = regime_pred."""
    tol = TOL if tol is None else tol
    c = lambda t: t.detach().cpu()
    dist = distances(got, ref)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in OUTPUTS + ("levels",):
        assert got[k].shape == ref[k].shape, k
        assert bool(torch.isfinite(c(got[k]).double()).all()), k
    assert got["levels"].dtype == torch.int32 and torch.equal(c(got["levels"]), ref["levels"])
    rf64 = ref["regime_filt"]
    K = rf64.shape[-1]
    mine = c(got["regime_filt"]).argmax(-1) if "regimes" not in got else c(got["regimes"])
    if K > 1:
        top = rf64.topk(2, dim=-1).values
        decided = (top[..., 0] - top[..., 1]) > GAP
        excused = float((~decided).double().mean())
        print(what, "regimes: share under the gap", excused)
        assert excused <= EXCUSED, excused
        assert torch.equal(mine[decided], rf64.argmax(-1)[decided])
    if mask is not None:
        hidden = mask == 0
        assert bool(hidden.any())
        assert bool((c(got["log_lik"])[hidden] == 0).all())
        # equal in exact arithmetic; each is within its own bar of the float64 value
        gap = (c(got["regime_filt"]) - c(got["regime_pred"])).abs()[hidden]
        assert float(gap.max()) < tol["regime_filt"] + tol["regime_pred"], float(gap.max())
    return dist


def run(DEV, args, mask=None, **kw):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_filter(*(a.to(DEV) for a in args), mask=None if mask is None else mask.to(DEV), **kw)


def per_step(DEV, case):
    args, mask, ref = reference(case)
    got = run(DEV, args, mask)
    return check_outputs(got, ref, mask, what=str(case))


def yardsticks():
    """The float32 torch restatement against the float64 one over CASES + [LONG_CASE]: the numbers YARDSTICK holds."""
    from kvae.kalman import lgssm_ops
    worst = {}
    for case in CASES + [LONG_CASE]:
        args, mask, ref = reference(case)
        f32 = lgssm_ops.switching_filter_torch(*args, mask=mask)
        for k, v in distances(f32, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ---- exactness: every regime path enumerated, independent of the restatement -------------------------------------------------
def _kalman_step(mu, Sig, y, u, A, Bm, Q, Cm, R):
    """One float64 predict + update of a batch [N, ...] under ONE regime's (A, Bm, Q); the density is N(y; C mu_pred, S + 1e-6 I),
    level 0 of the project's Cholesky ladder (lgssm_ops.safe_cholesky_items), which every well-conditioned S takes."""
    mp = mu @ A.T + u @ Bm.T
    Sp = A @ Sig @ A.T + Q
    S = Cm @ Sp @ Cm.T + R
    S = 0.5 * (S + S.mT)
    r = y - mp @ Cm.T
    Sj = S + 1e-6 * torch.eye(2, dtype=S.dtype)
    ll = -0.5 * ((r.unsqueeze(-2) @ torch.linalg.inv(Sj) @ r.unsqueeze(-1)).reshape(-1) + torch.logdet(Sj) + 2 * math.log(2 * math.pi))
    Kg = Sp @ Cm.T @ torch.linalg.inv(S)
    mf = mp + (Kg @ r.unsqueeze(-1)).squeeze(-1)
    IKC = torch.eye(mu.shape[-1], dtype=S.dtype) - Kg @ Cm
    Sf = IKC @ Sp @ IKC.mT + Kg @ R @ Kg.mT
    return mf, 0.5 * (Sf + Sf.mT), ll


def enumerate_paths(args):
    """Exact log p(a_t | a_{0:t-1}) [B,T] and p(s_t | a_{0:t}) [B,T,K] of float64 `args` by enumerating every regime prefix:
    s_0 uniform, s_t | s_{t-1} ~ P, one Kalman filter per prefix, its joint log p(a_{0:t}, s_{0:t}) carried along."""
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    B, T, _ = Y.shape
    K, n = A.shape[0], A.shape[1]
    ll_out, rf_out = torch.zeros(B, T, dtype=torch.float64), torch.zeros(B, T, K, dtype=torch.float64)
    for b in range(B):
        mu, Sig = mu0.expand(1, n), Sigma0.expand(1, n, n)
        lj, last = torch.zeros(1, dtype=torch.float64), None
        prev_total = torch.zeros((), dtype=torch.float64)
        for t in range(T):
            N = mu.shape[0]
            mus, Sigs, ljs, lasts = [], [], [], []
            for j in range(K):
                mf, Sf, ll = _kalman_step(mu, Sig, Y[b, t].expand(N, -1), U[b, t].expand(N, -1), A[j], Bm[j], Q[j], Cm, R)
                lp = torch.full((N,), -math.log(K), dtype=torch.float64) if t == 0 else P[last, j].log()
                mus.append(mf), Sigs.append(Sf), ljs.append(lj + lp + ll), lasts.append(torch.full((N,), j, dtype=torch.long))
            mu, Sig, lj, last = torch.cat(mus), torch.cat(Sigs), torch.cat(ljs), torch.cat(lasts)
            total = torch.logsumexp(lj, 0)
            ll_out[b, t] = total - prev_total
            prev_total = total
            for j in range(K):
                rf_out[b, t, j] = torch.logsumexp(lj[last == j], 0).sub(total).exp() if bool((last == j).any()) else 0.0
    return ll_out, rf_out


def exact_first_steps(K, T, B=2):
    """GPB2 carries K Gaussians and the exact posterior after step 0 has K components, so steps 0 and 1 are exact for any K."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=3)
    args = tuple(a.double() for a in args)
    got = lgssm_ops.switching_filter_torch(*args)
    ll, rf = enumerate_paths(args)
    e_ll, e_rf = rel_err(got["log_lik"][:, :2], ll[:, :2]), rel_err(got["regime_filt"][:, :2], rf[:, :2])
    print("exact through t = 1", (K, T), e_ll, e_rf)
    assert e_ll < 1e-9 and e_rf < 1e-9, (e_ll, e_rf)
    return ll, rf, got


def exact_identity_prior(K=3, T=6, B=2):
    """P = I: a regime never changes, every column of the pair grid has one live pair, nothing is collapsed - exact at every
    step; and the zeros of P (log P = -inf) leave every finite output finite."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=4, p_stay=1.0)
    args = tuple(a.double() for a in args)
    assert bool((args[5] == torch.eye(K, dtype=torch.float64)).all())
    got = lgssm_ops.switching_filter_torch(*args)
    ll, rf = enumerate_paths(args)
    e_ll, e_rf = rel_err(got["log_lik"], ll), rel_err(got["regime_filt"], rf)
    print("P = I", e_ll, e_rf)
    assert e_ll < 1e-9 and e_rf < 1e-9, (e_ll, e_rf)
    for k in OUTPUTS:
        assert bool(torch.isfinite(got[k]).all()), k
    assert bool(torch.isfinite(got["state"]["mu"]).all()) and bool(torch.isfinite(got["state"]["Sigma"]).all())
    assert not bool(torch.isnan(got["state"]["log_w"]).any())
    return args


def exact_shared_dynamics(K=3, T=6, B=2):
    """All regimes share A, B, Q: every pair's Kalman step is the same, the mixture is one Gaussian - exact at every step, equal
    to a single filter, with regime_filt uniform (the sticky prior is doubly stochastic)."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=5, shared=True)
    args = tuple(a.double() for a in args)
    # the rows of the float32 prior sum to 1 + 1.5e-8, which a single filter knows nothing of: renormalised in float64
    args = args[:5] + (args[5] / args[5].sum(-1, keepdim=True),) + args[6:]
    got = lgssm_ops.switching_filter_torch(*args)
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    ll = torch.zeros(B, T, dtype=torch.float64)
    mu, Sig = mu0.expand(B, -1), Sigma0.expand(B, -1, -1)
    for t in range(T):
        mu, Sig, ll[:, t] = _kalman_step(mu, Sig, Y[:, t], U[:, t], A[0], Bm[0], Q[0], Cm, R)
    e_ll = rel_err(got["log_lik"], ll)
    e_rf = rel_err(got["regime_filt"], torch.full((B, T, K), 1.0 / K, dtype=torch.float64))
    e_mu = rel_err(got["mus_filt"][:, -1], mu)
    print("shared dynamics", e_ll, e_rf, e_mu)
    assert e_ll < 1e-9 and e_rf < 1e-9 and e_mu < 1e-9, (e_ll, e_rf, e_mu)


def gpb2_error(K, T, B=4):
    """log_lik_seq of the float64 restatement against full enumeration: the size of the GPB2 approximation (reported, not asserted)."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=6)
    args = tuple(a.double() for a in args)
    got = lgssm_ops.switching_filter_torch(*args)
    ll, _ = enumerate_paths(args)
    return float((got["log_lik_seq"] - ll.sum(1)).abs().max()), float(ll.sum(1).abs().max())


def identity_prior_on_kernel(DEV, K=3, T=6, B=2):
    """The zeros of P on the kernel: no NaN or inf in any finite output, and the float64 run's numbers under the bars."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=4, p_stay=1.0)
    got = run(DEV, args)
    ref = lgssm_ops.switching_filter_torch(*(a.double() for a in args))
    check_outputs(got, ref, None, what="P = I on the kernel")


# ---- agreement with the existing filter -------------------------------------------------------------------------------------
def _kalman_filter(args, DEV):
    """A KalmanFilter over switching dynamics holding `args`' regimes (R = r I, as the module builds it)."""
    from kvae.kalman.kalman_filter import KalmanFilter
    from kvae.kalman.switch_dyn_param import StickyRegimePrior, SwitchingDynamicsParameter
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    K = A.shape[0]
    dyn = SwitchingDynamicsParameter(A, Bm, Cm.expand(K, -1, -1).clone(), Q, prior=StickyRegimePrior(K, 0.8))
    assert float(R[0, 1]) == 0.0 and float(R[0, 0]) == float(R[1, 1])
    kf = KalmanFilter(1.0, math.sqrt(float(R[0, 0])), mu0, Sigma0, dyn)
    kf.R.copy_(R)
    return kf.to(DEV).eval()


def vs_existing_filter(DEV, K, B=3, T=9):
    """K identical regimes (K = 1: the one regime): the switching filter is the existing filter.  log_lik, a_pred, S, levels
    against KalmanFilter.predictive and mus_filt / Sigmas_filt against KalmanFilter.filter over the single regime, under the
    per-step bars."""
    args, mask = inputs(B, T, K, masked=True, seed=7, shared=True)
    one = tuple(a[:1] if i < 3 else a for i, a in enumerate(args[:5])) + (prior(1),) + args[6:]
    kf1, kfK = _kalman_filter(one, DEV), _kalman_filter(args, DEV)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    got = kfK.filter_regimes(Y, U, mk)
    pred = kf1.predictive(Y, U, mk)
    mf, Sf = pred["filter"][0].squeeze(-1), pred["filter"][1]
    c = lambda t: t.detach().cpu().double()
    for name, g, w in (("log_lik", got["log_lik"], pred["ll"]), ("log_lik_seq", got["log_lik_seq"], pred["seq_ll"]),
                       ("a_pred", got["a_pred"], pred["a_pred"]), ("S", got["S"], pred["S"]), ("mus_filt", got["mus_filt"], mf),
                       ("Sigmas_filt", got["Sigmas_filt"], Sf)):
        d = float((c(g) - c(w)).abs().max())
        print("vs the existing filter", K, name, d, TOL[name])
        assert d < TOL[name], (name, d)
    assert torch.equal(got["levels"].cpu(), pred["levels"].cpu())
    assert float((c(got["regime_filt"]) - 1.0 / K).abs().max()) < TOL["regime_filt"]


# ---- streaming, partial outputs, repeatability -----------------------------------------------------------------------------------
def _same(a, b, what):
    for k in OUTPUTS + ("levels",):
        if k == "log_lik_seq":
            continue
        assert torch.equal(a[k], b[k]), (what, k)
    for k in STATE:
        assert torch.equal(a["state"][k], b["state"][k]), (what, "state", k)


def streaming(DEV, case):
    """Chunks of (1, T - 1) and of (3, 4, rest), each continuing from the state of the one before: the outputs, concatenated, and
    the final state are the bits of the single call."""
    args, mask, _ = reference(case)
    assert mask is not None
    T = case[1]
    whole = run(DEV, args, mask)
    for sizes in ((1, T - 1), (3, 4, T - 7)):
        assert sum(sizes) == T and all(s > 0 for s in sizes)
        parts, state, t0 = [], None, 0
        for s in sizes:
            sl = slice(t0, t0 + s)
            parts.append(run(DEV, args[:8] + (args[8][:, sl], args[9][:, sl]), mask[:, sl], state=state))
            state, t0 = parts[-1]["state"], t0 + s
        joined = {k: torch.cat([p[k] for p in parts], 1) for k in OUTPUTS + ("levels",) if k != "log_lik_seq"}
        joined["state"] = parts[-1]["state"]
        _same(joined, whole, sizes)


def partial_outputs(DEV, case):
    """Each output alone gives the bits of the full call, nothing else is returned; two full calls give the same bits."""
    from kvae.kalman import lgssm_ops
    args, mask, _ = reference(case)
    full, again = run(DEV, args, mask), run(DEV, args, mask)
    _same(full, again, "second call")
    assert torch.equal(full["log_lik_seq"], again["log_lik_seq"])
    for k in lgssm_ops._SWF_OUTPUTS:
        one = run(DEV, args, mask, want=(k,))
        assert [n for n, v in one.items() if v is not None] == [k], k
        if k == "state":
            for s in STATE:
                assert torch.equal(one["state"][s], full["state"][s]), s
        else:
            assert torch.equal(one[k], full[k]), k


# ---- routing ------------------------------------------------------------------------------------------------------------------
def routing(DEV):
    """K = 9 and n = 5 are outside the kernel: the Python layer takes switching_filter_torch (float32 there), impl="hip" raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    ok = torch.zeros(1, device=DEV)
    S = lgssm_ops.switching_filter_supported
    assert S(8, 4, 4, 2, ok) and S(1, 1, 1, 2, ok)
    assert not S(9, 4, 4, 2, ok) and not S(3, 5, 2, 2, ok) and not S(3, 4, 5, 2, ok) and not S(3, 4, 2, 3, ok)
    assert not S(3, 4, 2, 2, ok.double())
    for case in ((2, 4, 9, 4, 2, False), (2, 4, 3, 5, 2, True)):
        args, mask = inputs(*case, seed=8)
        got = run(DEV, args, mask)
        ref = lgssm_ops.switching_filter_torch(*(a.double() for a in args), mask=mask)
        f32 = lgssm_ops.switching_filter_torch(*args, mask=mask)
        for k in OUTPUTS:
            assert got[k].dtype == torch.float32
            assert rel_err(got[k].cpu(), ref[k]) < 1e-4, k
            if DEV == "cpu":
                assert torch.equal(got[k], f32[k]), k                      # the restatement itself
        with pytest.raises(ValueError, match="impl='hip'"):
            run(DEV, args, mask, impl="hip")
    args, mask = inputs(2, 3, 2)
    with pytest.raises(ValueError):
        run(DEV, args, mask, want=("regimes",))
    with pytest.raises(ValueError):
        run(DEV, args, mask, impl="kernel")
    with pytest.raises(ValueError, match="state"):
        run(DEV, args, mask, state={"log_w": torch.zeros(2, 3), "mu": torch.zeros(2, 2, 4), "Sigma": torch.zeros(2, 2, 4, 4)})
    forced = run(DEV, args, mask, impl="torch")
    assert rel_err(forced["regime_filt"].cpu(), run(DEV, args, mask)["regime_filt"].cpu()) < 1e-4


# ---- the C ABI through raw pointers ------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """Error codes of include/kvae_lgssm.h, and not a byte of any output written on error."""
    from kvae import _native as N
    B, T, K, n, m = 2, 3, 3, 4, 2
    args, mask = inputs(B, T, K, n, m, masked=True)
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), mask=mask.to(DEV))
    # buffers large enough for the shapes the failing calls claim (K = 9, n = 5) too
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    outs = dict(regime_filt=big(B, T, 9), regime_pred=big(B, T, 9), ll=big(B, T), seq_ll=big(B), a_pred=big(B, T, 3), S_out=big(B, T, 3, 3),
                mus_filt=big(B, T, 5), Sigmas_filt=big(B, T, 5, 5), levels=big(B, T, dt=torch.int32), out_log_w=big(B, 9),
                out_mu=big(B, 9, 5), out_Sigma=big(B, 9, 5, 5))
    st = dict(state_log_w=torch.zeros(B, 9, device=DEV), state_mu=torch.zeros(B, 9, 5, device=DEV),
              state_Sigma=torch.eye(5, device=DEV).repeat(B, 9, 1, 1))

    def call(drop=(), **kw):
        pr = N.SwfProblem()
        pr.B, pr.T, pr.K, pr.n, pr.m, pr.p = B, T, K, n, m, 2
        for k, v in list(ins.items()) + list(outs.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in kw.items():
            setattr(pr, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        rc = lib.dll.kvae_lgssm_switching_filter(C.byref(pr), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool((v == 7).all()) for v in outs.values())
    assert lib.dll.kvae_lgssm_switching_filter(None, None) == 2
    for k in ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u"):
        assert call(drop=(k,)) == 2, k                                      # KVAE_ERR_NULL
    assert call(drop=("ll",)) == 2                                          # seq_ll reads ll
    for kw in (dict(B=0), dict(T=0), dict(B=-1)):
        assert call(**kw) == 1, kw                                          # KVAE_ERR_DIMS
    for kw in (dict(K=9), dict(K=0), dict(n=5), dict(n=0), dict(m=5), dict(p=3), dict(p=1)):
        assert call(**kw) == 4, kw                                          # KVAE_ERR_ARG
    assert call(state_log_w=st["state_log_w"]) == 4 and call(state_mu=st["state_mu"], state_Sigma=st["state_Sigma"]) == 4
    assert untouched()
    assert call(drop=("mu0", "Sigma0"), **st) == 0                          # a carried state replaces (mu0, Sigma0)
    assert call(drop=("mask",)) == 0 and call(drop=tuple(outs)) == 0 and call(drop=("seq_ll", "ll")) == 0
    assert call() == 0
    assert not any(bool((v.reshape(-1)[:2] == 7).all()) for v in outs.values())


# ---- model level -----------------------------------------------------------------------------------------------------------------
def small_model(kind="switching", K=3):
    from post_cases import small_model as make
    return make(kind, K)


def _model_case(DEV, K=3, B=3, T=12):
    model = small_model("switching", K).to(DEV)
    g = torch.Generator().manual_seed(21 + K)
    x = (torch.rand(B, T, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    mask = torch.ones(B, T)
    mask[:, 4:7] = 0
    u = (0.3 * torch.randn(B, T, model.u_dim, generator=g)).to(DEV)
    return model, x, mask, u, g


def _model_reference(model, a_vae, u, mask, dtype=torch.float64):
    from kvae.kalman import lgssm_ops
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().to(dtype)
    return lgssm_ops.switching_filter_torch(d(dyn.A), d(dyn.B), d(dyn.Q), d(dyn.C[0]), d(kf.R), dyn.prior.transition_matrix.to(dtype),
                                            d(kf.mu0), d(kf.Sigma0), d(a_vae), d(u), mask=mask)


def model_yardsticks(DEV="cpu"):
    """The float32 restatement against the float64 one on the model-level case: the numbers MODEL_YARDSTICK holds (the encoder
    needs the host simulation injected on the CPU)."""
    model, x, mask, u, _ = _model_case(DEV)
    model.eval()
    with torch.no_grad():
        a = model.encode_sequence(x, sample=False)[0]
    return distances(_model_reference(model, a, u, mask, torch.float32), _model_reference(model, a, u, mask))


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
    out = model.filter_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    again = model.filter_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    keys = OUTPUTS + ("levels", "regimes", "a_vae", "n_obs", "x_pred")
    for k in keys:
        assert torch.equal(out[k], again[k]), k
    assert model.training and dyn.tau == 0.37                               # left as they were
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_after = model(x, u=u)
    for k in ("state_probs", "mus_smooth", "Sigmas_smooth", "a_samples", "x_logits"):
        assert torch.equal(fwd_before[k], fwd_after[k]), k
    n, p = model.z_dim, model.a_dim
    shapes = dict(regime_filt=(B, T, K), regime_pred=(B, T, K), regimes=(B, T), log_lik=(B, T), log_lik_seq=(B,), a_pred=(B, T, p),
                  S=(B, T, p, p), mus_filt=(B, T, n), Sigmas_filt=(B, T, n, n), levels=(B, T), a_vae=(B, T, p), n_obs=(B,), x_pred=x.shape)
    for k, s in shapes.items():
        assert tuple(out[k].shape) == tuple(s), k
    assert out["regimes"].dtype == torch.int64 and torch.equal(out["n_obs"].cpu(), mask.sum(1))
    assert set(out["state"]) == set(STATE)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.encode_sequence(x, sample=False)[0], out["a_vae"])
    model.train()
    ref = _model_reference(model, out["a_vae"], u, mask)
    check_outputs(out, ref, mask, tol=MODEL_TOL, what="model")
    # a stream: two chunks are the bits of the whole
    first = model.filter_regimes(x[:, :5], u=u[:, :5], mask=mask[:, :5].to(DEV))
    rest = model.filter_regimes(x[:, 5:], u=u[:, 5:], mask=mask[:, 5:].to(DEV), state=first["state"])
    for k in ("regime_filt", "log_lik", "regimes", "mus_filt"):
        assert torch.equal(torch.cat([first[k], rest[k]], 1), out[k]), k
    eps = torch.randn(B * T, model.a_dim, generator=g).to(DEV)
    with noise.inject(eps_a=eps):
        drawn = model.filter_regimes(x, sample_a=True)
    assert not torch.equal(drawn["a_vae"], out["a_vae"]) and "x_pred" not in drawn


def model_errors(DEV):
    import pytest
    lstm = small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.filter_regimes(x)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.filter_regimes(torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 3, 4, device=DEV))
    model = small_model("switching").to(DEV)
    for bad in (dict(mask=torch.ones(2, 4)), dict(mask=torch.ones(3, 3)), dict(u=torch.zeros(2, 4, 4)), dict(u=torch.zeros(2, 3, 3)),
                dict(u=torch.zeros(2, 3))):
        with pytest.raises(ValueError):
            model.filter_regimes(x, **bad)


def filter_scores(DEV):
    from kvae.train.prediction import regime_filter_scores
    model, x, mask, u, _ = _model_case(DEV, B=2, T=6)
    for kw in (dict(), dict(mask=mask[:2, :6].to(DEV), u=u[:2, :6])):
        sc = regime_filter_scores(model, {"images": x[:2, :6]}, **kw)
        assert set(sc) == {"log_lik_per_step", "log_lik_per_step_map", "regime_agreement", "regime_kl"}
        assert all(isinstance(v, float) and math.isfinite(v) for v in sc.values()), sc
        assert 0.0 <= sc["regime_agreement"] <= 1.0 and sc["regime_kl"] >= -1e-6


if __name__ == "__main__":
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "kalman-vae_amd"), str(root), str(root / "tests")]
    torch.set_num_threads(4)
    print("YARDSTICK", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    from hostsim.build import build
    from kvae import _native
    _native._set_test_backend(_native.LgssmLib(build()))
    print("MODEL_YARDSTICK", {k: float(f"{v:.3g}") for k, v in model_yardsticks().items()})
    for K, T in ((2, 10), (3, 8)):
        print("GPB2 error of log_lik_seq (abs, against |log p(a)|)", (K, T), gpb2_error(K, T))
