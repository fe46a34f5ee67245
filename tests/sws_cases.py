"""Device-agnostic cases of kvae_lgssm_switching_smoother / lgssm_ops.switching_smoother / KalmanFilter.smooth_regimes /
KVAE.smooth_regimes: run against the host simulation (tests/test_switching_smoother.py: the kernel bodies of csrc/lgssm_swf.h and
csrc/lgssm_sws.h on emulated wavefronts) and against the gfx950 library (tests/test_gpu_switching_smoother.py).  The reference is
lgssm_ops.switching_smoother_torch in FLOAT64 on the same float32-rounded numbers; the exactness cases are independent of it (one
float64 Kalman filter and RTS smoother per regime, or every regime path enumerated)."""
import ctypes as C
import math

import torch

from golden_util import rel_err
from swf_cases import CASES, EXCUSED, GAP, LONG_CASE, _kalman_step, inputs, small_model
import swf_cases

SMOOTH = ("regime_smooth", "regime_pairs", "mus_smooth", "Sigmas_smooth")
# Yardsticks, by the project's standing rule (swf_cases.YARDSTICK): the largest ABSOLUTE distance of switching_smoother_torch in
# FLOAT32 from its float64 run on the same inputs over CASES + [LONG_CASE] with seed 0, measured on the CPU by yardsticks()
# (rerun: python tests/sws_cases.py).  Bars = 4 x: the margin covers another summation order.
YARDSTICK = {"regime_smooth": 7.93e-7, "regime_pairs": 7.70e-7, "mus_smooth": 1.30e-6, "Sigmas_smooth": 2.55e-6}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
# the model-level case (swf_cases._model_case: the small switching KVAE's own parameters), measured the same way by
# model_yardsticks() with the host simulation injected
MODEL_YARDSTICK = {"regime_smooth": 1.91e-7, "regime_pairs": 1.86e-7, "mus_smooth": 2.73e-7, "Sigmas_smooth": 6.41e-6}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}


_REF = {}


def reference(case, seed=0):
    """(args32, mask, the float64 restatement), computed once per case and shared among the tests; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        from kvae.kalman import lgssm_ops
        args, mask = inputs(*case, seed=seed)
        _REF[key] = (args, mask, lgssm_ops.switching_smoother_torch(*(a.double() for a in args), mask=mask))
    return _REF[key]


def distances(got, ref):
    """Largest absolute distance of every smoother output from the float64 run (0 for the empty regime_pairs of T = 1)."""
    c = lambda t: t.detach().cpu().double()
    return {k: (float((c(got[k]) - ref[k]).abs().max()) if ref[k].numel() else 0.0) for k in SMOOTH}


def regimes_of(rs):
    return (rs == rs.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)


def check_outputs(got, ref, tol=None, what=""):
    """The four smoother outputs against the float64 run under the bars; regimes wherever the float64 gap says the decision is not
    a toss-up, which must be nearly everywhere; the sums of regime_pairs are regime_smooth (each within its own bar)."""
    tol = TOL if tol is None else tol
    c = lambda t: t.detach().cpu()
    dist = distances(got, ref)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in SMOOTH:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(c(got[k])).all()), k
    rs64 = ref["regime_smooth"]
    K = rs64.shape[-1]
    mine = regimes_of(c(got["regime_smooth"])) if "regimes" not in got else c(got["regimes"])
    if K > 1:
        top = rs64.topk(2, dim=-1).values
        decided = (top[..., 0] - top[..., 1]) > GAP
        excused = float((~decided).double().mean())
        print(what, "regimes: share under the gap", excused)
        assert excused <= EXCUSED, excused
        assert torch.equal(mine[decided], rs64.argmax(-1)[decided])
    if ref["regime_pairs"].shape[1]:
        rp, rs = c(got["regime_pairs"]).double(), c(got["regime_smooth"]).double()
        assert float((rp.sum(-1) - rs[:, :-1]).abs().max()) < tol["regime_pairs"] + tol["regime_smooth"]
        assert float((rp.sum(-2) - rs[:, 1:]).abs().max()) < tol["regime_pairs"] + tol["regime_smooth"]
    return dist


def run(DEV, args, mask=None, **kw):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_smoother(*(a.to(DEV) for a in args), mask=None if mask is None else mask.to(DEV), **kw)


def same_filter_bits(got, flt, what=""):
    """The filter keys of a smoother call are the bits of the filter's own call."""
    for k in swf_cases.OUTPUTS + ("levels",):
        assert torch.equal(got[k], flt[k]), (what, k)
    for k in swf_cases.STATE:
        assert torch.equal(got["state"][k], flt["state"][k]), (what, "state", k)


def per_step(DEV, case):
    args, mask, ref = reference(case)
    got = run(DEV, args, mask, impl="hip")
    same_filter_bits(got, swf_cases.run(DEV, args, mask, impl="hip"), str(case))
    return check_outputs(got, ref, what=str(case))


def yardsticks():
    """The float32 torch restatement against the float64 one over CASES + [LONG_CASE]: the numbers YARDSTICK holds."""
    from kvae.kalman import lgssm_ops
    worst = {}
    for case in CASES + [LONG_CASE]:
        args, mask, ref = reference(case)
        f32 = lgssm_ops.switching_smoother_torch(*args, mask=mask)
        for k, v in distances(f32, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def reference_leaves_no_regime_out():
    """On these inputs no (b, t) of the float64 reference falls under the decision gap."""
    for case in CASES + [LONG_CASE]:
        rs = reference(case)[2]["regime_smooth"]
        if rs.shape[-1] > 1:
            top = rs.topk(2, dim=-1).values
            assert bool(((top[..., 0] - top[..., 1]) > GAP).all()), case


# ---- exactness: references independent of the restatement ------------------------------------------------------------------------
def _rts_step(mf, Sf, u_next, ms_next, Ss_next, A, Bm, Q):
    """One plain float64 RTS step of a batch [N, ...] under ONE regime's (A, Bm, Q)."""
    mp = mf @ A.T + u_next @ Bm.T
    Sp = A @ Sf @ A.T + Q
    J = Sf @ A.T @ torch.linalg.inv(Sp)
    ms = mf + (J @ (ms_next - mp).unsqueeze(-1)).squeeze(-1)
    Ss = Sf + J @ (Ss_next - Sp) @ J.mT
    return ms, 0.5 * (Ss + Ss.mT)


def _single_smoother(Y, U, A, Bm, Q, Cm, R, mu0, Sigma0):
    """(smoothed means [B,T,n], covariances [B,T,n,n], log p(a) [B]) of one regime's filter + RTS smoother, float64."""
    B, T, _ = Y.shape
    mu, Sig = mu0.expand(B, -1), Sigma0.expand(B, -1, -1)
    mf, Sf, ll = [], [], torch.zeros(B, dtype=torch.float64)
    for t in range(T):
        mu, Sig, l = _kalman_step(mu, Sig, Y[:, t], U[:, t], A, Bm, Q, Cm, R)
        mf.append(mu), Sf.append(Sig)
        ll = ll + l
    ms, Ss = [mf[-1]], [Sf[-1]]
    for t in range(T - 2, -1, -1):
        m_, S_ = _rts_step(mf[t], Sf[t], U[:, t + 1], ms[0], Ss[0], A, Bm, Q)
        ms.insert(0, m_), Ss.insert(0, S_)
    return torch.stack(ms, 1), torch.stack(Ss, 1), ll


def _mix(w, ms, Ss):
    """Moment match over the leading K axis: w [K,B], ms [K,B,T,n], Ss [K,B,T,n,n]."""
    m_ = (w[:, :, None, None] * ms).sum(0)
    d = ms - m_
    return m_, (w[:, :, None, None, None] * (Ss + d.unsqueeze(-1) * d.unsqueeze(-2))).sum(0)


def _assert_exact(errs, what):
    print(what, errs)
    for k, v in errs.items():
        assert v < 1e-9, (what, k, v)


def exact_identity_prior(K=3, T=6, B=2):
    """P = I: a regime never changes - K independent RTS smoothers mixed by the final weights p(s | a) ~ p(a | s) / K; every
    output is exact, regime_pairs is diag(p(s | a)) at every step."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=4, p_stay=1.0)
    args = tuple(a.double() for a in args)
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    assert bool((P == torch.eye(K, dtype=torch.float64)).all())
    got = lgssm_ops.switching_smoother_torch(*args)
    per = [_single_smoother(Y, U, A[k], Bm[k], Q[k], Cm, R, mu0, Sigma0) for k in range(K)]
    w = torch.softmax(torch.stack([p[2] for p in per]), 0)                       # [K,B]
    m_, S_ = _mix(w, torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]))
    rs = w.T.unsqueeze(1).expand(B, T, K)
    _assert_exact({"regime_smooth": rel_err(got["regime_smooth"], rs), "regime_pairs": rel_err(got["regime_pairs"], torch.diag_embed(rs[:, 1:])),
                   "mus_smooth": rel_err(got["mus_smooth"], m_), "Sigmas_smooth": rel_err(got["Sigmas_smooth"], S_)}, "P = I")
    for k in SMOOTH:
        assert bool(torch.isfinite(got[k]).all()), k


def exact_shared_dynamics(K=3, T=7, B=2):
    """All regimes share A, B, Q: the frames say nothing about the regimes - one RTS smoother, regime_smooth uniform and
    regime_pairs = P / K under the symmetric prior."""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, T, K, seed=5, shared=True)
    args = tuple(a.double() for a in args)
    args = args[:5] + (args[5] / args[5].sum(-1, keepdim=True),) + args[6:]      # the float32 rows sum to 1 + 1.5e-8
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    got = lgssm_ops.switching_smoother_torch(*args)
    ms, Ss, _ = _single_smoother(Y, U, A[0], Bm[0], Q[0], Cm, R, mu0, Sigma0)
    _assert_exact({"regime_smooth": rel_err(got["regime_smooth"], torch.full((B, T, K), 1.0 / K, dtype=torch.float64)),
                   "regime_pairs": rel_err(got["regime_pairs"], (P / K).expand(B, T - 1, K, K)),
                   "mus_smooth": rel_err(got["mus_smooth"], ms), "Sigmas_smooth": rel_err(got["Sigmas_smooth"], Ss)}, "shared dynamics")


def exact_two_steps(K, B=2):
    """T = 2: the pair marginal is the filter's normalised c_ij, so regime_smooth and regime_pairs are exact for any K - against
    the K^2 paths enumerated.  (The z mean is not: mu_s^k_1 stands in for the pair-conditional mean.)"""
    from kvae.kalman import lgssm_ops
    args, _ = inputs(B, 2, K, seed=3)
    args = tuple(a.double() for a in args)
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    got = lgssm_ops.switching_smoother_torch(*args)
    lj = torch.zeros(B, K, K, dtype=torch.float64)
    for i in range(K):
        m0, S0, l0 = _kalman_step(mu0.expand(B, -1), Sigma0.expand(B, -1, -1), Y[:, 0], U[:, 0], A[i], Bm[i], Q[i], Cm, R)
        for j in range(K):
            lj[:, i, j] = -math.log(K) + l0 + P[i, j].log() + _kalman_step(m0, S0, Y[:, 1], U[:, 1], A[j], Bm[j], Q[j], Cm, R)[2]
    pairs = torch.softmax(lj.reshape(B, -1), -1).reshape(B, K, K)
    rs = torch.stack([pairs.sum(2), pairs.sum(1)], 1)
    _assert_exact({"regime_pairs": rel_err(got["regime_pairs"][:, 0], pairs), "regime_smooth": rel_err(got["regime_smooth"], rs)}, f"T = 2, K = {K}")


def pair_sums(K=3, T=8, B=3):
    """sum_k regime_pairs_t(j, k) = regime_smooth_t(j) and sum_j regime_pairs_t(j, k) = regime_smooth_{t+1}(k), float64."""
    from kvae.kalman import lgssm_ops
    args, mask = inputs(B, T, K, masked=True, seed=9)
    got = lgssm_ops.switching_smoother_torch(*(a.double() for a in args), mask=mask)
    rp, rs = got["regime_pairs"], got["regime_smooth"]
    rows, cols = float((rp.sum(-1) - rs[:, :-1]).abs().max()), float((rp.sum(-2) - rs[:, 1:]).abs().max())
    print("pair sums", rows, cols)
    assert rows < 1e-12 and cols < 1e-12
    assert float((rs.sum(-1) - 1).abs().max()) < 1e-12


def hard_prior_inputs(K=3, T=9, B=2):
    """StickyRegimePrior(K, 1.0) - zeros in P, dead columns, M_t(j) = 0 - with a mask."""
    return inputs(B, T, K, masked=True, seed=4, p_stay=1.0)


def hard_prior_is_finite():
    from kvae.kalman import lgssm_ops
    args, mask = hard_prior_inputs()
    got = lgssm_ops.switching_smoother_torch(*(a.double() for a in args), mask=mask)
    for k in SMOOTH:
        assert bool(torch.isfinite(got[k]).all()), k


def hard_prior_on_kernel(DEV):
    from kvae.kalman import lgssm_ops
    args, mask = hard_prior_inputs()
    got = run(DEV, args, mask, impl="hip")
    for k in SMOOTH:
        assert bool(torch.isfinite(got[k].cpu()).all()), k
    check_outputs(got, lgssm_ops.switching_smoother_torch(*(a.double() for a in args), mask=mask), what="hard prior on the kernel")


def gpb2_error(K, T, B=4):
    """Mean absolute error of the smoother's and of the filter's regime marginals and z mean against the exact smoothed posterior
    (every regime path enumerated, one Kalman filter + RTS smoother each), float64: the size of the GPB2 approximation (reported,
    not asserted)."""
    from kvae.kalman import lgssm_ops
    import itertools
    args, _ = inputs(B, T, K, seed=6)
    args = tuple(a.double() for a in args)
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    got = lgssm_ops.switching_smoother_torch(*args)
    n = A.shape[1]
    lps, means, onehots = [], [], []
    for path in itertools.product(range(K), repeat=T):
        mu, Sig = mu0.expand(B, -1), Sigma0.expand(B, -1, -1)
        lp = torch.full((B,), -math.log(K), dtype=torch.float64)
        mf, Sf = [], []
        for t, s in enumerate(path):
            if t > 0:
                lp = lp + P[path[t - 1], s].log()
            mu, Sig, l = _kalman_step(mu, Sig, Y[:, t], U[:, t], A[s], Bm[s], Q[s], Cm, R)
            lp = lp + l
            mf.append(mu), Sf.append(Sig)
        ms, Ss = [mf[-1]], Sf[-1]
        for t in range(T - 2, -1, -1):
            s = path[t + 1]
            m_, Ss = _rts_step(mf[t], Sf[t], U[:, t + 1], ms[0], Ss, A[s], Bm[s], Q[s])
            ms.insert(0, m_)
        lps.append(lp), means.append(torch.stack(ms, 1)), onehots.append(torch.nn.functional.one_hot(torch.tensor(path), K).double())
    w = torch.softmax(torch.stack(lps), 0)                                       # [paths,B]
    rs = torch.einsum("pb,ptk->btk", w, torch.stack(onehots))
    zm = torch.einsum("pb,pbtn->btn", w, torch.stack(means))
    mae = lambda a, b: float((a - b).abs().mean())
    return {"regime_smooth": mae(got["regime_smooth"], rs), "regime_filt": mae(got["regime_filt"], rs),
            "mus_smooth": mae(got["mus_smooth"], zm), "mus_filt": mae(got["mus_filt"], zm)}


# ---- agreement with the existing smoother ------------------------------------------------------------------------------------
def vs_existing_smoother(DEV, K, B=3, T=9):
    """K identical regimes (K = 1: the one regime): the switching smoother is KalmanFilter.smooth over the single regime, under
    the per-step bars; regime_smooth is uniform."""
    args, mask = inputs(B, T, K, masked=True, seed=7, shared=True)
    one = tuple(a[:1] if i < 3 else a for i, a in enumerate(args[:5])) + (swf_cases.prior(1),) + args[6:]
    kf1, kfK = swf_cases._kalman_filter(one, DEV), swf_cases._kalman_filter(args, DEV)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    got = kfK.smooth_regimes(Y, U, mk)
    with torch.no_grad():
        ms, Ss = kf1.smooth(Y, U, mk)[:2]
    c = lambda t: t.detach().cpu().double()
    for name, g, w in (("mus_smooth", got["mus_smooth"], ms.squeeze(-1)), ("Sigmas_smooth", got["Sigmas_smooth"], Ss)):
        d = float((c(g) - c(w)).abs().max())
        print("vs the existing smoother", K, name, d, TOL[name])
        assert d < TOL[name], (name, d)
    assert float((c(got["regime_smooth"]) - 1.0 / K).abs().max()) < TOL["regime_smooth"]


def single_step(DEV):
    """T = 1: nothing to smooth - mus_smooth = mus_filt and regime_smooth = regime_filt, bit for bit; regime_pairs is empty."""
    args, mask = inputs(3, 1, 5, seed=2)
    got = run(DEV, args, mask, impl="hip")
    assert torch.equal(got["mus_smooth"], got["mus_filt"]) and torch.equal(got["regime_smooth"], got["regime_filt"])
    assert tuple(got["regime_pairs"].shape) == (3, 0, 5, 5)
    assert float((got["Sigmas_smooth"] - got["Sigmas_filt"]).abs().max()) < TOL["Sigmas_smooth"]


# ---- partial outputs, repeatability, routing ---------------------------------------------------------------------------------
def partial_outputs(DEV, case):
    """Each smoother output alone (and next to one filter output) gives the bits of the full call, nothing else is returned; two
    full calls give the same bits."""
    args, mask, _ = reference(case)
    full, again = run(DEV, args, mask, impl="hip"), run(DEV, args, mask, impl="hip")
    for k in SMOOTH:
        assert torch.equal(full[k], again[k]), k
    same_filter_bits(full, again, "second call")
    for k in SMOOTH:
        one = run(DEV, args, mask, want=(k,), impl="hip")
        assert [n for n, v in one.items() if v is not None] == [k], k
        assert torch.equal(one[k], full[k]), k
    two = run(DEV, args, mask, want=("log_lik_seq", "mus_smooth", "regime_smooth"), impl="hip")
    assert sorted(n for n, v in two.items() if v is not None) == ["log_lik_seq", "mus_smooth", "regime_smooth"]
    for k in ("log_lik_seq", "mus_smooth", "regime_smooth"):
        assert torch.equal(two[k], full[k]), k
    only_filter = run(DEV, args, mask, want=("regime_filt",), impl="hip")
    assert torch.equal(only_filter["regime_filt"], full["regime_filt"])


def carried_state(DEV, case=(3, 12, 7, 4, 2, True)):
    """A carried-in state goes to the forward: the filter keys of the second chunk are the bits of the filter's own chunked call,
    and the smoother outputs are the float64 restatement's from the same state (smoothing conditional on the window alone)."""
    from kvae.kalman import lgssm_ops
    args, mask, _ = reference(case)
    first = swf_cases.run(DEV, args[:8] + (args[8][:, :5], args[9][:, :5]), mask[:, :5], impl="hip")
    rest = args[:8] + (args[8][:, 5:], args[9][:, 5:])
    got = run(DEV, rest, mask[:, 5:], state=first["state"], impl="hip")
    same_filter_bits(got, swf_cases.run(DEV, rest, mask[:, 5:], state=first["state"], impl="hip"), "carried state")
    st64 = {k: v.detach().cpu().double() for k, v in first["state"].items()}
    check_outputs(got, lgssm_ops.switching_smoother_torch(*(a.double() for a in rest), mask=mask[:, 5:], state=st64), what="carried state")


def routing(DEV):
    """K = 9 and n = 5 are outside the kernel: the Python layer takes switching_smoother_torch (float32 there), impl="hip" raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    ok = torch.zeros(1, device=DEV)
    S = lgssm_ops.switching_smoother_supported
    assert S(8, 4, 4, 2, ok) and S(1, 1, 1, 2, ok)
    assert not S(9, 4, 4, 2, ok) and not S(3, 5, 2, 2, ok) and not S(3, 4, 5, 2, ok) and not S(3, 4, 2, 3, ok)
    assert not S(3, 4, 2, 2, ok.double())
    for case in ((2, 4, 9, 4, 2, False), (2, 4, 3, 5, 2, True)):
        args, mask = inputs(*case, seed=8)
        got = run(DEV, args, mask)
        ref = lgssm_ops.switching_smoother_torch(*(a.double() for a in args), mask=mask)
        f32 = lgssm_ops.switching_smoother_torch(*args, mask=mask)
        for k in SMOOTH:
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
    forced = run(DEV, args, mask, impl="torch")
    assert rel_err(forced["regime_smooth"].cpu(), run(DEV, args, mask)["regime_smooth"].cpu()) < 1e-4


# ---- the C ABI through raw pointers ------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """Error codes of include/kvae_lgssm.h, and not a byte of any output or of the history written on error."""
    from kvae import _native as N
    B, T, K, n, m = 2, 3, 3, 4, 2
    args, mask = inputs(B, T, K, n, m, masked=True)
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), mask=mask.to(DEV))
    # buffers large enough for the shapes the failing calls claim (K = 9, n = 5) too
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    fouts = dict(regime_filt=big(B, T, 9), regime_pred=big(B, T, 9), ll=big(B, T), seq_ll=big(B), a_pred=big(B, T, 3), S_out=big(B, T, 3, 3),
                 mus_filt=big(B, T, 5), Sigmas_filt=big(B, T, 5, 5), levels=big(B, T, dt=torch.int32), out_log_w=big(B, 9),
                 out_mu=big(B, 9, 5), out_Sigma=big(B, 9, 5, 5))
    hist = dict(hist_mu=big(B, T, 9, 5), hist_Sigma=big(B, T, 9, 5, 5), hist_W=big(B, T, 9, 9), hist_w=big(B, 9))
    souts = dict(regime_smooth=big(B, T, 9), regime_pairs=big(B, T, 9, 9), mus_smooth=big(B, T, 5), Sigmas_smooth=big(B, T, 5, 5))
    st = dict(state_log_w=torch.zeros(B, 9, device=DEV), state_mu=torch.zeros(B, 9, 5, device=DEV),
              state_Sigma=torch.eye(5, device=DEV).repeat(B, 9, 1, 1))

    def call(drop=(), **kw):
        pr = N.SwsProblem()
        f = pr.filt
        f.B, f.T, f.K, f.n, f.m, f.p = B, T, K, n, m, 2
        for k, v in list(ins.items()) + list(fouts.items()):
            if k not in drop:
                setattr(f, k, v.data_ptr())
        for k, v in list(hist.items()) + list(souts.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in kw.items():
            setattr(f, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        rc = lib.dll.kvae_lgssm_switching_smoother(C.byref(pr), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    everything = list(fouts.values()) + list(hist.values()) + list(souts.values())
    untouched = lambda: all(bool((v == 7).all()) for v in everything)
    assert lib.dll.kvae_lgssm_switching_smoother(None, None) == 2
    for k in names + tuple(hist):
        assert call(drop=(k,)) == 2, k                                      # KVAE_ERR_NULL
    assert call(drop=("ll",)) == 2                                          # seq_ll reads ll
    for kw in (dict(B=0), dict(T=0), dict(B=-1)):
        assert call(**kw) == 1, kw                                          # KVAE_ERR_DIMS
    for kw in (dict(K=9), dict(K=0), dict(n=5), dict(n=0), dict(m=5), dict(p=3), dict(p=1)):
        assert call(**kw) == 4, kw                                          # KVAE_ERR_ARG
    assert call(state_log_w=st["state_log_w"]) == 4 and call(state_mu=st["state_mu"], state_Sigma=st["state_Sigma"]) == 4
    assert untouched()
    assert call(drop=("mu0", "Sigma0"), **st) == 0                          # a carried state replaces (mu0, Sigma0)
    assert call(drop=("mask",)) == 0 and call(drop=tuple(fouts) + tuple(souts)) == 0 and call(drop=tuple(souts)) == 0
    assert call(drop=tuple(fouts)) == 0 and call(T=1) == 0
    assert call() == 0
    assert not any(bool((v.reshape(-1)[:2] == 7).all()) for v in everything)


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _model_reference(model, a_vae, u, mask, dtype=torch.float64):
    from kvae.kalman import lgssm_ops
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().to(dtype)
    return lgssm_ops.switching_smoother_torch(d(dyn.A), d(dyn.B), d(dyn.Q), d(dyn.C[0]), d(kf.R), dyn.prior.transition_matrix.to(dtype),
                                              d(kf.mu0), d(kf.Sigma0), d(a_vae), d(u), mask=mask)


def model_yardsticks(DEV="cpu"):
    """The float32 restatement against the float64 one on the model-level case: the numbers MODEL_YARDSTICK holds (the encoder
    needs the host simulation injected on the CPU)."""
    model, x, mask, u, _ = swf_cases._model_case(DEV)
    model.eval()
    with torch.no_grad():
        a = model.encode_sequence(x, sample=False)[0]
    return distances(_model_reference(model, a, u, mask, torch.float32), _model_reference(model, a, u, mask))


def model_level(DEV, K=3, B=3, T=12):
    from kvae import noise
    model, x, mask, u, g = swf_cases._model_case(DEV, K, B, T)
    model.train()
    dyn = model.kalman_filter.dyn_params
    dyn.tau = 0.37
    before = {k: v.clone() for k, v in model.state_dict().items()}
    nz = dict(eps_a=torch.randn(B * T, model.a_dim, generator=g).to(DEV), eps_z=torch.randn(B, T, model.z_dim, generator=g).to(DEV),
              gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV))
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_before = model(x, u=u)
    out = model.smooth_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    again = model.smooth_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    for k in SMOOTH + ("regimes", "a_smooth", "a_vae", "n_obs", "x_smooth"):
        assert torch.equal(out[k], again[k]), k
    assert model.training and dyn.tau == 0.37                               # left as they were
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_after = model(x, u=u)
    for k in ("state_probs", "mus_smooth", "Sigmas_smooth", "a_samples", "x_logits"):
        assert torch.equal(fwd_before[k], fwd_after[k]), k
    n, p = model.z_dim, model.a_dim
    shapes = dict(regime_smooth=(B, T, K), regime_pairs=(B, T - 1, K, K), regimes=(B, T), mus_smooth=(B, T, n), Sigmas_smooth=(B, T, n, n),
                  a_smooth=(B, T, p), a_vae=(B, T, p), n_obs=(B,), x_smooth=x.shape, regime_filt=(B, T, K), log_lik=(B, T))
    for k, s in shapes.items():
        assert tuple(out[k].shape) == tuple(s), k
    assert out["regimes"].dtype == torch.int64 and torch.equal(out["n_obs"].cpu(), mask.sum(1))
    assert torch.equal(out["regimes"], regimes_of(out["regime_smooth"]))
    flt = model.filter_regimes(x, u=u, mask=mask.to(DEV))
    same_filter_bits(out, flt, "model")
    assert torch.equal(out["a_vae"], flt["a_vae"])
    Cm = dyn.C[0].detach()
    assert float((out["a_smooth"] - out["mus_smooth"] @ Cm.mT).abs().max()) == 0.0
    ref = _model_reference(model, out["a_vae"], u, mask)
    check_outputs(out, ref, tol=MODEL_TOL, what="model")
    assert "x_smooth" not in model.smooth_regimes(x)
    return model, x, mask, u


def model_errors(DEV):
    import pytest
    lstm = small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.smooth_regimes(x)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.smooth_regimes(torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 3, 4, device=DEV))
    model = small_model("switching").to(DEV)
    for bad in (dict(mask=torch.ones(2, 4)), dict(u=torch.zeros(2, 4, 4))):
        with pytest.raises(ValueError):
            model.smooth_regimes(x, **bad)


def smoother_scores(DEV):
    from kvae.train.imputation import regime_smoother_scores
    model, x, mask, u, _ = swf_cases._model_case(DEV, B=2, T=8)
    model.train()
    sc = regime_smoother_scores(model, x, mask[:, :8], u=u)
    assert model.training
    assert set(sc) == {"mse_smooth", "mse_impute", "mse_pred", "regime_agreement"}
    assert all(isinstance(v, float) and math.isfinite(v) for v in sc.values()), sc
    assert 0.0 <= sc["regime_agreement"] <= 1.0 and min(sc["mse_smooth"], sc["mse_impute"], sc["mse_pred"]) >= 0.0


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
    for K, T in ((2, 8), (3, 6), (2, 12), (3, 7)):
        print("GPB2 mean absolute error against the exact smoothed posterior", (K, T), {k: float(f"{v:.3g}") for k, v in gpb2_error(K, T).items()})
