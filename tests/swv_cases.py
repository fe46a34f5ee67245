"""Device-agnostic cases of kvae_lgssm_switching_viterbi / lgssm_ops.switching_viterbi / KalmanFilter.viterbi_regimes /
KVAE.viterbi_regimes: run against the host simulation (tests/test_switching_viterbi.py: the kernel body of csrc/lgssm_swv.h on
emulated wavefronts) and against the gfx950 library (tests/test_gpu_switching_viterbi.py).  The reference is
lgssm_ops.switching_viterbi_torch in FLOAT64 on the same float32-rounded numbers; the exactness cases are independent of it (one
float64 Kalman filter along a given regime path, every regime path enumerated)."""
import ctypes as C
import itertools
import math

import torch

import swf_cases
from golden_util import rel_err

CASES, LONG_CASE = swf_cases.CASES, swf_cases.LONG_CASE   # (B, T, K, n, m, masked): (1,1,1) ... (17,3,3) and (2,70,7)
FLOATS = ("scores", "path_log_joint", "mus_filt", "Sigmas_filt")
STATE = ("score", "mu", "Sigma")
# Yardsticks, by the project's standing rule (swf_cases.YARDSTICK): the largest ABSOLUTE distance of switching_viterbi_torch in
# FLOAT32 from its float64 run on the same inputs - scores and the beliefs per (b, t), path_log_joint and the state per sequence -
# over CASES + [LONG_CASE] with seed 0, measured on the CPU by yardsticks() (rerun: python tests/swv_cases.py).  Bars = 4 x: the
# margin covers another summation order.  (scores are running sums: the long case sets their figure.)
YARDSTICK = {"scores": 6.08e-05, "path_log_joint": 5.11e-05, "mus_filt": 3.8e-07, "Sigmas_filt": 7.8e-08, "state_score": 6.08e-05,
             "state_mu": 5.09e-07, "state_Sigma": 6.6e-08}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
# the model-level case (model_level below: the small switching KVAE's own parameters, Sigma0 = 20 I, R = 0.03^2 I), measured the
# same way by model_yardsticks() with the host simulation injected
MODEL_YARDSTICK = {"scores": 7.67e-07, "path_log_joint": 3.79e-07, "mus_filt": 4.1e-07, "Sigmas_filt": 7.94e-06, "state_score": 7.67e-07,
                   "state_mu": 9.45e-07, "state_Sigma": 2.58e-05}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}
MARGIN = 1e-4   # a float64 decision margin above which float32 must take the same decision (swf_cases.GAP)


_REF = {}


def reference(case, seed=0):
    """(args32, mask, the float64 restatement with its decision margins), computed once per case and shared; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        from kvae.kalman import lgssm_torch
        args, mask = swf_cases.inputs(*case, seed=seed)
        _REF[key] = (args, mask, lgssm_torch._swv_forward(*(a.double() for a in args), mask, None, margins=True))
    return _REF[key]


def run(DEV, args, mask=None, **kw):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_viterbi(*(a.to(DEV) for a in args), mask=None if mask is None else mask.to(DEV), **kw)


def _dist(a, b):
    """Largest absolute distance of two tensors whose -inf entries must coincide exactly."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    ninf = b == -float("inf")
    assert torch.equal(a == -float("inf"), ninf), "-inf entries differ"
    return float((a - b)[~ninf].abs().max()) if bool((~ninf).any()) else 0.0


def distances(got, ref):
    out = {k: _dist(got[k], ref[k]) for k in FLOATS}
    for k in STATE:
        out["state_" + k] = _dist(got["state"][k], ref["state"][k])
    return out


def check_outputs(got, ref, tol=None, what="", first_step=True):
    """Every output of one call against the float64 run: the floats under the bars, -inf entries in the same places, levels equal,
    path and backptr per sequence wherever every float64 decision margin of the sequence exceeds MARGIN - which must leave out no
    sequence - and backptr 0 at the first step of a stream without carried state."""
    tol = TOL if tol is None else tol
    c = lambda t: t.detach().cpu()
    dist = distances(got, ref)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in FLOATS + ("path", "backptr", "levels"):
        assert got[k].shape == ref[k].shape, k
        assert not bool(torch.isnan(c(got[k]).double()).any()), k
    for k in ("path", "backptr", "levels"):
        assert got[k].dtype == torch.int32, k
    assert torch.equal(c(got["levels"]), ref["levels"])
    decided = ref["margin"] > MARGIN
    print(what, "smallest decision margin", float(ref["margin"].min()))
    assert bool(decided.all()), ref["margin"]
    assert torch.equal(c(got["path"])[decided], ref["path"][decided])
    assert torch.equal(c(got["backptr"])[decided], ref["backptr"][decided])
    if first_step:
        assert bool((c(got["backptr"])[:, 0] == 0).all())
    return dist


def per_step(DEV, case):
    args, mask, ref = reference(case)
    return check_outputs(run(DEV, args, mask), ref, what=str(case))


def yardsticks():
    """The float32 torch restatement against the float64 one over CASES + [LONG_CASE]: the numbers YARDSTICK holds."""
    from kvae.kalman import lgssm_ops
    worst = {}
    for case in CASES + [LONG_CASE]:
        args, mask, ref = reference(case)
        f32 = lgssm_ops.switching_viterbi_torch(*args, mask=mask)
        for k, v in distances(f32, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ---- 2. exactness, independent of the restatement --------------------------------------------------------------------------------
def path_filter64(args, mask, b, paths):
    """N float64 Kalman filters along the regime paths [N,T] of sequence b: (joint [N,T] = the cumulative log p(a_{0:t}, s_{0:t} |
    u) - chain term -log K + sum log P plus the densities of the observed frames, N(y; C mu_pred, S + 1e-6 I) as
    swf_cases._kalman_step (level 0 of the ladder) -, mus [N,T,n], Sigmas [N,T,n,n] the filtered beliefs).  A hidden step predicts."""
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = args
    K, n = A.shape[0], A.shape[1]
    N, T = paths.shape
    mu, Sig = mu0.expand(N, n), Sigma0.expand(N, n, n)
    run_, joint, mus, Sigs = torch.full((N,), -math.log(K), dtype=torch.float64), [], [], []
    eye, eye2 = torch.eye(n, dtype=torch.float64), torch.eye(2, dtype=torch.float64)
    for t in range(T):
        s = paths[:, t]
        if t > 0:
            run_ = run_ + P[paths[:, t - 1], s].log()
        mp = (A[s] @ mu.unsqueeze(-1)).squeeze(-1) + Bm[s] @ U[b, t]
        Sp = A[s] @ Sig @ A[s].mT + Q[s]
        if mask is None or float(mask[b, t]) != 0.0:
            S = Cm @ Sp @ Cm.T + R
            S = 0.5 * (S + S.mT)
            r = Y[b, t] - mp @ Cm.T
            Sj = S + 1e-6 * eye2
            run_ = run_ - 0.5 * ((r.unsqueeze(-2) @ torch.linalg.inv(Sj) @ r.unsqueeze(-1)).reshape(-1) + torch.logdet(Sj) + 2 * math.log(2 * math.pi))
            Kg = Sp @ Cm.T @ torch.linalg.inv(S)
            mu = mp + (Kg @ r.unsqueeze(-1)).squeeze(-1)
            IKC = eye - Kg @ Cm
            Sig = IKC @ Sp @ IKC.mT + Kg @ R @ Kg.mT
        else:
            mu, Sig = mp, Sp
        Sig = 0.5 * (Sig + Sig.mT)
        joint.append(run_), mus.append(mu), Sigs.append(Sig)
    return torch.stack(joint, 1), torch.stack(mus, 1), torch.stack(Sigs, 1)


def score_is_exact(case, seed=0):
    """2a, the float64 restatement: path_log_joint is the joint of ONE Kalman filter along the returned path, and mus_filt /
    Sigmas_filt are that filter's beliefs, at 1e-9 relative."""
    args, mask, ref = reference(case, seed)
    a64 = tuple(a.double() for a in args)
    for b in range(case[0]):
        joint, mus, Sigs = path_filter64(a64, mask, b, ref["path"][b:b + 1].long())
        e = (rel_err(ref["path_log_joint"][b:b + 1], joint[:, -1]), rel_err(ref["mus_filt"][b:b + 1], mus), rel_err(ref["Sigmas_filt"][b:b + 1], Sigs))
        assert max(e) < 1e-9, (case, b, e)


def score_is_exact_on_kernel(DEV, case):
    """2a / 3, the kernel: path_log_joint equals KalmanFilter.path_log_joint(path) under the path_log_joint bar, and mus_filt /
    Sigmas_filt equal KalmanFilter.filter pinned to the returned path under the beliefs' bars."""
    args, mask, _ = reference(case)
    kf = swf_cases._kalman_filter(args, DEV)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), None if mask is None else mask.to(DEV)
    got = kf.viterbi_regimes(Y, U, mk)
    c = lambda t: t.detach().cpu().double()
    d = float((c(got["path_log_joint"]) - c(kf.path_log_joint(Y, U, got["path"], mk))).abs().max())
    print("path_log_joint vs path_log_joint(path)", case, d, TOL["path_log_joint"])
    assert d < TOL["path_log_joint"], d
    dyn = kf.dyn_params
    dyn.reset_state()
    with dyn.pinned(torch.nn.functional.one_hot(got["path"].long(), dyn.K).to(Y.dtype)):
        mf, Sf = kf.filter(Y, U, mk)[:2]
    for k, w in (("mus_filt", mf.squeeze(-1)), ("Sigmas_filt", Sf)):
        d = float((c(got[k]) - c(w)).abs().max())
        print("vs the filter pinned to the path", case, k, d, TOL[k])
        assert d < TOL[k], (k, d)
    with torch.no_grad():
        bad = got["path"].clone()
        bad[:, 0] = (bad[:, 0] + 1) % dyn.K
    if dyn.K > 1:   # another path scores differently: the number is a function of the path
        assert not torch.equal(kf.path_log_joint(Y, U, bad, mk), kf.path_log_joint(Y, U, got["path"], mk))


def enumerate_paths(args64, mask, b):
    """Every regime path of sequence b with its exact joint: (paths [K^T, T], joint [K^T])."""
    K, T = args64[0].shape[0], args64[8].shape[1]
    paths = torch.tensor(list(itertools.product(range(K), repeat=T)), dtype=torch.long)
    return paths, path_filter64(args64, mask, b, paths)[0][:, -1]


def true_map_when_short(DEV, K, T, B=3):
    """2b. T <= 2: every survivor of step 1 extends an exact step-0 belief, so the returned path is the true MAP of the enumeration
    of all K^T paths - the float64 restatement, and the kernel wherever the enumeration's own margin exceeds MARGIN."""
    from kvae.kalman import lgssm_ops
    args, mask = swf_cases.inputs(B, T, K, seed=11)
    a64 = tuple(a.double() for a in args)
    ref = lgssm_ops.switching_viterbi_torch(*a64)
    got = run(DEV, args)
    for b in range(B):
        paths, joint = enumerate_paths(a64, None, b)
        best = paths[int(joint.argmax())]
        assert torch.equal(ref["path"][b].long(), best), (K, T, b)
        assert rel_err(ref["path_log_joint"][b:b + 1], joint.max().reshape(1)) < 1e-9
        top = joint.topk(2).values
        assert float(top[0] - top[1]) > MARGIN
        assert torch.equal(got["path"][b].cpu().long(), best), (K, T, b)


def bounded_by_the_map(DEV, K, T, B=6):
    """2c. masked: path_log_joint <= the enumerated MAP joint <= the enumerated log p(a) (float64 restatement at 1e-9, the kernel
    under its bar).  Returns how many of the B paths are the true MAP (reported, not asserted)."""
    from kvae.kalman import lgssm_ops
    args, mask = swf_cases.inputs(B, T, K, masked=True, seed=12)
    a64 = tuple(a.double() for a in args)
    ref = lgssm_ops.switching_viterbi_torch(*a64, mask=mask)
    got = run(DEV, args, mask)
    hits = 0
    for b in range(B):
        paths, joint = enumerate_paths(a64, mask, b)
        best, total = float(joint.max()), float(torch.logsumexp(joint, 0))
        plj = float(ref["path_log_joint"][b])
        assert plj <= best + 1e-9 * abs(best) and best <= total, (b, plj, best, total)
        assert float(got["path_log_joint"][b]) <= best + TOL["path_log_joint"], (b, float(got["path_log_joint"][b]), best)
        mine = path_filter64(a64, mask, b, ref["path"][b:b + 1].long())[0][0, -1]
        assert abs(float(mine) - plj) < 1e-9 * abs(plj)
        hits += int(torch.equal(ref["path"][b].long(), paths[int(joint.argmax())]))
    print("true MAP found", (K, T), hits, "of", B)
    return hits, B


def identity_prior(DEV, K=3, T=6, B=2):
    """2d. StickyRegimePrior(K, 1.0): no regime ever changes - the path is constant, scores[:, :, j] = -log K plus the cumulative
    log-likelihood of the filter pinned at j, bp_t(j) = j, and the -inf of log P leave no NaN anywhere."""
    from kvae.kalman import lgssm_ops
    args, _ = swf_cases.inputs(B, T, K, seed=4, p_stay=1.0)
    a64 = tuple(a.double() for a in args)
    assert bool((a64[5] == torch.eye(K, dtype=torch.float64)).all())
    pinned = torch.stack([path_filter64(a64, None, b, torch.arange(K)[:, None].expand(K, T))[0].T for b in range(B)])   # [B,T,K]
    ref = lgssm_ops.switching_viterbi_torch(*a64)
    assert rel_err(ref["scores"], pinned) < 1e-9
    got = run(DEV, args)
    for out in (ref, got):
        path = out["path"].cpu()
        assert bool((path == path[:, :1]).all())
        assert bool((out["backptr"].cpu()[:, 1:] == torch.arange(K, dtype=torch.int32)).all())
        for k in FLOATS + STATE[1:]:
            v = out[k] if k in out else out["state"][k]
            assert bool(torch.isfinite(v.cpu().double()).all()), k
    d = float((got["scores"].cpu().double() - pinned).abs().max())
    print("P = I on the kernel", d, TOL["scores"])
    assert d < TOL["scores"], d
    assert torch.equal(got["path"].cpu(), ref["path"])


def shared_dynamics(DEV, K=3, T=6, B=2):
    """2e. all regimes share A, B, Q: every column holds the same numbers, staying is the best transition of the sticky prior, the
    final scores tie and the tie rule returns regime 0 throughout."""
    from kvae.kalman import lgssm_ops
    args, mask = swf_cases.inputs(B, T, K, masked=True, seed=5, shared=True)
    for out in (lgssm_ops.switching_viterbi_torch(*(a.double() for a in args), mask=mask), run(DEV, args, mask)):
        assert bool((out["path"] == 0).all())
        sc = out["scores"]
        assert bool((sc == sc[..., :1]).all())


def single_regime(DEV, B=3, T=9):
    """2f. K = 1: scores are the cumulative KalmanFilter.predictive log-likelihood, the beliefs are KalmanFilter.filter's."""
    args, mask = swf_cases.inputs(B, T, 1, masked=True, seed=7)
    kf = swf_cases._kalman_filter(args, DEV)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    got = kf.viterbi_regimes(Y, U, mk)
    pred = kf.predictive(Y, U, mk)
    c = lambda t: t.detach().cpu().double()
    assert bool((got["path"] == 0).all()) and bool((got["backptr"] == 0).all())
    assert torch.equal(got["levels"].cpu(), pred["levels"].cpu())
    for name, g, w in (("scores", got["scores"][..., 0], c(pred["ll"]).cumsum(1)), ("path_log_joint", got["path_log_joint"], pred["seq_ll"]),
                       ("mus_filt", got["mus_filt"], pred["filter"][0].squeeze(-1)), ("Sigmas_filt", got["Sigmas_filt"], pred["filter"][1])):
        d = float((c(g) - c(w)).abs().max())
        print("K = 1 vs the existing filter", name, d, TOL[name])
        assert d < TOL[name], (name, d)


# ---- 4. chunks, partial outputs ----------------------------------------------------------------------------------------------------
def backtrace(scores_last, backptr):
    """The path of a whole stream from its concatenated back-pointers [B,T,K] and the scores of its last step [B,K], in Python."""
    B, T, _ = backptr.shape
    s = (scores_last == scores_last.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)
    path = [s]
    for t in range(T - 1, 0, -1):
        s = backptr[:, t].long().gather(1, s.unsqueeze(1)).squeeze(1)
        path.append(s)
    return torch.stack(path[::-1], 1)


def streaming(DEV, case):
    """Chunks of (1, T - 1) and of (3, 4, rest), each continuing from the state of the one before: scores, backptr (concatenated)
    and the final state are the bits of the whole-sequence call, and a Python backtrace over the concatenated backptr reproduces
    the whole call's path."""
    args, mask, _ = reference(case)
    assert mask is not None
    T = case[1]
    whole = run(DEV, args, mask)
    assert torch.equal(backtrace(whole["scores"][:, -1], whole["backptr"]), whole["path"].long())
    for sizes in ((1, T - 1), (3, 4, T - 7)):
        assert sum(sizes) == T and all(s > 0 for s in sizes)
        parts, state, t0 = [], None, 0
        for s in sizes:
            sl = slice(t0, t0 + s)
            parts.append(run(DEV, args[:8] + (args[8][:, sl], args[9][:, sl]), mask[:, sl], state=state))
            state, t0 = parts[-1]["state"], t0 + s
        for k in ("scores", "backptr", "levels"):
            assert torch.equal(torch.cat([p[k] for p in parts], 1), whole[k]), (sizes, k)
        for k in STATE:
            assert torch.equal(state[k], whole["state"][k]), (sizes, "state", k)
        joined = torch.cat([p["backptr"] for p in parts], 1)
        assert torch.equal(backtrace(parts[-1]["scores"][:, -1], joined), whole["path"].long()), sizes
        assert torch.equal(parts[-1]["path"], whole["path"][:, T - sizes[-1]:])           # the last chunk ends where the stream does
        assert torch.equal(parts[-1]["path_log_joint"], whole["path_log_joint"])


def partial_outputs(DEV, case):
    """Each output alone gives the bits of the full call, nothing else is returned; two full calls give the same bits."""
    from kvae.kalman import lgssm_ops
    args, mask, _ = reference(case)
    full, again = run(DEV, args, mask), run(DEV, args, mask)
    for k in lgssm_ops._SWV_OUTPUTS:
        one = run(DEV, args, mask, want=(k,))
        assert [n for n, v in one.items() if v is not None] == [k], k
        for a in (one, again):
            if k == "state":
                assert all(torch.equal(a["state"][s], full["state"][s]) for s in STATE)
            else:
                assert torch.equal(a[k], full[k]), k


# ---- 5. routing and the C ABI ------------------------------------------------------------------------------------------------------
def routing(DEV):
    """K = 9 and n = 5 are outside the kernel: the Python layer takes switching_viterbi_torch (float32 there), impl="hip" raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    ok = torch.zeros(1, device=DEV)
    S = lgssm_ops.switching_viterbi_supported
    assert S(8, 4, 4, 2, ok) and S(1, 1, 1, 2, ok)
    assert not S(9, 4, 4, 2, ok) and not S(3, 5, 2, 2, ok) and not S(3, 4, 5, 2, ok) and not S(3, 4, 2, 3, ok) and not S(3, 4, 2, 2, ok.double())
    for case in ((2, 4, 9, 4, 2, False), (2, 4, 3, 5, 2, True)):
        args, mask = swf_cases.inputs(*case, seed=8)
        got = run(DEV, args, mask)
        ref = lgssm_ops.switching_viterbi_torch(*(a.double() for a in args), mask=mask)
        f32 = lgssm_ops.switching_viterbi_torch(*args, mask=mask)
        for k in FLOATS:
            assert got[k].dtype == torch.float32
            assert rel_err(got[k].cpu(), ref[k]) < 1e-4, k
            if DEV == "cpu":
                assert torch.equal(got[k], f32[k]), k                      # the restatement itself
        assert got["path"].dtype == torch.int32 and torch.equal(got["path"].cpu(), ref["path"])
        with pytest.raises(ValueError, match="impl='hip'"):
            run(DEV, args, mask, impl="hip")
    args, mask = swf_cases.inputs(2, 3, 2)
    with pytest.raises(ValueError):
        run(DEV, args, mask, want=("regimes",))
    with pytest.raises(ValueError):
        run(DEV, args, mask, impl="kernel")
    with pytest.raises(ValueError, match="state"):
        run(DEV, args, mask, state={"score": torch.zeros(2, 3), "mu": torch.zeros(2, 2, 4), "Sigma": torch.zeros(2, 2, 4, 4)})
    forced = run(DEV, args, mask, impl="torch")
    assert rel_err(forced["scores"].cpu(), run(DEV, args, mask)["scores"].cpu()) < 1e-4


def c_abi(lib, DEV):
    """Error codes of include/kvae_lgssm.h, and not a byte of any output written on error."""
    from kvae import _native as N
    B, T, K, n, m = 2, 3, 3, 4, 2
    args, mask = swf_cases.inputs(B, T, K, n, m, masked=True)
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), mask=mask.to(DEV))
    # buffers large enough for the shapes the failing calls claim (K = 9, n = 5) too
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    i32 = torch.int32
    outs = dict(path=big(B, T, dt=i32), path_log_joint=big(B), scores=big(B, T, 9), backptr=big(B, T, 9, dt=i32), mus_filt=big(B, T, 5),
                Sigmas_filt=big(B, T, 5, 5), levels=big(B, T, dt=i32), out_score=big(B, 9), out_mu=big(B, 9, 5), out_Sigma=big(B, 9, 5, 5))
    ws = dict(ws_bp=big(B, T, dt=i32), ws_mu=big(B, T, 9, 5), ws_Sigma=big(B, T, 9, 5, 5))
    st = dict(state_score=torch.zeros(B, 9, device=DEV), state_mu=torch.zeros(B, 9, 5, device=DEV),
              state_Sigma=torch.eye(5, device=DEV).repeat(B, 9, 1, 1))

    def call(drop=(), **kw):
        pr = N.SwvProblem()
        pr.B, pr.T, pr.K, pr.n, pr.m, pr.p = B, T, K, n, m, 2
        for k, v in list(ins.items()) + list(outs.items()) + list(ws.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in kw.items():
            setattr(pr, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        rc = lib.dll.kvae_lgssm_switching_viterbi(C.byref(pr), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    untouched = lambda: all(bool((v == 7).all()) for v in list(outs.values()) + list(ws.values()))
    assert lib.dll.kvae_lgssm_switching_viterbi(None, None) == 2
    for k in names + ("ws_bp", "ws_mu", "ws_Sigma"):
        assert call(drop=(k,)) == 2, k                                      # KVAE_ERR_NULL
    for kw in (dict(B=0), dict(T=0), dict(B=-1)):
        assert call(**kw) == 1, kw                                          # KVAE_ERR_DIMS
    for kw in (dict(K=9), dict(K=0), dict(n=5), dict(n=0), dict(m=5), dict(p=3), dict(p=1)):
        assert call(**kw) == 4, kw                                          # KVAE_ERR_ARG
    assert call(state_score=st["state_score"]) == 4 and call(state_mu=st["state_mu"], state_Sigma=st["state_Sigma"]) == 4
    assert untouched()
    assert call(drop=("mu0", "Sigma0"), **st) == 0                          # a carried state replaces (mu0, Sigma0)
    assert call(drop=("mask",)) == 0 and call(drop=tuple(outs)) == 0
    assert call(drop=("path", "mus_filt", "Sigmas_filt") + tuple(ws)) == 0   # nothing to walk back: no workspace needed
    assert call() == 0
    assert not any(bool((v.reshape(-1)[:2] == 7).all()) for v in outs.values())


# ---- 7. model level ----------------------------------------------------------------------------------------------------------------
def _model_reference(model, a_vae, u, mask, dtype=torch.float64):
    from kvae.kalman import lgssm_torch
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().to(dtype)
    return lgssm_torch._swv_forward(d(dyn.A), d(dyn.B), d(dyn.Q), d(dyn.C[0]), d(kf.R), dyn.prior.transition_matrix.to(dtype),
                                    d(kf.mu0), d(kf.Sigma0), d(a_vae), d(u), mask, None, margins=True)


def model_yardsticks(DEV="cpu"):
    """The float32 restatement against the float64 one on the model-level case: the numbers MODEL_YARDSTICK holds (the encoder
    needs the host simulation injected on the CPU)."""
    model, x, mask, u, _ = swf_cases._model_case(DEV)
    model.eval()
    with torch.no_grad():
        a = model.encode_sequence(x, sample=False)[0]
    return distances(_model_reference(model, a, u, mask, torch.float32), _model_reference(model, a, u, mask))


def model_level(DEV, K=3, B=3, T=12):
    """7. the model level: every output against float64 under 4 x MODEL_YARDSTICK, and what the call leaves untouched."""
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
    out = model.viterbi_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    again = model.viterbi_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    keys = FLOATS + ("path", "backptr", "levels", "regimes", "regimes_log_joint", "a_vae", "n_obs", "mus_smooth", "Sigmas_smooth", "a_imputed", "x_imputed")
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
    shapes = dict(path=(B, T), regimes=(B, T), path_log_joint=(B,), regimes_log_joint=(B,), scores=(B, T, K), backptr=(B, T, K), mus_filt=(B, T, n),
                  Sigmas_filt=(B, T, n, n), levels=(B, T), a_vae=(B, T, p), n_obs=(B,), mus_smooth=(B, T, n, 1), Sigmas_smooth=(B, T, n, n),
                  a_imputed=(B, T, p), x_imputed=x.shape)
    for k, s in shapes.items():
        assert tuple(out[k].shape) == tuple(s), k
    assert out["regimes"].dtype == torch.int64 and torch.equal(out["regimes"], out["path"].long())
    assert torch.equal(out["regimes_log_joint"], out["path_log_joint"]) and torch.equal(out["n_obs"].cpu(), mask.sum(1))
    assert set(out["state"]) == set(STATE)
    plain = model.viterbi_regimes(x, u=u, mask=mask.to(DEV), smooth=False)
    assert "mus_smooth" not in plain and "x_imputed" not in plain and torch.equal(plain["path"], out["path"])
    # a stream: two chunks give the bits of the whole in scores, backptr and state
    first = model.viterbi_regimes(x[:, :5], u=u[:, :5], mask=mask[:, :5].to(DEV), smooth=False)
    rest = model.viterbi_regimes(x[:, 5:], u=u[:, 5:], mask=mask[:, 5:].to(DEV), state=first["state"], smooth=False)
    for k in ("scores", "backptr"):
        assert torch.equal(torch.cat([first[k], rest[k]], 1), out[k]), k
    for k in STATE:
        assert torch.equal(rest["state"][k], out["state"][k]), k
    assert torch.equal(backtrace(rest["scores"][:, -1], torch.cat([first["backptr"], rest["backptr"]], 1)), out["regimes"])
    # every output against float64 under 4 x MODEL_YARDSTICK
    check_outputs(out, _model_reference(model, out["a_vae"], u, mask), tol=MODEL_TOL, what="model")


def model_errors(DEV):
    import pytest
    lstm = swf_cases.small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.viterbi_regimes(x)
    Y, U = torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 3, 4, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.viterbi_regimes(Y, U)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.path_log_joint(Y, U, torch.zeros(2, 3, dtype=torch.long, device=DEV))
    model = swf_cases.small_model("switching").to(DEV)
    with pytest.raises(ValueError):
        model.kalman_filter.path_log_joint(Y, U, torch.zeros(2, 4, dtype=torch.long, device=DEV))
    st = model.viterbi_regimes(x, smooth=False)["state"]
    for bad in (dict(mask=torch.ones(2, 4)), dict(u=torch.zeros(2, 4, 4)), dict(u=torch.zeros(2, 3, 3)), dict(smooth=False, decode=True),
                dict(state=st)):
        with pytest.raises(ValueError):
            model.viterbi_regimes(x, **bad)


def viterbi_scores(DEV):
    from kvae.train.prediction import viterbi_scores as scores
    model, x, mask, u, _ = swf_cases._model_case(DEV, B=2, T=6)
    names = ("viterbi", "decode", "filter", "smooth")
    for kw in (dict(), dict(mask=mask[:2, :6].to(DEV), u=u[:2, :6])):
        sc = scores(model, {"images": x[:2, :6]}, **kw)
        assert set(sc) == {"log_lik"} | {"log_joint_" + k for k in names} | {"agreement_" + k for k in names}
        assert all(isinstance(v, float) and not math.isnan(v) for v in sc.values()), sc
        assert sc["agreement_viterbi"] == 1.0 and all(0.0 <= sc["agreement_" + k] <= 1.0 for k in names)
        assert math.isfinite(sc["log_joint_viterbi"]) and math.isfinite(sc["log_lik"])
        assert sc["log_joint_viterbi"] <= sc["log_lik"] + 1e-3 * abs(sc["log_lik"])   # a joint with one path is below the marginal


if __name__ == "__main__":
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "kalman-vae_amd"), str(root), str(root / "tests")]
    torch.set_num_threads(4)
    print("YARDSTICK", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print("smallest decision margin", min(float(reference(c)[2]["margin"].min()) for c in CASES + [LONG_CASE]))
    from hostsim.build import build
    from kvae import _native
    lib = _native.LgssmLib(build())
    _native._set_test_backend(lib)
    print("MODEL_YARDSTICK", {k: float(f"{v:.3g}") for k, v in model_yardsticks().items()})
    lib.dll.kvae_hostsim_wave_emu(1)
    worst = {}
    for case in CASES + [LONG_CASE]:
        for k, v in per_step("cpu", case).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("emulated kernel", {k: float(f"{v:.3g}") for k, v in worst.items()})
    print("true MAP found", [bounded_by_the_map("cpu", K, T) for K, T in ((2, 6), (3, 5))])
