"""Device-agnostic cases of kvae_lgssm_switching_marginal / kvae_lgssm_switching_marginal_bwd / lgssm_ops.switching_log_marginal /
KalmanFilter.regime_log_marginal / the "regime_marginal" objective: run against the host simulation
(tests/test_switching_marginal.py: the kernel bodies of csrc/lgssm_swf.h and csrc/lgssm_swm.h on emulated wavefronts) and against
the gfx950 library (tests/test_gpu_switching_marginal.py).  The reference is FLOAT64 autograd of
lgssm_ops.switching_log_marginal_torch on the same float32-rounded numbers, one sequence at a time (which gives the per-sequence
partials the ABI writes to its workspace); the exactness cases are independent of that autograd (every regime path enumerated,
one filter per regime, a single filter)."""
import ctypes as C
import math

import torch

import swf_cases as F

CASES = F.CASES + [F.LONG_CASE]
NAMES = ("A", "Bm", "Q", "Cm", "R", "P", "mu0", "Sigma0", "Y", "U")
PARAMS = ("gA", "gB", "gQ", "gC", "gP", "g_mu0", "g_Sigma0")                 # the B-summed outputs, per tensor
BLOCKS = ("ws_A", "ws_B", "ws_Q", "ws_C", "ws_logP", "ws_mu0", "ws_Sigma0")  # the blocks of the workspace, per sequence
OUTPUTS = ("gA", "gB", "gQ", "gC", "g_logP", "g_mu0", "g_Sigma0", "gY", "gU", "ll_recomputed")   # the output fields of kvae_swm_grads
_FIELD_OF = dict(ws_A="gA", ws_B="gB", ws_Q="gQ", ws_C="gC", ws_logP="g_logP", ws_mu0="g_mu0", ws_Sigma0="g_Sigma0")
_ARG_OF = dict(gA=0, gB=1, gQ=2, gC=3, gP=5, g_mu0=6, g_Sigma0=7, gY=8, gU=9)
# Yardsticks, by the project's standing rule: the float32 autograd run of switching_log_marginal_torch against its float64 run
# over CASES with seed 0 and the upstreams of upstream(), as |f32 - f64| / max(1, |f64|) in max-norm within the slice - per (b, t)
# for gY and gU, per sequence for each block of the workspace, per tensor for the B-summed gradients (summed over b in float32,
# ascending) - the largest over all slices, measured on the CPU by yardsticks() (rerun: python tests/swm_cases.py).
# Bars = 4 x: the margin covers another summation order.  Every pair of the reference sits at ladder level 0 (asserted), so no
# item is left out.
YARDSTICK = {"gY": 3.41e-06, "gU": 3.46e-06, "ws_A": 1.27e-06, "ws_B": 1.14e-06, "ws_Q": 2.72e-06, "ws_C": 1.43e-06, "ws_logP": 1.88e-06,
             "ws_mu0": 6.5e-07, "ws_Sigma0": 8.5e-07, "gA": 1.21e-06, "gB": 9.37e-07, "gQ": 2.82e-06, "gC": 9.86e-07, "gP": 1.14e-06,
             "g_mu0": 6.66e-07, "g_Sigma0": 5.82e-07}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
# the model-level case (model_level below), measured the same way by model_yardsticks(): gradients of seq_ll.sum() w.r.t. a, u and
# the dynamics' A, B, Q, C per tensor
MODEL_YARDSTICK = {"A": 2.82e-07, "B": 5.12e-08, "Q": 1.89e-07, "C": 5.02e-07, "a": 2.31e-07, "u": 5.01e-09}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}


def layout(K, n, m):
    """Float offsets of the blocks of one sequence's partial (include/kvae_lgssm.h, kvae_swm_grads.ws) and the row length G."""
    off, out = 0, {}
    for name, size in (("ws_A", K * n * n), ("ws_B", K * n * m), ("ws_Q", K * n * n), ("ws_C", 2 * n), ("ws_logP", K * K), ("ws_mu0", n),
                       ("ws_Sigma0", n * n)):
        out[name] = (off, off + size)
        off += size
    return out, off


def upstream(B, T, seed=0):
    g = torch.Generator().manual_seed(7000 + 100 * seed + 10 * B + T)
    return torch.randn(B, T, generator=g, dtype=torch.float64), torch.randn(B, generator=g, dtype=torch.float64)


def restated(args, mask, g_ll, g_seq, dtype):
    """Autograd of the restatement in `dtype`, one sequence at a time: dict(ll, seq_ll, levels, gY, gU, the blocks of the workspace
    [B, ...] per sequence, the B-summed gradients (ascending b, in `dtype`))."""
    from kvae.kalman import lgssm_ops
    B = args[8].shape[0]
    per, outs = [], []
    for b in range(B):
        a = [t.to(dtype).clone() for t in args]
        a[8], a[9] = a[8][b:b + 1].clone(), a[9][b:b + 1].clone()
        for i, t in enumerate(a):
            t.requires_grad_(i != 4)
        out = lgssm_ops.switching_log_marginal_torch(*a, mask=None if mask is None else mask[b:b + 1])
        loss = 0.0
        if g_ll is not None:
            loss = loss + (out["ll"] * g_ll[b:b + 1].to(dtype)).sum()
        if g_seq is not None:
            loss = loss + (out["seq_ll"] * g_seq[b:b + 1].to(dtype)).sum()
        loss.backward()
        per.append([torch.zeros_like(t) if t.grad is None else t.grad for t in a])   # P at T = 1: never read
        outs.append({k: v.detach() for k, v in out.items()})
    res = {k: torch.cat([o[k] for o in outs]) for k in ("ll", "seq_ll", "levels")}
    res["gY"], res["gU"] = torch.cat([p[8] for p in per]), torch.cat([p[9] for p in per])
    P = args[5].to(dtype)
    for blk, i in (("ws_A", 0), ("ws_B", 1), ("ws_Q", 2), ("ws_C", 3), ("ws_mu0", 6), ("ws_Sigma0", 7)):
        res[blk] = torch.stack([p[i] for p in per])
    res["ws_logP"] = torch.stack([p[5] * P for p in per])
    for name in PARAMS:
        acc = torch.zeros_like(per[0][_ARG_OF[name]])
        for p in per:
            acc = acc + p[_ARG_OF[name]]
        res[name] = acc
    return res


_REF = {}


def reference(case, seed=0):
    """(args32, mask, g_ll, g_seq, the float64 run), computed once per case and shared among the tests; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        args, mask = F.inputs(*case, seed=seed)
        g_ll, g_seq = upstream(case[0], case[1], seed)
        g_ll, g_seq = g_ll.float().double(), g_seq.float().double()
        ref = restated(args, mask, g_ll, g_seq, torch.float64)
        assert int(ref["levels"].max()) == 0, case                           # no item is left out
        _REF[key] = (args, mask, g_ll, g_seq, ref)
    return _REF[key]


def _slices(k, got, ref):
    """|got - ref| / max(1, |ref|), max-norm within the slice; the largest over the slices of entry k."""
    g, r = got.detach().cpu().double(), ref.detach().double()
    if k in ("gY", "gU"):
        g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    elif k in BLOCKS:
        g, r = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
    else:
        g, r = g.reshape(1, -1), r.reshape(1, -1)
    return float(((g - r).abs().amax(1) / r.abs().amax(1).clamp_min(1.0)).max())


def distances(got, ref, keys=None):
    return {k: _slices(k, got[k], ref[k]) for k in (keys or YARDSTICK) if got.get(k) is not None}


def yardsticks():
    worst = {}
    for case in CASES:
        args, mask, g_ll, g_seq, ref = reference(case)
        f32 = restated(args, mask, g_ll, g_seq, torch.float32)
        for k, v in distances(f32, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------
def raw(DEV, args, mask, g_ll, g_seq, want=OUTPUTS, filt=("ll", "seq_ll", "levels")):
    """kvae_lgssm_switching_marginal, then kvae_lgssm_switching_marginal_bwd for the outputs named in `want`, through ctypes: dict
    of the forward's outputs, the workspace split into its blocks, the requested gradients (gP derived from g_logP)."""
    from kvae import _native as N
    from kvae.kalman import lgssm_ops as O
    a = [t.float().to(DEV).contiguous() for t in args]
    mk = None if mask is None else mask.float().to(DEV).contiguous()
    K, n, m = a[0].shape[0], a[0].shape[1], a[1].shape[2]
    B, T, _ = a[8].shape
    new = lambda *s, dt=torch.float32: torch.full(s, float("nan") if dt == torch.float32 else -1, device=DEV, dtype=dt)
    hist = (new(B, T, K), new(B, T, K, n), new(B, T, K, n, n))
    sp, keep = O._swm_problem(*a, mk, hist)
    out = {"ll": new(B, T), "seq_ll": new(B), "levels": new(B, T, dt=torch.int32), "a_pred": new(B, T, 2), "mus_filt": new(B, T, n),
           "regime_filt": new(B, T, K)}
    out = {k: v for k, v in out.items() if k in filt or (k == "ll" and "seq_ll" in filt)}
    for k, v in out.items():
        setattr(sp.filt, k, v.data_ptr())
    lib = N.lib_for(a[8])
    lib.check(lib.dll.kvae_lgssm_switching_marginal(C.byref(sp), N.stream_for(a[8])), "kvae_lgssm_switching_marginal")
    blocks, G = layout(K, n, m)
    assert lib.dll.kvae_lgssm_switching_marginal_ws_floats(B, K, n, m) == B * G
    ws = new(B, G)
    shapes = dict(gA=(K, n, n), gB=(K, n, m), gQ=(K, n, n), gC=(2, n), g_logP=(K, K), g_mu0=(n,), g_Sigma0=(n, n), gY=(B, T, 2), gU=(B, T, m),
                  ll_recomputed=(B, T))
    grads = {k: new(*shapes[k]) for k in want}
    g = N.SwmGrads()
    gl = None if g_ll is None else g_ll.float().to(DEV).contiguous()
    gs = None if g_seq is None else g_seq.float().to(DEV).contiguous()
    g.g_ll, g.g_seq, g.ws = N.ptr(gl), N.ptr(gs), ws.data_ptr()
    for k, v in grads.items():
        setattr(g, k, v.data_ptr())
    lib.check(lib.dll.kvae_lgssm_switching_marginal_bwd(C.byref(sp), C.byref(g), N.stream_for(a[8])), "kvae_lgssm_switching_marginal_bwd")
    if DEV != "cpu":
        torch.cuda.synchronize()
    del keep
    out.update(grads)
    out["ws"] = ws
    if want:
        for k, (lo, hi) in blocks.items():
            out[k] = ws[:, lo:hi].reshape(B, *shapes[_FIELD_OF[k]])
    if "g_logP" in grads:
        P = a[5]
        out["gP"] = torch.where(P > 0, grads["g_logP"] / torch.where(P > 0, P, torch.ones_like(P)), torch.zeros_like(P))
    return out


def check(got, ref, mask, tol=None, what="", keys=None):
    tol = TOL if tol is None else tol
    dist = distances(got, ref, keys)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in dist:
        assert bool(torch.isfinite(got[k]).all()), k
    if mask is not None and got.get("gY") is not None:
        hidden = mask == 0
        assert bool(hidden.any()) and bool((got["gY"].cpu()[hidden] == 0).all())       # exact zeros, selected
    return dist


def gradients(DEV, case):
    """Every gradient of the raw ABI against float64 autograd per slice, the forward's values against the filter's bit for bit."""
    args, mask, g_ll, g_seq, ref = reference(case)
    got = raw(DEV, args, mask, g_ll, g_seq, filt=("ll", "seq_ll", "levels", "a_pred", "mus_filt", "regime_filt"))
    assert not bool(torch.isnan(got["ws"]).any())                                        # every element written
    filt = F.run(DEV, args, mask, impl="hip")
    for k, fk in (("ll", "log_lik"), ("seq_ll", "log_lik_seq"), ("levels", "levels"), ("a_pred", "a_pred"), ("mus_filt", "mus_filt"),
                  ("regime_filt", "regime_filt")):
        assert torch.equal(got[k], filt[fk]), k
    assert torch.equal(got["levels"].cpu(), ref["levels"])
    # the adjoint recomputes the pair step by the forward's own functions (csrc/lgssm_sw_pair.h): their ll must be the forward's bits
    assert torch.equal(got["ll_recomputed"], got["ll"])
    return check(got, ref, mask, what=str(case))


def upstreams(DEV, case=(3, 5, 3, 4, 2, True)):
    """Only g_ll, only g_seq, both - through the autograd Function: each against its own float64 run, and the two single runs sum to
    the run with both (the adjoint is linear in the upstreams), within the bars."""
    from kvae.kalman import lgssm_ops
    args, mask, g_ll, g_seq, ref = reference(case)
    runs = {}
    for name, (gl, gs) in (("ll", (g_ll, None)), ("seq", (None, g_seq)), ("both", (g_ll, g_seq))):
        a = [t.to(DEV).clone().requires_grad_(i != 4) for i, t in enumerate(args)]
        out = lgssm_ops.switching_log_marginal(*a, mask=mask.to(DEV), impl="hip")
        loss = 0.0
        if gl is not None:
            loss = loss + (out["ll"] * gl.float().to(DEV)).sum()
        if gs is not None:
            loss = loss + (out["seq_ll"] * gs.float().to(DEV)).sum()
        loss.backward()
        runs[name] = {k: a[i].grad for k, i in _ARG_OF.items()}
        keys = PARAMS + ("gY", "gU")
        own = ref if name == "both" else restated(args, mask, gl, gs, torch.float64)
        check(runs[name], own, mask, what="upstream " + name, keys=keys)
    for k in _ARG_OF:
        s = runs["ll"][k].double() + runs["seq"][k].double()
        d = _slices(k, s, runs["both"][k].cpu().double())
        print("upstreams: ll + seq against both", k, d, TOL[k])
        assert d < TOL[k], (k, d)


def bits(DEV, case=(3, 5, 3, 4, 2, True)):
    """Every output alone gives the bits of the full call; two full calls are bit-identical."""
    args, mask, g_ll, g_seq, _ = reference(case)
    full, again = raw(DEV, args, mask, g_ll, g_seq), raw(DEV, args, mask, g_ll, g_seq)
    for k in OUTPUTS + ("ws", "ll", "seq_ll", "levels"):
        assert torch.equal(full[k], again[k]), k
    for k in OUTPUTS:
        one = raw(DEV, args, mask, g_ll, g_seq, want=(k,))
        assert torch.equal(one[k], full[k]), k
        assert torch.equal(one["ws"], full["ws"]), k


# ---- independent of the restatement's autograd: float64, on the CPU --------------------------------------------------------------
def _grads64(fn, args, mask=None):
    a = [t.double().clone().requires_grad_(i != 4) for i, t in enumerate(args)]
    fn(*a, mask=mask).backward()
    return [t.grad for t in a]


def _restated_total(*a, mask=None):
    from kvae.kalman import lgssm_ops
    return lgssm_ops.switching_log_marginal_torch(*a, mask=mask)["seq_ll"].sum()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1.0))


def _single_filter_total(A, Bm, Q, Cm, R, mu0, Sigma0, Y, U):
    """sum_b log p(a_b | u_b) of ONE regime's filter, the density at ladder level 0 (swf_cases._kalman_step)."""
    B, T, _ = Y.shape
    Q, Sigma0 = 0.5 * (Q + Q.mT), 0.5 * (Sigma0 + Sigma0.mT)
    mu, Sig, total = mu0.expand(B, -1), Sigma0.expand(B, -1, -1), 0.0
    for t in range(T):
        mu, Sig, ll = F._kalman_step(mu, Sig, Y[:, t], U[:, t], A, Bm, Q, Cm, R)
        total = total + ll.sum()
    return total


def exact_two_steps(K):
    """T = 2: GPB2 is exact, so the gradient is that of log sum over the K^2 enumerated regime paths (one Kalman filter each)."""
    args, _ = F.inputs(2, 2, K, seed=3)

    def enumerated(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None):
        Qs, S0 = 0.5 * (Q + Q.mT), 0.5 * (Sigma0 + Sigma0.mT)
        B = Y.shape[0]
        paths = []
        for s0 in range(K):
            m1, S1, l1 = F._kalman_step(mu0.expand(B, -1), S0.expand(B, -1, -1), Y[:, 0], U[:, 0], A[s0], Bm[s0], Qs[s0], Cm, R)
            for s1 in range(K):
                _, _, l2 = F._kalman_step(m1, S1, Y[:, 1], U[:, 1], A[s1], Bm[s1], Qs[s1], Cm, R)
                paths.append(-math.log(K) + l1 + P[s0, s1].log() + l2)
        return torch.logsumexp(torch.stack(paths), 0).sum()

    ga, gb = _grads64(_restated_total, args), _grads64(enumerated, args)
    for i, name in enumerate(NAMES):
        if ga[i] is not None:
            assert _rel(ga[i], gb[i]) < 1e-9, (K, name, _rel(ga[i], gb[i]))


def exact_identity_prior(K=3, T=6, B=2):
    """P = I: log p(a) = log (1/K) sum_k p_k(a), so the gradient is sum_k softmax_k(log p_k) grad log p_k over K single filters."""
    args, _ = F.inputs(B, T, K, seed=4, p_stay=1.0)

    def mixture(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None):
        per = []
        for k in range(K):
            per.append(torch.stack([_single_filter_total(A[k], Bm[k], Q[k], Cm, R, mu0, Sigma0, Y[b:b + 1], U[b:b + 1]) for b in range(B)]))
        return (torch.logsumexp(torch.stack(per), 0) - math.log(K)).sum()

    ga, gb = _grads64(_restated_total, args), _grads64(mixture, args)
    for i, name in enumerate(NAMES):
        if name in ("R", "P"):
            continue
        assert bool(torch.isfinite(ga[i]).all()), name
        assert _rel(ga[i], gb[i]) < 1e-9, (name, _rel(ga[i], gb[i]))
    assert bool(torch.isfinite(ga[5]).all())


def exact_shared_dynamics(K=3, T=6, B=2):
    """Shared A, B, Q: the mixture is one Gaussian; gY, gU, gC, g_mu0, g_Sigma0 are a single filter's, and the per-regime gradients
    of A, B, Q sum to it."""
    args, _ = F.inputs(B, T, K, seed=5, shared=True)
    args = [a.double() for a in args]
    args[5] = args[5] / args[5].sum(-1, keepdim=True)   # the float32 prior's rows sum to 1 + 1.5e-8 (swf_cases.exact_shared_dynamics)
    ga = _grads64(_restated_total, args)
    one = lambda A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None: _single_filter_total(A[0], Bm[0], Q[0], Cm, R, mu0, Sigma0, Y, U)
    gb = _grads64(one, args)
    for i in (3, 6, 7, 8, 9):
        assert _rel(ga[i], gb[i]) < 1e-9, (NAMES[i], _rel(ga[i], gb[i]))
    for i in (0, 1, 2):
        assert _rel(ga[i].sum(0), gb[i][0]) < 1e-9, (NAMES[i], _rel(ga[i].sum(0), gb[i][0]))


def value_is_the_filters():
    """The float64 log_lik of the restatement is switching_filter_torch's within 1e-12, levels equal."""
    from kvae.kalman import lgssm_ops
    for case in CASES:
        args, mask, _, _, ref = reference(case)
        filt = lgssm_ops.switching_filter_torch(*(a.double() for a in args), mask=mask)
        assert float((ref["ll"] - filt["log_lik"]).abs().max()) < 1e-12 and torch.equal(ref["levels"], filt["levels"])


# ---- zeros of P --------------------------------------------------------------------------------------------------------------
def hard_prior(DEV):
    """StickyRegimePrior(3, 1.0) = I with a mask at T = 9: finite gradients from the restatement and the kernel, g_logP exactly 0
    off the diagonal, the kernel under the bars."""
    args, mask = F.inputs(2, 9, 3, masked=True, seed=4, p_stay=1.0)
    assert bool((args[5] == torch.eye(3)).all()) and mask is not None
    g_ll, g_seq = upstream(2, 9, 4)
    g_ll, g_seq = g_ll.float().double(), g_seq.float().double()
    ref = restated(args, mask, g_ll, g_seq, torch.float64)
    for k in YARDSTICK:
        assert bool(torch.isfinite(ref[k]).all()), k
    assert int(ref["levels"].max()) == 0
    got = raw(DEV, args, mask, g_ll, g_seq)
    off = ~torch.eye(3, dtype=torch.bool)
    assert bool((got["g_logP"].cpu()[off] == 0).all()) and bool((got["ws_logP"].cpu()[:, off] == 0).all())
    assert bool((got["gP"].cpu()[off] == 0).all())
    check(got, ref, mask, what="P = I")


# ---- ladder ------------------------------------------------------------------------------------------------------------------
def ladder_inputs(r11=-2e-6):
    """A slightly indefinite R whose negative direction the state does not reach: the second row of C is 0, so S = C Sp C^T + R has
    S_11 = R_11 < 0 at every pair - not positive definite until the ladder's jitter exceeds |R_11| (level 1 for -2e-6 and -5e-6,
    level 2 for -2e-5) - while Sp C^T has a zero second column, so the gain's solve with the unjittered S stays well conditioned
    in float32.  The second channel of Y is scaled to the size of sqrt(jitter), which keeps its share of ll of order 1."""
    args, mask = F.inputs(2, 5, 3, masked=True, seed=1)
    args = [a.clone() for a in args]
    args[3][1, :] = 0.0
    args[4] = torch.tensor([[0.05, 0.0], [0.0, r11]])
    args[8][..., 1] *= 1e-3
    return tuple(args), mask


def ladder(DEV, r11, level):
    """Every (b, t) of the float64 reference sits at ladder level `level` > 0; the kernel's levels are the reference's; every
    gradient under the bars."""
    args, mask = ladder_inputs(r11)
    g_ll, g_seq = upstream(2, 5, 11)
    g_ll, g_seq = g_ll.float().double(), g_seq.float().double()
    ref = restated(args, mask, g_ll, g_seq, torch.float64)
    assert level > 0 and bool((ref["levels"] == level).all()), ref["levels"]
    got = raw(DEV, args, mask, g_ll, g_seq)
    assert torch.equal(got["levels"].cpu(), ref["levels"])
    assert torch.equal(got["ll_recomputed"], got["ll"])
    filt = F.run(DEV, args, mask, impl="hip")
    assert torch.equal(got["ll"], filt["log_lik"]) and torch.equal(got["levels"], filt["levels"])
    check(got, ref, mask, what="ladder %g" % r11)


# ---- against existing code, on the kernel ------------------------------------------------------------------------------------
def vs_log_marginal(DEV, K, B=3, T=9):
    """K identical regimes (K = 1: the one regime): gY, gU, gC and gA summed over k agree with
    KalmanFilter.log_marginal(...)["seq_ll"].sum().backward() of the single regime, within the sum of the two bars (that adjoint's
    bars, pred_grad_cases.TOL, are about 5e-4 for gY and gC; both bars are taken from this file, the smaller, so the test asks
    more than the sum of the two)."""
    args, mask = F.inputs(B, T, K, masked=True, seed=7, shared=True)
    one = tuple(a[:1] if i < 3 else a for i, a in enumerate(args[:5])) + (F.prior(1),) + args[6:]
    kf1, kfK = F._kalman_filter(one, DEV), F._kalman_filter(args, DEV)
    kf1.train(), kfK.train()
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    y1, u1 = Y.clone().requires_grad_(True), U.clone().requires_grad_(True)
    kf1.dyn_params.reset_state()
    kf1.log_marginal(y1, u1, mk)["seq_ll"].sum().backward()
    yK, uK = Y.clone().requires_grad_(True), U.clone().requires_grad_(True)
    out = kfK.regime_log_marginal(yK, uK, mk)
    out["seq_ll"].sum().backward()
    d1, dK = kf1.dyn_params, kfK.dyn_params
    pairs = {"gY": (yK.grad, y1.grad), "gU": (uK.grad, u1.grad), "gC": (dK.C.grad.sum(0), d1.C.grad.sum(0)),
             "gA": (dK.A.grad.sum(0), d1.A.grad.sum(0))}
    for k, (g, w) in pairs.items():
        d = _slices(k, g, w.cpu().double())
        print("vs log_marginal", K, k, d, 2 * TOL[k])
        assert d < 2 * TOL[k], (k, d)


# ---- routing -----------------------------------------------------------------------------------------------------------------
def routing(DEV):
    """K = 9, n = 5, float64 and host tensors take the restatement; impl="hip" raises there; a state raises ValueError."""
    import pytest
    from kvae.kalman import lgssm_ops
    for case in ((2, 3, 9, 4, 2, False), (2, 3, 3, 5, 2, True)):
        args, mask = F.inputs(*case, seed=8)
        a = [t.to(DEV).clone().requires_grad_(i != 4) for i, t in enumerate(args)]
        out = lgssm_ops.switching_log_marginal(*a, mask=mask)
        out["seq_ll"].sum().backward()
        assert out["ll"].dtype == torch.float32 and all(bool(torch.isfinite(t.grad).all()) for i, t in enumerate(a) if i != 4)
        with pytest.raises(ValueError, match="impl='hip'"):
            lgssm_ops.switching_log_marginal(*a, mask=mask, impl="hip")
    args, mask = F.inputs(2, 3, 2)
    a64 = [t.to(DEV).double() for t in args]
    assert lgssm_ops.switching_log_marginal(*a64, mask=mask)["ll"].dtype == torch.float64
    with pytest.raises(ValueError, match="impl='hip'"):
        lgssm_ops.switching_log_marginal(*a64, mask=mask, impl="hip")
    a32 = [t.to(DEV) for t in args]
    with pytest.raises(ValueError, match="state"):
        lgssm_ops.switching_log_marginal(*a32, mask=mask, state={"log_w": torch.zeros(2, 2), "mu": torch.zeros(2, 2, 4),
                                                                 "Sigma": torch.zeros(2, 2, 4, 4)})
    with pytest.raises(ValueError):
        lgssm_ops.switching_log_marginal(*a32, mask=mask, impl="kernel")
    forced = lgssm_ops.switching_log_marginal(*a32, mask=mask, impl="torch")
    assert float((forced["ll"].cpu() - lgssm_ops.switching_log_marginal(*a32, mask=mask)["ll"].cpu()).abs().max()) < 1e-4


def host_tensors_take_the_restatement():
    """Without a backend for host tensors (the GPU tier: nothing injected) the op on CPU tensors is the restatement."""
    from kvae.kalman import lgssm_ops
    args, mask = F.inputs(2, 3, 2)
    a = lgssm_ops.switching_log_marginal(*args, mask=mask)
    b = lgssm_ops.switching_log_marginal_torch(*args, mask=mask)
    assert torch.equal(a["ll"], b["ll"])


# ---- the C ABI through raw pointers ------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """Every error code, and under each not a byte of any output, of the history or of the workspace written."""
    from kvae import _native as N
    B, T, K, n, m = 2, 3, 3, 4, 2
    args, mask = F.inputs(B, T, K, n, m, masked=True)
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), mask=mask.to(DEV))
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    # buffers large enough for the shapes the failing calls claim (K = 9, n = 5) too
    fo = dict(ll=big(B, T), seq_ll=big(B), levels=big(B, T, dt=torch.int32), regime_filt=big(B, T, 9), mus_filt=big(B, T, 5))
    hist = dict(hist_lw=big(B, T, 9), hist_mu=big(B, T, 9, 5), hist_Sigma=big(B, T, 9, 5, 5))
    go = dict(ws=big(B, 9 * 75 + 10 + 81 + 5 + 25), ll_recomputed=big(B, T), gA=big(9, 5, 5), gB=big(9, 5, 5), gQ=big(9, 5, 5), gC=big(2, 5), g_logP=big(9, 9),
              g_mu0=big(5), g_Sigma0=big(5, 5), gY=big(B, T, 2), gU=big(B, T, 5))
    up = dict(g_ll=torch.ones(B, T, device=DEV), g_seq=torch.ones(B, device=DEV))
    st = dict(state_log_w=torch.zeros(B, 9, device=DEV), state_mu=torch.zeros(B, 9, 5, device=DEV),
              state_Sigma=torch.eye(5, device=DEV).repeat(B, 9, 1, 1))

    def problem(drop=(), **kw):
        sp = N.SwmProblem()
        pr = sp.filt
        pr.B, pr.T, pr.K, pr.n, pr.m, pr.p = B, T, K, n, m, 2
        for k, v in list(ins.items()) + list(fo.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in hist.items():
            if k not in drop:
                setattr(sp, k, v.data_ptr())
        for k, v in kw.items():
            setattr(pr, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        return sp

    def fwd(drop=(), **kw):
        rc = lib.dll.kvae_lgssm_switching_marginal(C.byref(problem(drop, **kw)), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    def bwd(drop=(), gdrop=(), **kw):
        g = N.SwmGrads()
        for k, v in list(up.items()) + list(go.items()):
            if k not in gdrop:
                setattr(g, k, v.data_ptr())
        rc = lib.dll.kvae_lgssm_switching_marginal_bwd(C.byref(problem(drop, **kw)), C.byref(g), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    untouched = lambda *groups: all(bool((v == 7).all()) for grp in groups for v in grp.values())
    assert lib.dll.kvae_lgssm_switching_marginal(None, None) == 2 and lib.dll.kvae_lgssm_switching_marginal_bwd(None, None, None) == 2
    for call in (fwd, bwd):
        for k in names + tuple(hist):
            assert call(drop=(k,)) == 2, k                                  # KVAE_ERR_NULL
        assert call(drop=("ll",)) == 2                                      # seq_ll reads ll
        for kw in (dict(B=0), dict(T=0), dict(B=-1)):
            assert call(**kw) == 1, kw                                      # KVAE_ERR_DIMS
        for kw in (dict(K=9), dict(K=0), dict(n=5), dict(n=0), dict(m=5), dict(p=3)):
            assert call(**kw) == 4, kw                                      # KVAE_ERR_ARG
        assert call(state_log_w=st["state_log_w"]) == 4                     # a partial state, and a whole one
        assert call(**st) == 4 and call(drop=("mu0", "Sigma0"), **st) == 4
    assert lib.dll.kvae_lgssm_switching_marginal_bwd(C.byref(problem()), None, None) == 2
    assert bwd(gdrop=("g_ll", "g_seq")) == 2 and bwd(gdrop=("ws",)) == 2
    assert untouched(fo, hist, go)
    assert bwd(gdrop=tuple(k for k in go if k != "ws")) == 0 and untouched(go)          # no output asked for: no launch
    assert fwd() == 0 and not untouched(hist) and bwd() == 0
    assert not any(bool((v.reshape(-1)[:2] == 7).all()) for grp in (fo, hist, go) for v in grp.values())
    assert bwd(gdrop=("g_ll",)) == 0 and bwd(gdrop=("g_seq",)) == 0 and bwd(drop=("mask",)) == 0


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _model_case(DEV, K=3, B=3, T=12):
    """swf_cases' model-level case (the small switching KVAE, a mask, a random u) in training mode, and the encodings of its frames."""
    model, x, mask, u, _ = F._model_case(DEV, K, B, T)
    model.eval()
    with torch.no_grad():
        a = model.encode_sequence(x, sample=False)[0]
    model.train()
    return model, a.detach().cpu(), u.cpu(), mask, x.cpu()


def _model_restated(model, a, u, mask, dtype):
    """seq_ll and its gradients w.r.t. a, u and the dynamics' A, B, Q, C from autograd of the restatement over the state_dict."""
    from kvae.kalman import lgssm_ops
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().to(dtype).clone()
    leaves = {"A": d(dyn.A), "B": d(dyn.B), "Q": d(dyn.Q), "C": d(dyn.C), "a": d(a), "u": d(u)}
    for v in leaves.values():
        v.requires_grad_(True)
    out = lgssm_ops.switching_log_marginal_torch(leaves["A"], leaves["B"], leaves["Q"], leaves["C"][0], d(kf.R),
                                                 dyn.prior.transition_matrix.to(dtype), d(kf.mu0), d(kf.Sigma0), leaves["a"], leaves["u"], mask=mask)
    out["seq_ll"].sum().backward()
    return out, {k: v.grad for k, v in leaves.items()}


def model_yardsticks():
    model, a, u, mask, _ = _model_case("cpu")
    (_, g32), (_, g64) = _model_restated(model, a, u, mask, torch.float32), _model_restated(model, a, u, mask, torch.float64)
    return {k: _slices("gA", g32[k], g64[k]) for k in g64}


def model_level(DEV):
    """regime_log_marginal(...)["seq_ll"].sum().backward() against float64 autograd of the restatement over the state_dict: a, u, A,
    B, Q, C per tensor; the posterior network's parameters get no gradient; lstm dynamics raise."""
    import pytest
    model, a, u, mask, _ = _model_case(DEV)
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    ak, uk = a.to(DEV).requires_grad_(True), u.to(DEV).requires_grad_(True)
    model.zero_grad()
    out = kf.regime_log_marginal(ak, uk, mask.to(DEV))
    filt = kf.filter_regimes(ak.detach(), uk.detach(), mask.to(DEV))
    assert torch.equal(out["ll"], filt["log_lik"]) and torch.equal(out["seq_ll"], filt["log_lik_seq"]) and torch.equal(out["levels"], filt["levels"])
    out["seq_ll"].sum().backward()
    ref, g64 = _model_restated(model, a, u, mask, torch.float64)
    assert int(ref["levels"].max()) == 0
    got = {"a": ak.grad, "u": uk.grad, "A": dyn.A.grad, "B": dyn.B.grad, "Q": dyn.Q.grad, "C": dyn.C.grad}
    for k, v in got.items():
        dist = _slices("gA", v, g64[k])
        print("model", k, dist, MODEL_TOL[k])
        assert dist < MODEL_TOL[k], (k, dist)
    assert bool((dyn.C.grad[1:] == 0).all())                                  # the switching model emits through C[0] alone
    post = [p for k, p in dyn.named_parameters() if k not in ("A", "B", "C", "Q")]
    assert post and all(p.grad is None for p in post)
    lstm = F.small_model("lstm").to(DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.kalman_filter.regime_log_marginal(torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 3, lstm.u_dim, device=DEV))
    with pytest.raises(ValueError, match="kf_objective"):
        lstm.compute_loss(torch.zeros(2, 3, 1, 32, 32, device=DEV), {}, kf_objective="regime_marginal")


def model_compute_loss(DEV):
    """compute_loss(kf_objective="regime_marginal"): elbo_kf = log_lik_seq.sum() / num_el of filter_regimes over the same a; a
    training-mode forward returns None for the LGSSM stacks; "elbo" and the default are bit-identical under injected noise before
    and after a regime_marginal step; the Trainer still refuses an unknown objective."""
    import pytest
    from kvae import noise
    from kvae.train.train import Trainer
    model, _, u, mask, x = _model_case(DEV)
    K = model.K
    x, u, mask = x.to(DEV), u.to(DEV), mask.to(DEV)
    B, T = x.shape[:2]
    g = torch.Generator().manual_seed(3)
    nz = dict(eps_a=torch.randn(B * T, model.a_dim, generator=g).to(DEV), eps_z=torch.randn(B, T, model.z_dim, generator=g).to(DEV),
              gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV))

    def step(objective):
        model.zero_grad()
        model.kalman_filter.dyn_params.reset_state()
        if objective is not None:
            model.kf_objective = objective
        try:
            with noise.inject(**nz):
                out = model(x, u=u, mask=mask)
                losses = model.compute_loss(x, out, mask=mask, with_metrics=False)
        finally:
            model.__dict__.pop("kf_objective", None)
        losses["loss"].backward()
        return out, losses, {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}

    _, l_d, g_d = step(None)
    out_r, l_r, g_r = step("regime_marginal")
    for k in ("mus_smooth", "Sigmas_smooth", "mus_filt", "Sigmas_filt", "mus_pred", "Sigmas_pred", "state_probs"):
        assert out_r[k] is None, k
    assert out_r["ABC"] == (None, None, None)
    with torch.no_grad():
        f = model.kalman_filter.filter_regimes(out_r["a_samples"].detach(), u, mask, want=("log_lik_seq",))
    want = float(f["log_lik_seq"].double().sum() / mask.sum().double())
    bar = F.MODEL_TOL["log_lik_seq"] * B / float(mask.sum())
    print("elbo_kf", float(l_r["elbo_kf"]), want, abs(float(l_r["elbo_kf"]) - want), "bar", bar)
    assert abs(float(l_r["elbo_kf"]) - want) <= bar, (float(l_r["elbo_kf"]), want, bar)
    for k, p in model.named_parameters():
        if "regime_posterior" in k or "posterior" in k:
            assert g_r[k] is None, k
        elif p.requires_grad and not k.startswith("kalman_filter.dyn_params.C"):
            assert g_r[k] is not None and bool(torch.isfinite(g_r[k]).all()), k
    _, l_e, g_e = step("elbo")
    assert torch.equal(l_d["loss"], l_e["loss"]) and torch.equal(l_d["elbo_kf"], l_e["elbo_kf"])
    for k in g_d:
        assert (g_d[k] is None and g_e[k] is None) or torch.equal(g_d[k], g_e[k]), k
    model.eval()
    model.kf_objective = "regime_marginal"
    try:
        with torch.no_grad(), noise.inject(**nz):
            ev = model(x, u=u, mask=mask)
    finally:
        del model.kf_objective
    assert ev["mus_smooth"] is not None and ev["state_probs"] is not None
    model.train()
    with pytest.raises(ValueError, match="kf_objective"):
        Trainer(model, use_graph=False, kf_objective="nonsense")
    with pytest.raises(ValueError, match="kf_objective"):
        Trainer(F.small_model("lstm").to(DEV), use_graph=False, kf_objective="regime_marginal")


if __name__ == "__main__":
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "kalman-vae_amd"), str(root), str(root / "tests")]
    torch.set_num_threads(4)
    print("YARDSTICK", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print("MODEL_YARDSTICK", {k: float(f"{v:.3g}") for k, v in model_yardsticks().items()})
