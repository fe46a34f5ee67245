"""Device-agnostic cases of kvae_lgssm_predictive / lgssm_ops.predictive / KalmanFilter.predictive / KVAE.score /
KVAE.log_likelihood: run against the host simulation (tests/test_predictive.py: the kernel bodies of csrc/lgssm_pred.h on emulated
wavefronts) and against the gfx950 library (tests/test_gpu_predictive.py).  The reference of the kernel level is
lgssm_ops.predictive_torch in FLOAT64 on the same float32-rounded inputs; the joint-Gaussian case is independent of it (the
density of the stacked observed a_t assembled from the open-loop recursion).  The reference of the model level is a float64
restatement over the model's state_dict (oracle/torch_oracle.py) with the same injected draws."""
import itertools
import math

import torch

# (B, T, n) of the per-item parity, both tiers; p = 2.  The smallest at which each body can go wrong.
SHAPES_N4 = [(1, 1, 4), (3, 37, 4), (65, 6, 4), (2, 200, 4)]    # one item; a ragged last wavefront; B > 64 lanes; T = 200
SHAPES_N16 = [(2, 9, 16), (5, 13, 16), (2, 200, 16)]            # 65 items: not a multiple of four
SHAPES_RT = [(2, 7, 3), (3, 5, 7)]                              # the run-time-dimension body
SHAPES = SHAPES_N4 + SHAPES_N16 + SHAPES_RT
# beyond the list above: the sequence sums at one full and one-past-full stride of the wavefront (T = 1 and 200 are in SHAPES).
# Held to the bars measured on SHAPES.
SEQ_SHAPES = [(2, 64, 4), (2, 65, 4)]
CMODES = ("shared", "packed")   # one C [p,n] for all steps | C_t out of a packed step record with a row stride of its own
# Yardsticks, by the rule of parity_cases.RNN_YARDSTICK: the largest per-(b,t) ratio |got - ref| /
# max(1, |ref|) (max-norm within the slice for a_pred and S) of predictive_torch in FLOAT32 against its float64 run on the same
# rounded inputs, over SHAPES x CMODES, every step observed (rerun: python tests/pred_cases.py).  Bars = 4 x.
# Largest ratios the kernels reach against the same float64 run, host simulation | gfx950: DESIGN.md section 12.
YARDSTICK = {"ll": 4.43e-5, "nis": 1.36e-4, "a_pred": 1.39e-6, "S": 1.68e-6}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
OUTPUTS = ("ll", "nis", "a_pred", "S", "levels", "seq_ll")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: float64 draws rounded through float32, mus_pred / Sigmas_pred from a float64 filter with the reference's conventions
# ---------------------------------------------------------------------------------------------------------------------------
def filter64(A, Bm, C, Q, R, mu0, S0, Y, U, mask):
    """The reference's filter_step (kalman_filter.py:62-101 there) over T steps in float64: (mus_pred [B,T,n], Sigmas_pred)."""
    B, T, n = A.shape[:3]
    eye = torch.eye(n, dtype=torch.float64)
    mu, Sig = mu0.expand(B, n).unsqueeze(-1), S0.expand(B, n, n)
    mps, Sps = [], []
    for t in range(T):
        Ct = C if C.dim() == 2 else C[:, t]
        mp = A[:, t] @ mu + Bm[:, t] @ U[:, t].unsqueeze(-1)
        Sp = A[:, t] @ Sig @ A[:, t].mT + Q[:, t]
        S = Ct @ Sp @ Ct.mT + R
        S = 0.5 * (S + S.mT)
        K = torch.linalg.solve(S, (Sp @ Ct.mT).mT).mT * mask[:, t].view(B, 1, 1)
        mu = mp + K @ (Y[:, t].unsqueeze(-1) - Ct @ mp)
        IK = eye - K @ Ct
        Sig = IK @ Sp @ IK.mT + K @ R @ K.mT
        Sig = 0.5 * (Sig + Sig.mT)
        mps.append(mp.squeeze(-1)), Sps.append(Sp)
    return torch.stack(mps, 1), torch.stack(Sps, 1)


_IN = {}


def inputs(B, T, n, cmode="shared", mask=None, p=2):
    """One case: A = I + 0.1 N, B = 0.3 N, C = N, Q = L L^T + 0.01 I with L = 0.3 N, R = 0.03^2 I, mu0 = 0, Sigma0 = 20 I, Y, U = N,
    all float64 values that float32 holds exactly.  mask: random (30 % hidden) with t = 0 of the first and the last step of the
    last sequence hidden, and the whole second sequence where B >= 3 (a single item stays observed).  Returns the float64 model
    and, as float32 tensors, what the kernel reads: mp, Sp, C, R, Y, mask."""
    key = (B, T, n, cmode, None if mask is None else tuple(mask.flatten().tolist()), p)
    if key in _IN:
        return _IN[key]
    g = torch.Generator().manual_seed(100000 * (cmode == "packed") + 1000 * B + 10 * T + n)
    rnd = lambda t: t.float().double()
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    m = max(1, n // 4)
    A, Bm = rnd(eye + 0.1 * r(B, T, n, n)), rnd(0.3 * r(B, T, n, m))
    C = rnd(r(p, n)) if cmode == "shared" else rnd(r(B, T, p, n))
    L = 0.3 * r(B, T, n, n)
    Q = rnd(L @ L.mT + 0.01 * eye)
    Q = 0.5 * (Q + Q.mT)
    R = rnd(0.03 ** 2 * torch.eye(p, dtype=torch.float64))
    mu0, S0 = torch.zeros(n, dtype=torch.float64), 20.0 * eye
    Y, U = rnd(r(B, T, p)), rnd(r(B, T, m))
    if mask is None:
        mask = (torch.rand(B, T, generator=g) > 0.3).double()
        if B * T > 1:
            mask[0, 0] = 0
            mask[-1, -1] = 0
        if B >= 3:
            mask[1] = 0
    mask = mask.double()
    mp, Sp = filter64(A, Bm, C, Q, R, mu0, S0, Y, U, mask)
    case = dict(B=B, T=T, n=n, p=p, cmode=cmode, A=A, Bm=Bm, C=C, Q=Q, R=R, mu0=mu0, S0=S0, Y=Y, U=U, mask=mask, mp64=mp, Sp64=Sp,
                k=dict(mp=mp.float(), Sp=Sp.float(), C=C.float(), R=R.float(), Y=Y.float(), mask=mask.float()))
    _IN[key] = case
    return case


_REF = {}


def reference(case, masked=True, dtype=torch.float64):
    """predictive_torch in `dtype` on the float32-rounded kernel inputs of the case; the float64 runs are computed once and shared."""
    from kvae.kalman import lgssm_ops
    key = (id(case), masked, dtype)
    if key not in _REF:
        k = case["k"]
        _REF[key] = lgssm_ops.predictive_torch(k["mp"].to(dtype), k["Sp"].to(dtype), k["C"].to(dtype), k["R"].to(dtype), k["Y"].to(dtype),
                                               k["mask"].to(dtype) if masked else None)
    return _REF[key]


def shift(t):
    """The same values in a buffer that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    off = 1 + ((16 - buf.data_ptr() % 16) % 16) // 4
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def run(DEV, case, masked=True, want=OUTPUTS, unaligned=False, pad=4, impl="kernel"):
    """lgssm_ops.predictive on DEV.  cmode "packed": C_t is read out of a step record [B,T,pad + p n + 4] at float offset `pad`
    (pad = 4: rows and slots 16-byte aligned, pad = 3: not).  unaligned: every operand a view offset by one float."""
    from kvae.kalman import lgssm_ops
    k = {name: t.to(DEV) for name, t in case["k"].items()}
    B, T, n, p = case["B"], case["T"], case["n"], case["p"]
    packed, slots, Cm = None, lgssm_ops.Slots(), k["C"]
    if case["cmode"] == "packed" and not unaligned:
        packed = torch.cat([torch.zeros(B, T, pad, device=DEV), k["C"].flatten(2), torch.zeros(B, T, 4, device=DEV)], -1).contiguous()
        slots = lgssm_ops.Slots(C=pad)
        Cm = packed[..., pad:pad + p * n].unflatten(-1, (p, n))
    if unaligned:
        k = {name: shift(t) for name, t in k.items()}
        Cm = k["C"]
    return lgssm_ops.predictive(k["mp"], k["Sp"], Cm, k["R"], k["Y"], k["mask"] if masked else None, packed=packed, slots=slots,
                                want=want, impl=impl)


def ratios(got, ref):
    """Largest per-(b,t) ratio |got - ref| / max(1, |ref|) of each output (max-norm within the slice for a_pred and S)."""
    c = lambda t: t.detach().cpu().double()
    out = {}
    for name, red in (("ll", None), ("nis", None), ("a_pred", (-1,)), ("S", (-1, -2))):
        if got.get(name) is None:
            continue
        err, scale = (c(got[name]) - ref[name]).abs(), ref[name].abs()
        if red is not None:
            err, scale = err.amax(red), scale.amax(red)
        out[name] = float((err / scale.clamp_min(1.0)).max())
    return out


def check_seq(got_seq, ref_ll, mask):
    """seq_ll against the float64 sum: T_obs x (ll bar) x max(1, largest |ll_t| of the sequence); exactly 0 with nothing observed."""
    got_seq = got_seq.detach().cpu().double()
    for b in range(ref_ll.shape[0]):
        t_obs = int(mask[b].sum())
        if t_obs == 0:
            assert float(got_seq[b]) == 0.0, (b, float(got_seq[b]))
            continue
        bar = t_obs * TOL["ll"] * max(1.0, float(ref_ll[b].abs().max()))
        assert abs(float(got_seq[b] - ref_ll[b].sum())) <= bar, (b, float(got_seq[b]), float(ref_ll[b].sum()), bar)


def check(DEV, B, T, n, cmode="shared", masked=True, worst=None, **kw):
    """All six outputs of one call against the float64 run under TOL; every ladder level 0 (no item is left out of the
    comparison); hidden steps exactly 0 in ll and nis."""
    case = inputs(B, T, n, cmode)
    got, ref = run(DEV, case, masked, **kw), reference(case, masked)
    assert int(ref["levels"].abs().max()) == 0 and int(reference(case, masked, torch.float32)["levels"].abs().max()) == 0
    assert got["levels"].dtype == torch.int32 and int(got["levels"].abs().max()) == 0
    figs = ratios(got, ref)
    print("predictive", DEV, (B, T, n), cmode, "masked" if masked else "observed", kw, figs)
    for name, v in figs.items():
        assert v < TOL[name], (name, v, TOL[name])
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), v)
    mask = case["mask"] if masked else torch.ones(B, T, dtype=torch.float64)
    check_seq(got["seq_ll"], ref["ll"], mask)
    hidden = mask == 0
    assert not bool(got["ll"].cpu()[hidden].any()) and not bool(got["nis"].cpu()[hidden].any())
    assert bool(torch.isfinite(got["a_pred"]).all()) and bool(torch.isfinite(got["S"]).all())
    return got


def yardsticks():
    """The float32 torch restatement against the float64 one over SHAPES x CMODES: the numbers YARDSTICK holds."""
    worst = {k: 0.0 for k in YARDSTICK}
    for (B, T, n), cmode in itertools.product(SHAPES, CMODES):
        case = inputs(B, T, n, cmode)
        f32, ref = reference(case, False, torch.float32), reference(case, False)
        assert int(f32["levels"].abs().max()) == 0 and int(ref["levels"].abs().max()) == 0
        for name, v in ratios(f32, ref).items():
            worst[name] = max(worst[name], v)
    return worst


# ---- independent of the restatement: the joint Gaussian of the stacked observed a_t ------------------------------------------
def joint_gaussian(DEV, B, T, n):
    """log N(stacked observed a; open-loop means, covariance blocks C_s P_s (A_{s+1..t})^T C_t^T (+ R on the diagonal)) in
    float64 against the kernel's seq_ll, under the seq_ll bar.  t = 0 hidden in the first sequence, the last step in the last."""
    mask = torch.ones(B, T)
    mask[0, 0] = 0
    mask[-1, -1] = 0
    d = inputs(B, T, n, "packed", mask=mask)
    p = d["p"]
    got = run(DEV, d)
    ref = reference(d)
    # the decomposition with nothing rounded and no jitter (the ladder's level 0 adds 1e-6 I to S_t, which the bar absorbs)
    S = d["C"] @ d["Sp64"] @ d["C"].mT + d["R"]
    Lc = torch.linalg.cholesky(0.5 * (S + S.mT))
    w = torch.linalg.solve_triangular(Lc, (d["Y"] - (d["C"] @ d["mp64"].unsqueeze(-1)).squeeze(-1)).unsqueeze(-1), upper=False).squeeze(-1)
    exact = -0.5 * ((w * w).sum(-1) + 2 * Lc.diagonal(dim1=-2, dim2=-1).log().sum(-1) + p * math.log(2 * math.pi)) * d["mask"]
    eye = torch.eye(n, dtype=torch.float64)
    for b in range(B):
        m, P, mz, Pz = d["mu0"], d["S0"], [], []
        for t in range(T):
            m = d["A"][b, t] @ m + d["Bm"][b, t] @ d["U"][b, t]
            P = d["A"][b, t] @ P @ d["A"][b, t].mT + d["Q"][b, t]
            mz.append(m), Pz.append(P)
        obs = [t for t in range(T) if d["mask"][b, t] > 0]
        k = len(obs)
        mean = torch.cat([d["C"][b, t] @ mz[t] for t in obs])
        cov = torch.zeros(k * p, k * p, dtype=torch.float64)
        for (i, s), (j, t) in itertools.product(enumerate(obs), enumerate(obs)):
            if s <= t:
                F = eye
                for q in range(s + 1, t + 1):
                    F = d["A"][b, q] @ F
                blk = d["C"][b, s] @ Pz[s] @ F.mT @ d["C"][b, t].mT + (d["R"] if s == t else 0)
                cov[i * p:(i + 1) * p, j * p:(j + 1) * p] = blk
                cov[j * p:(j + 1) * p, i * p:(i + 1) * p] = blk.mT
        y = torch.cat([d["Y"][b, t] for t in obs])
        joint = float(torch.distributions.MultivariateNormal(mean, 0.5 * (cov + cov.mT)).log_prob(y))
        assert abs(float(exact[b].sum()) - joint) <= 1e-7 * abs(joint), (float(exact[b].sum()), joint)   # the identity, in float64
        bar = k * TOL["ll"] * max(1.0, float(ref["ll"][b].abs().max()))
        mine = float(got["seq_ll"][b])
        print("joint", DEV, (B, T, n, b), mine, joint, abs(mine - joint), bar)
        assert abs(mine - joint) <= bar, (mine, joint, bar)


# ---- subsets of the outputs, repeatability --------------------------------------------------------------------------------------
def partial_outputs(DEV, B, T, n, cmode="packed"):
    """Every subset of `want` (NULL output pointers in the call) gives the bits of the full call and None for the rest; two full
    calls are bit-identical."""
    case = inputs(B, T, n, cmode)
    full, again = run(DEV, case), run(DEV, case)
    for k in OUTPUTS:
        assert torch.equal(full[k], again[k]), k
    for r in range(1, len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, r):
            part = run(DEV, case, want=want)
            for k in OUTPUTS:
                if k in want:
                    assert torch.equal(part[k], full[k]), (want, k)
                else:
                    assert part[k] is None, (want, k)


# ---- the ladder -------------------------------------------------------------------------------------------------------------
LADDER_EIG = -1.0001e-4   # -1e-4, a hair past float32(1e-4) (the level-2 jitter) so that rounding cannot decide the level


def ladder(DEV, n, b=1, t=3, B=3, T=6, impl="kernel"):
    """Sigma_{t|t-1} of one item replaced by an indefinite matrix for which S_t has the eigenvalues (-1e-4, 2e-3): levels 0..2
    fail (pivot <= 0) and level 3 (jitter 1e-3) factorises.  The item is built at the scale of R, so that float32 holds S_t to
    1e-10 and the comparison under the ll bar is meaningful.  Its neighbours stay at level 0."""
    from kvae.kalman import lgssm_ops
    base = inputs(B, T, n, "packed", mask=torch.ones(B, T))
    case = dict(base, k={name: v.clone() for name, v in base["k"].items()})
    C, R = case["k"]["C"][b, t].double(), case["k"]["R"].double()
    g = torch.Generator().manual_seed(7)
    V, _ = torch.linalg.qr(torch.randn(2, 2, generator=g, dtype=torch.float64))
    W = torch.linalg.pinv(C) @ V                                        # C W = V
    target = V @ torch.diag(torch.tensor([LADDER_EIG, 2e-3], dtype=torch.float64)) @ V.T - R
    Sp = W @ (V.T @ target @ V) @ W.T
    case["k"]["Sp"][b, t] = (0.5 * (Sp + Sp.T)).float()
    args = lambda dt: [case["k"][name].to(dt) for name in ("mp", "Sp", "C", "R", "Y")]
    ref = lgssm_ops.predictive_torch(*args(torch.float64))
    S64 = ref["S"][b, t]
    lam = float(torch.linalg.eigvalsh(S64)[0])
    assert abs(lam - LADDER_EIG) < 1e-8 and float(torch.linalg.eigvalsh(case["k"]["Sp"][b, t].double())[0]) < 0, lam
    got = run(DEV, case, masked=False, impl=impl)
    lv = got["levels"].cpu()
    assert int(lv[b, t]) >= 1 and int(lv[b, t]) == int(ref["levels"][b, t]) == 3, (int(lv[b, t]), int(ref["levels"][b, t]))
    others = torch.ones(B, T, dtype=torch.bool)
    others[b, t] = False
    assert not bool(lv[others].any()) and not bool(ref["levels"][others].any())
    figs = ratios(got, ref)       # the float64 run took the same level: the comparison is at that level
    print("ladder", DEV, n, impl, "level", int(lv[b, t]), "eig", lam, "ll", float(got["ll"][b, t]), float(ref["ll"][b, t]), figs)
    for name, v in figs.items():
        assert v < TOL[name], (name, v, TOL[name])
    check_seq(got["seq_ll"], ref["ll"], torch.ones(B, T))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """The error codes of include/kvae_lgssm.h through raw pointers."""
    import ctypes as C
    from kvae import _native as N
    buf = torch.zeros(4096, device=DEV)
    lv = torch.zeros(64, dtype=torch.int32, device=DEV)
    ptr = buf.data_ptr()

    def prob(**kw):
        pr = N.PredProblem()
        pr.B, pr.T, pr.n, pr.p = 2, 3, 4, 2
        for k in ("mus_pred", "Sigmas_pred", "R", "y", "mask", "ll", "nis", "a_pred", "S_out", "seq_ll"):
            setattr(pr, k, ptr)
        pr.levels = lv.data_ptr()
        pr.C = N.Stack(ptr, 0, 0)
        for k, v in kw.items():
            setattr(pr, k, v)
        return pr

    call = lambda pr: lib.dll.kvae_lgssm_predictive(C.byref(pr), None)
    assert call(prob()) == 0
    for kw in (dict(B=0), dict(T=0), dict(B=-1), dict(n=0), dict(n=17), dict(p=0), dict(p=17), dict(p=3)):
        assert call(prob(**kw)) == 1, kw                                        # KVAE_ERR_DIMS
    for kw in (dict(mus_pred=None), dict(Sigmas_pred=None), dict(R=None), dict(y=None), dict(C=N.Stack(None, 0, 0)), dict(ll=None)):
        assert call(prob(**kw)) == 2, kw                                        # KVAE_ERR_NULL (seq_ll without ll)
    assert lib.dll.kvae_lgssm_predictive(None, None) == 2
    for kw in (dict(C=N.Stack(ptr, -1, 0)), dict(C=N.Stack(ptr, 0, -8))):
        assert call(prob(**kw)) == 4, kw                                        # KVAE_ERR_ARG
    assert call(prob(mask=None)) == 0 and call(prob(ll=None, seq_ll=None)) == 0
    assert call(prob(ll=None, nis=None, a_pred=None, S_out=None, levels=None, seq_ll=None)) == 0   # nothing asked: no launch
    if DEV != "cpu":
        torch.cuda.synchronize()


def unsupported_takes_torch(DEV):
    """a_dim 3 and float64 tensors are outside the kernel: the Python layer takes predictive_torch; forcing the kernel raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    case = inputs(2, 5, 4, "shared", p=3)
    k = {name: t.to(DEV) for name, t in case["k"].items()}
    assert not lgssm_ops.predictive_supported(4, 3, k["Sp"]) and not lgssm_ops.predictive_supported(17, 2)
    assert not lgssm_ops.predictive_supported(4, 2, k["Sp"].double())
    got = lgssm_ops.predictive(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], k["mask"])
    ref = reference(case)
    assert got["S"].shape == (2, 5, 3, 3) and all(v < 1e-4 for v in ratios(got, ref).values())
    with pytest.raises(RuntimeError):
        lgssm_ops.predictive(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], k["mask"], impl="kernel")
    with pytest.raises(ValueError):
        lgssm_ops.predictive(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], want=("lls",))
    d = inputs(2, 5, 4, "shared")
    k64 = {name: t.double().to(DEV) for name, t in d["k"].items()}
    out = lgssm_ops.predictive(k64["mp"], k64["Sp"], k64["C"], k64["R"], k64["Y"], k64["mask"])
    assert out["ll"].dtype == torch.float64 and float((out["ll"].cpu() - reference(d)["ll"]).abs().max()) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
MODELS = [("lstm", 3), ("switching", 3), ("switching", 7)]
# Yardsticks of the model level: the float32 run of the float64 restatement below (plain torch on the host) against its float64
# run, same injected draws, largest ratio |f32 - f64| / max(1, |f64|) per entry over MODELS (rerun: the CPU tier's
# test_model_yardsticks prints them).  Bars = 4 x.  What the product reaches: DESIGN.md section 12.
MODEL_YARDSTICK = {"log_lik": 5.04e-7, "nis": 2.17e-8, "a_pred": 1.72e-8, "S": 4.76e-8, "log_lik_seq": 1.95e-7,
                   "log_px_a": 1.22e-7, "log_pa": 2.94e-7, "log_qa": 1.55e-7, "log_ps_qs": 2.94e-7, "log_px": 1.27e-7, "elbo": 8.21e-8}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}
SCORE_KEYS = ("log_lik", "nis", "a_pred", "S", "log_lik_seq")
LL_KEYS = ("log_px_a", "log_pa", "log_qa", "log_ps_qs", "log_px", "elbo")


def small_model(kind="lstm", K=3):
    from post_cases import small_model as make
    return make(kind, K)


def model_inputs(model, K, B=2, T=10, S=3, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 17 + K)
    x = (torch.rand(B, T, 1, 32, 32, generator=g) > 0.7).float()
    u = 0.3 * torch.randn(B, T, model.u_dim, generator=g)
    mask = torch.ones(B, T)
    mask[:, 4:8] = 0
    gum = lambda rows: -torch.empty(rows, T, K).exponential_(generator=g).log()
    return dict(x=x, u=u, mask=mask, S=S, eps_a=torch.randn(B * T, model.a_dim, generator=g), gumbel=gum(B),
                ll_a=torch.randn(B, S, T, model.a_dim, generator=g), gumbel_rows=gum(B * S))


def _state(model, dtype):
    return {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}


def _kf(sd):
    return sd["kalman_filter.Q"], sd["kalman_filter.R"], sd["kalman_filter.mu0"], sd["kalman_filter.Sigma0"]


def score_restated(model, x, u, mask, dtype, path=None, gumbel=None):
    """KVAE.score over the model's state_dict in `dtype`, plain torch on the host: the oracle's encoder and filter
    (oracle/torch_oracle.py), predictive_torch over its one-step-ahead beliefs.  path [B,T]: the pinned regimes
    (regimes="map"); else gumbel [B,T,K] for the eval-mode draw."""
    from kvae.kalman import lgssm_ops
    from oracle import torch_oracle as O
    sd, cfg = _state(model, dtype), model.config
    kind = cfg.dynamics_model.lower()
    B, T = x.shape[:2]
    a_mu, _ = O.encoder(sd, x.flatten(0, 1).to(dtype), cfg.noise_emission)
    a = a_mu.unflatten(0, (B, T))
    return _predict_restated(model, sd, kind, a, u.to(dtype), None if mask is None else mask.to(dtype), path, gumbel), a


def _predict_restated(model, sd, kind, a, u, mask, path, gumbel):
    from kvae.kalman import lgssm_ops
    from oracle import torch_oracle as O
    dyn = O.split_dyn(sd)
    Qb, R, mu0, S0 = _kf(sd)
    B, T = a.shape[:2]
    dt = a.dtype
    mk = torch.ones(B, T, dtype=dt) if mask is None else mask
    extra = {}
    if kind == "switching" and path is not None:
        A, Bm, Q, Cm = dyn["A"][path], dyn["B"][path], dyn["Q"][path], dyn["C"][0].expand(B, T, -1, -1)
        mu, Sig = mu0.expand(B, -1).unsqueeze(-1), S0.expand(B, -1, -1)
        mps, Sps = [], []
        for t in range(T):
            mu, Sig, mu_p, Sig_p = O.filter_step(mu, Sig, a[:, t], u[:, t], A[:, t], Bm[:, t], Cm[:, t], Q[:, t], R, mk[:, t])
            mps.append(mu_p), Sps.append(Sig_p)
        mp, Sp = torch.stack(mps, 1), torch.stack(Sps, 1)
    else:
        dynp = model.kalman_filter.dyn_params
        out = O.lgssm_filter(a, u, mk, dyn, kind, Qb, R, mu0, S0, tau=float(getattr(dynp, "tau", 1.0)), is_training=False,
                             gumbel=None if gumbel is None else gumbel.to(dt),
                             trans_matrix=dynp.prior.transition_matrix.to(dt) if kind == "switching" else None)
        mp, Sp, Cm = out["mus_pred"], out["Sigmas_pred"], out["C_list"]
        if kind == "switching":
            extra["log_ps_qs"] = (out["log_pseq"] - out["log_qseq"]).sum(-1)
    pred = lgssm_ops.predictive_torch(mp.squeeze(-1), Sp, Cm, R, a, mask)
    return dict(log_lik=pred["ll"], nis=pred["nis"], a_pred=pred["a_pred"], S=pred["S"], log_lik_seq=pred["seq_ll"], **extra)


def log_likelihood_restated(model, x, u, mask, S, dtype, ll_a, gumbel_rows):
    """KVAE.log_likelihood over the model's state_dict in `dtype`, plain torch on the host, the same draws."""
    from oracle import torch_oracle as O
    sd, cfg = _state(model, dtype), model.config
    kind = cfg.dynamics_model.lower()
    B, T = x.shape[:2]
    x = x.to(dtype)
    a_mu, a_var = (t.unflatten(0, (B, T)) for t in O.encoder(sd, x.flatten(0, 1), cfg.noise_emission))
    a_s = a_mu[:, None] + a_var.sqrt()[:, None] * ll_a.to(dtype)
    rows = a_s.reshape(B * S, T, -1)
    rep = lambda t: t.to(dtype).repeat_interleave(S, 0)
    mk = torch.ones(B, T, dtype=dtype) if mask is None else mask.to(dtype)
    pred = _predict_restated(model, sd, kind, rows, rep(u), rep(mk), None, gumbel_rows)
    log_pa = pred["log_lik_seq"].view(B, S)
    log_ps_qs = pred["log_ps_qs"].view(B, S) if "log_ps_qs" in pred else torch.zeros(B, S, dtype=dtype)
    logits = O.decoder(sd, rows.flatten(0, 1)).unflatten(0, (B, S, T))
    bce = torch.nn.functional.binary_cross_entropy_with_logits(logits, x[:, None].expand_as(logits), reduction="none")
    log_px_a = (-bce.sum(dim=(3, 4, 5)) * mk[:, None]).sum(-1)
    log_qa = (O.log_gaussian(a_s, a_mu[:, None], a_var[:, None]).sum(-1) * mk[:, None]).sum(-1)
    log_w = log_px_a + log_pa - log_qa + log_ps_qs
    return dict(log_px_a=log_px_a, log_pa=log_pa, log_qa=log_qa, log_ps_qs=log_ps_qs, log_w=log_w,
                log_px=torch.logsumexp(log_w, 1) - math.log(S), elbo=log_w.mean(1), n_obs=mk.sum(1))


def _ratio(got, ref):
    return float(((got.detach().cpu().double() - ref.double()).abs() / ref.double().abs().clamp_min(1.0)).max())


def model_yardsticks(paths):
    """The float32 run of the restatement against its float64 run over MODELS; paths: {(kind, K): the pinned regime path}."""
    worst = {k: 0.0 for k in MODEL_YARDSTICK}
    for kind, K in MODELS:
        model = small_model(kind, K)
        d = model_inputs(model, K)
        runs = {}
        for dt in (torch.float32, torch.float64):
            sc, _ = score_restated(model, d["x"], d["u"], d["mask"], dt, path=paths.get((kind, K)))
            ll = log_likelihood_restated(model, d["x"], d["u"], d["mask"], d["S"], dt, d["ll_a"], d["gumbel_rows"])
            runs[dt] = dict(sc, **{k: ll[k] for k in LL_KEYS})
        for k in worst:
            worst[k] = max(worst[k], _ratio(runs[torch.float32][k], runs[torch.float64][k]))
    return worst


def model_score(DEV, kind, K):
    """KVAE.score against the float64 restatement, and what the call promises about itself."""
    from kvae import noise
    model = small_model(kind, K).to(DEV)
    model.train()
    dyn = model.kalman_filter.dyn_params
    if kind == "switching":
        dyn.tau = 0.37
    before = {k: v.clone() for k, v in model.state_dict().items()}
    d = model_inputs(model, K)
    x, u, mask = d["x"].to(DEV), d["u"].to(DEV), d["mask"].to(DEV)
    B, T = x.shape[:2]
    nz = dict(eps_a=d["eps_a"].to(DEV), gumbel=d["gumbel"].to(DEV))
    model.eval()
    with torch.no_grad(), noise.inject(**nz):
        fwd_before = model(x, u=u, mask=mask)
    model.train()
    out = model.score(x, u=u, mask=mask, decode=True)
    again = model.score(x, u=u, mask=mask, decode=True)
    for k in SCORE_KEYS + ("levels", "a_vae", "x_pred", "n_obs"):
        assert torch.equal(out[k], again[k]), k                          # deterministic: bit-identical
    assert model.training and (kind != "switching" or dyn.tau == 0.37)
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    model.eval()
    with torch.no_grad(), noise.inject(**nz):
        fwd_after = model(x, u=u, mask=mask)
    model.train()
    for k in ("a_samples", "mus_smooth", "Sigmas_smooth", "x_logits", "state_probs"):
        assert torch.equal(fwd_before[k], fwd_after[k]), k
    p = model.a_dim
    assert out["log_lik"].shape == (B, T) and out["log_lik_seq"].shape == (B,) and out["nis"].shape == (B, T)
    assert out["a_pred"].shape == (B, T, p) and out["S"].shape == (B, T, p, p) and out["levels"].shape == (B, T)
    assert out["x_pred"].shape == x.shape and out["a_vae"].shape == (B, T, p)
    assert torch.equal(out["n_obs"].cpu(), torch.full((B,), float(T - 4))) and int(out["levels"].abs().max()) == 0
    assert not bool(out["log_lik"][:, 4:8].any()) and not bool(out["nis"][:, 4:8].any())
    path = None
    if kind == "switching":
        dec = model.decode_regimes(x, smooth=False)
        assert torch.equal(out["regimes"], dec["regimes"]) and torch.equal(out["regimes_logq"], dec["regimes_logq"])
        path = out["regimes"].cpu()
        assert torch.equal(out["state_probs"].cpu(), torch.nn.functional.one_hot(path, K).float())
    else:
        assert "regimes" not in out and torch.equal(model.score(x, u=u, mask=mask, regimes="draw")["log_lik"], out["log_lik"])
    ref, a64 = score_restated(model, d["x"], d["u"], d["mask"], torch.float64, path=path)
    assert _ratio(out["a_vae"], a64) < 1e-5
    figs = {k: _ratio(out[k], ref[k]) for k in SCORE_KEYS}
    print("score", DEV, kind, K, figs)
    for k, v in figs.items():
        assert v < MODEL_TOL[k], (k, v, MODEL_TOL[k])
    check_seq(out["log_lik_seq"], out["log_lik"].detach().cpu().double(), d["mask"])     # log_lik.sum(1) == log_lik_seq
    if kind == "switching":   # one eval-mode draw of the chain instead of the most likely path
        with noise.inject(gumbel=d["gumbel"].to(DEV)):
            drawn = model.score(x, u=u, mask=mask, regimes="draw")
        assert "regimes" not in drawn
        ref_d, _ = score_restated(model, d["x"], d["u"], d["mask"], torch.float64, gumbel=d["gumbel"])
        for k in SCORE_KEYS:
            assert _ratio(drawn[k], ref_d[k]) < MODEL_TOL[k], (k, _ratio(drawn[k], ref_d[k]))
    sampled = None
    with noise.inject(eps_a=d["eps_a"].to(DEV)):
        sampled = model.score(x, sample_a=True)
    assert not torch.equal(sampled["a_vae"], out["a_vae"]) and torch.equal(sampled["n_obs"].cpu(), torch.full((B,), float(T)))
    return figs, path


def model_log_likelihood(DEV, kind, K):
    """KVAE.log_likelihood: its identities, every part against the float64 restatement, the mask, S = 1."""
    from kvae import noise
    model = small_model(kind, K).to(DEV)
    model.train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    d = model_inputs(model, K)
    x, u, mask, S = d["x"].to(DEV), d["u"].to(DEV), d["mask"].to(DEV), d["S"]
    B, T = x.shape[:2]
    figs = {}
    for mk_host in (d["mask"], None):
        mk = None if mk_host is None else mask
        with noise.inject(ll_a=d["ll_a"].to(DEV), gumbel=d["gumbel_rows"].to(DEV)):
            out = model.log_likelihood(x, num_samples=S, u=u, mask=mk)
        ref = log_likelihood_restated(model, d["x"], d["u"], mk_host, S, torch.float64, d["ll_a"], d["gumbel_rows"])
        assert all(out[k].shape == (B, S) for k in ("log_w", "log_px_a", "log_pa", "log_qa", "log_ps_qs"))
        assert all(out[k].shape == (B,) for k in ("log_px", "elbo", "ess", "n_obs"))
        assert torch.equal(out["n_obs"].cpu(), torch.full((B,), float(T - 4 if mk_host is not None else T)))
        parts = out["log_px_a"] + out["log_pa"] - out["log_qa"] + out["log_ps_qs"]
        assert torch.equal(out["log_w"], parts)
        lse = torch.logsumexp(out["log_w"].double(), 1) - math.log(S)
        assert float(((out["log_px"].double() - lse).abs() / lse.abs().clamp_min(1.0)).max()) < 1e-6
        assert bool((out["elbo"] <= out["log_px"] + 1e-6 * out["log_px"].abs().clamp_min(1.0)).all())
        assert bool((out["ess"] >= 1 - 1e-5).all()) and bool((out["ess"] <= S + 1e-5).all())
        if kind == "lstm":
            assert not bool(out["log_ps_qs"].any())
        for k in LL_KEYS:
            v = _ratio(out[k], ref[k])
            figs[k] = max(figs.get(k, 0.0), v)
            assert v < MODEL_TOL[k], (k, v, MODEL_TOL[k], mk_host is not None)
    # the mask removes exactly the hidden frames' terms: both runs above are checked against the restatement, which differ there
    print("log_likelihood", DEV, kind, K, figs)
    with noise.inject(ll_a=d["ll_a"][:, :1].to(DEV), gumbel=d["gumbel_rows"][::S].to(DEV)):
        one = model.log_likelihood(x, num_samples=1, u=u, mask=mask)
    assert torch.equal(one["log_px"], one["log_w"][:, 0]) and torch.equal(one["elbo"], one["log_w"][:, 0])
    assert float((one["ess"] - 1).abs().max()) < 1e-5
    assert model.training and all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    return figs


def model_prediction_scores(DEV, kind="lstm", K=3):
    from kvae.train.prediction import prediction_scores
    model = small_model(kind, K).to(DEV)
    d = model_inputs(model, K)
    x, u, mask = d["x"].to(DEV), d["u"].to(DEV), d["mask"].to(DEV)
    got = prediction_scores(model, {"images": x}, mask=mask, u=u)
    assert all(isinstance(v, float) and math.isfinite(v) for v in got.values()) and len(got) == 4
    sc = model.score(x, u=u, mask=mask)
    a, ap, m = sc["a_vae"].cpu().double(), sc["a_pred"].cpu().double(), d["mask"].double()
    w, cnt = m[:, 1:], m[:, 1:].sum() * a.shape[-1]
    want = {"mse_kf": float((((ap[:, 1:] - a[:, 1:]) ** 2).sum(-1) * w).sum() / cnt),
            "mse_naive": float((((a[:, :-1] - a[:, 1:]) ** 2).sum(-1) * w).sum() / cnt),
            "log_lik_per_step": float(sc["log_lik"].cpu().double().sum() / m.sum()),
            "nis_mean": float(sc["nis"].cpu().double().sum() / m.sum())}
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), (k, got[k], want[k])
    assert got == prediction_scores(model, x, mask=mask, u=u) == prediction_scores(model, (x, None), mask=mask, u=u)


def model_errors(DEV):
    import pytest
    for kind in ("lstm", "switching"):
        model = small_model(kind).to(DEV)
        x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
        for bad in (dict(mask=torch.ones(2, 4)), dict(mask=torch.ones(3, 3)), dict(u=torch.zeros(2, 4, 4)), dict(u=torch.zeros(2, 3, 3)),
                    dict(u=torch.zeros(2, 3))):
            with pytest.raises(ValueError):
                model.score(x, **bad)
            with pytest.raises(ValueError):
                model.log_likelihood(x, **bad)
        with pytest.raises(ValueError, match="regimes"):
            model.score(x, regimes="viterbi")
        for s in (0, -1):
            with pytest.raises(ValueError, match="num_samples"):
                model.log_likelihood(x, num_samples=s)


def calibration(DEV, B=64, T=128):
    """B sequences of T steps drawn in float64 from a K = 1, n = 4 model's own A, B, C, Q, R, mu0, Sigma0 (z_{-1} ~ N(mu0, Sigma0)),
    fed to KalmanFilter.predictive: the mean of nis within 5 standard errors (2 / sqrt(B T)) of p = 2, the mean of ll within 5
    standard errors (the sample's own variance) of the mean of the float64 reference's ll."""
    from kvae.kalman import lgssm_ops
    model = small_model("lstm", 1).to(DEV).eval()
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().double()
    A, Bm, C, Q, R, mu0, S0 = d(dyn.A[0]), d(dyn.B[0]), d(dyn.C[0]), d(kf.Q), d(kf.R), d(kf.mu0), d(kf.Sigma0)
    n, m, p = A.shape[0], Bm.shape[1], C.shape[0]
    g = torch.Generator().manual_seed(123)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    LQ, LR, L0 = torch.linalg.cholesky(Q), torch.linalg.cholesky(R), torch.linalg.cholesky(S0)
    U = 0.3 * r(B, T, m)
    z = mu0 + r(B, n) @ L0.T
    ys = []
    for t in range(T):
        z = z @ A.T + U[:, t] @ Bm.T + r(B, n) @ LQ.T
        ys.append(z @ C.T + r(B, p) @ LR.T)
    Y = torch.stack(ys, 1)
    out = kf.predictive(Y.float().to(DEV), U.float().to(DEV))
    ex = lambda M: M.expand(B, T, *M.shape)
    mp, Sp = filter64(ex(A), ex(Bm), C, ex(Q), R, mu0, S0, Y.float().double(), U.float().double(), torch.ones(B, T, dtype=torch.float64))
    ref = lgssm_ops.predictive_torch(mp, Sp, C, R, Y.float().double())
    nis, ll = out["nis"].cpu().double(), out["ll"].cpu().double()
    items = B * T
    dev_nis = abs(float(nis.mean()) - p) / (2.0 / math.sqrt(items))
    dev_ll = abs(float(ll.mean()) - float(ref["ll"].mean())) / (float(ll.std()) / math.sqrt(items))
    print("calibration", DEV, "nis mean", float(nis.mean()), dev_nis, "s.e.; ll mean", float(ll.mean()), float(ref["ll"].mean()), dev_ll, "s.e.")
    assert int(out["levels"].abs().max()) == 0
    assert dev_nis <= 5 and dev_ll <= 5, (dev_nis, dev_ll)
    assert len(out["filter"]) == 7 and out["state_probs"].shape == (B, T, 1)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "kalman-vae_amd"))
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    print({k: float(f"{v:.3g}") for k, v in yardsticks().items()})
