"""Device-agnostic cases of kvae_lgssm_predictive_bwd / lgssm_ops.PredictiveLogLik / lgssm_ops.log_marginal /
KalmanFilter.log_marginal / compute_loss(kf_objective="marginal"): run against the host simulation (tests/test_predictive_grad.py:
the adjoint bodies of csrc/lgssm_pred.h on emulated wavefronts) and against the gfx950 library (tests/test_gpu_predictive_grad.py).
The reference of the kernel level is FLOAT64 autograd through lgssm_ops.log_marginal_torch on the float32-rounded inputs of
pred_cases.inputs (C a per-item leaf, so that its gradient is per item as the kernel's); the joint-Gaussian case is independent of
it.  The reference of the model level is float64 autograd through a restatement over the model's state_dict (the oracle's filter
on the host, log_marginal_torch) with the same injected draws."""
import ctypes as C
import itertools
import math

import torch

import pred_cases as pc

SHAPES, CMODES = pc.SHAPES, pc.CMODES
GRADS = ("g_mu", "g_Sigma", "gC", "gY")
# Yardsticks, by the rule of pred_cases.YARDSTICK: the largest per-(b,t) ratio |got - ref| / max(1, |ref|)
# (max-norm within the slice, for the error and for the reference) of the FLOAT32 autograd run of log_marginal_torch against its
# float64 run on the same rounded inputs and upstream gradients, over SHAPES x CMODES x {masked, observed}
# (rerun: python tests/pred_grad_cases.py).  Bars = 4 x.
# Largest ratios the kernels reach against the same float64 run, host simulation | gfx950: DESIGN.md section 13.
YARDSTICK = {"g_mu": 1.13e-4, "g_Sigma": 1.26e-4, "gC": 3.87e-4, "gY": 1.36e-4}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
_SLICE = {"g_mu": (-1,), "g_Sigma": (-1, -2), "gC": (-1, -2), "gY": (-1,)}


def upstream(case):
    """Random upstream gradients of ll [B,T] and seq_ll [B]: float64 values that float32 holds exactly."""
    if "g_ll" not in case:
        g = torch.Generator().manual_seed(7 + 1000 * case["B"] + 10 * case["T"] + case["n"])
        case["g_ll"] = torch.randn(case["B"], case["T"], generator=g, dtype=torch.float64).float().double()
        case["g_seq"] = torch.randn(case["B"], generator=g, dtype=torch.float64).float().double()
    return case["g_ll"], case["g_seq"]


def _objective(out, g_ll, g_seq, which):
    obj = 0.0
    if which in ("ll", "both"):
        obj = obj + (out["ll"] * g_ll.to(out["ll"])).sum()
    if which in ("seq", "both"):
        obj = obj + (out["seq_ll"] * g_seq.to(out["ll"])).sum()
    return obj


_REF = {}


def reference(case, masked=True, dtype=torch.float64, which="both"):
    """Autograd through log_marginal_torch in `dtype` on the float32-rounded kernel inputs; C expanded to a per-item leaf.  The
    float64 runs are computed once and shared."""
    from kvae.kalman import lgssm_ops
    key = (id(case), masked, dtype, which)
    if key not in _REF:
        k = case["k"]
        B, T = case["B"], case["T"]
        g_ll, g_seq = upstream(case)
        leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
        mp, Sp, Y = leaf(k["mp"]), leaf(k["Sp"]), leaf(k["Y"])
        Cm = leaf(k["C"].expand(B, T, *k["C"].shape[-2:]).contiguous())
        out = lgssm_ops.log_marginal_torch(mp, Sp, Cm, k["R"].to(dtype), Y, k["mask"].to(dtype) if masked else None)
        _objective(out, g_ll, g_seq, which).backward()
        _REF[key] = case, {"g_mu": mp.grad, "g_Sigma": Sp.grad, "gC": Cm.grad, "gY": Y.grad, "levels": out["levels"],
                          "ll": out["ll"].detach(), "seq_ll": out["seq_ll"].detach()}   # (the case is held: its id stays its own)
    return _REF[key][1]


SENTINEL = -12345.0


def raw(lib, DEV, case, masked=True, which="both", want=GRADS, unaligned=False, pad=4):
    """kvae_lgssm_predictive_bwd through raw pointers.  cmode "packed": C_t is read out of a step record [B,T,pad + p n + 4] at
    float offset `pad` and gC lands in the same slot of a gradient record (everything outside the slot must keep its sentinel);
    "shared": one C, gC a [B,T,p,n] buffer.  unaligned: every operand and output a view offset by one float.  Every output
    starts as NaN: an element nobody writes shows."""
    from kvae import _native as N
    k = {name: t.to(DEV) for name, t in case["k"].items()}
    B, T, n, p = case["B"], case["T"], case["n"], case["p"]
    g_ll, g_seq = (t.float().to(DEV) for t in upstream(case))
    sh = pc.shift if unaligned else (lambda t: t)
    k = {name: sh(t.contiguous()) for name, t in k.items()}
    g_ll, g_seq = sh(g_ll), sh(g_seq)
    pr = N.PredProblem()
    pr.B, pr.T, pr.n, pr.p = B, T, n, p
    pr.mus_pred, pr.Sigmas_pred, pr.R, pr.y = k["mp"].data_ptr(), k["Sp"].data_ptr(), k["R"].data_ptr(), k["Y"].data_ptr()
    pr.mask = k["mask"].data_ptr() if masked else None
    packed = case["cmode"] == "packed"
    rec = grec = None
    if packed:
        E = pad + p * n + 4
        rec = sh(torch.cat([torch.zeros(B, T, pad, device=DEV), k["C"].flatten(2), torch.zeros(B, T, 4, device=DEV)], -1).contiguous())
        pr.C = N.Stack(rec.data_ptr() + 4 * pad, T * E, E)
    else:
        pr.C = N.Stack(k["C"].data_ptr(), 0, 0)
    nan = lambda *s: sh(torch.full(s, float("nan"), device=DEV))
    g = N.PredGrads()
    g.g_ll = g_ll.data_ptr() if which in ("ll", "both") else None
    g.g_seq = g_seq.data_ptr() if which in ("seq", "both") else None
    out = {name: None for name in GRADS}
    if "g_mu" in want:
        out["g_mu"] = nan(B, T, n)
        g.g_mus_pred = out["g_mu"].data_ptr()
    if "g_Sigma" in want:
        out["g_Sigma"] = nan(B, T, n, n)
        g.g_Sigmas_pred = out["g_Sigma"].data_ptr()
    if "gY" in want:
        out["gY"] = nan(B, T, p)
        g.gY = out["gY"].data_ptr()
    if "gC" in want:
        if packed:
            grec = sh(torch.full((B, T, E), SENTINEL, device=DEV))
            g.gC = N.Stack(grec.data_ptr() + 4 * pad, T * E, E)
        else:
            out["gC"] = nan(B, T, p, n)
            g.gC = N.Stack(out["gC"].data_ptr(), T * p * n, p * n)
    rc = lib.dll.kvae_lgssm_predictive_bwd(C.byref(pr), C.byref(g), None)
    assert rc == 0, rc
    if DEV != "cpu":
        torch.cuda.synchronize()
    if grec is not None:
        out["gC"] = grec[..., pad:pad + p * n].unflatten(-1, (p, n)).clone()
        outside = torch.cat([grec[..., :pad], grec[..., pad + p * n:]], -1)
        assert bool((outside == SENTINEL).all()), "gC wrote outside its slot of the record"
    for name in want:
        assert bool(torch.isfinite(out[name]).all()), (name, "an element was not written")
    return out


def ratios(got, ref, items=None):
    """Largest per-(b,t) ratio |got - ref| / max(1, |ref|) of each gradient, max-norm within the slice.  items: a [B,T] bool
    selection."""
    out = {}
    for name in GRADS:
        if got.get(name) is None:
            continue
        d = got[name].detach().cpu().double()
        err, scale = (d - ref[name]).abs().amax(_SLICE[name]), ref[name].abs().amax(_SLICE[name])
        r = err / scale.clamp_min(1.0)
        out[name] = float((r if items is None else r[items]).max())
    return out


def kernel_levels(DEV, case, masked, **kw):
    return pc.run(DEV, case, masked, want=("levels",), **kw)["levels"]


def check(lib, DEV, B, T, n, cmode="shared", masked=True, worst=None, **kw):
    """The four gradients of one call against float64 autograd under TOL, every item; every ladder level 0 in the reference and in
    the kernel; hidden items exactly 0 in every output."""
    case = pc.inputs(B, T, n, cmode)
    got, ref = raw(lib, DEV, case, masked, **kw), reference(case, masked)
    assert int(ref["levels"].abs().max()) == 0 and int(reference(case, masked, torch.float32)["levels"].abs().max()) == 0
    fkw = {a: b for a, b in kw.items() if a in ("unaligned", "pad")}
    assert int(kernel_levels(DEV, case, masked, **fkw).abs().max()) == 0
    figs = ratios(got, ref)
    print("predictive_bwd", DEV, (B, T, n), cmode, "masked" if masked else "observed", kw, figs)
    for name, v in figs.items():
        assert v < TOL[name], (name, v, TOL[name])
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), v)
    if masked:
        hidden = case["mask"] == 0
        for name in GRADS:
            assert not bool(got[name].cpu()[hidden].any()), name          # exact zeros
            assert not bool(ref[name][hidden].any()), name
    return got


def yardsticks():
    """The float32 autograd run of log_marginal_torch against the float64 one: the numbers YARDSTICK holds."""
    worst = {k: 0.0 for k in GRADS}
    for (B, T, n), cmode, masked in itertools.product(SHAPES, CMODES, (True, False)):
        case = pc.inputs(B, T, n, cmode)
        f32, ref = reference(case, masked, torch.float32), reference(case, masked)
        assert int(f32["levels"].abs().max()) == 0 and int(ref["levels"].abs().max()) == 0
        for name, v in ratios(f32, ref).items():
            worst[name] = max(worst[name], v)
    return worst


# ---- upstream variants, subsets of the outputs, repeatability ------------------------------------------------------------------
def upstream_variants(lib, DEV, B, T, n, cmode="packed"):
    """Only g_ll, only g_seq, both: each under TOL against its own float64 run, and (linearity in w) the sum of the two single runs
    within two bars of the run with both."""
    case = pc.inputs(B, T, n, cmode)
    runs = {}
    for which in ("ll", "seq", "both"):
        runs[which] = raw(lib, DEV, case, True, which=which)
        for name, v in ratios(runs[which], reference(case, True, which=which)).items():
            assert v < TOL[name], (which, name, v)
    ref = reference(case, True)
    summed = {name: runs["ll"][name] + runs["seq"][name] for name in GRADS}
    for name, v in ratios(summed, ref).items():
        assert v < 2 * TOL[name], (name, v)


def partial_outputs(lib, DEV, B, T, n, cmode="packed"):
    """Every subset of the four outputs (NULL pointers for the rest) gives the bits of the full call; two full calls are
    bit-identical."""
    case = pc.inputs(B, T, n, cmode)
    full, again = raw(lib, DEV, case), raw(lib, DEV, case)
    for name in GRADS:
        assert torch.equal(full[name], again[name]), name
    for r in range(1, len(GRADS)):
        for want in itertools.combinations(GRADS, r):
            part = raw(lib, DEV, case, want=want)
            for name in GRADS:
                if name in want:
                    assert torch.equal(part[name], full[name]), (want, name)
                else:
                    assert part[name] is None


# ---- the autograd Function -------------------------------------------------------------------------------------------------------
def function_matches_raw(lib, DEV, B, T, n, cmode):
    """lgssm_ops.log_marginal(...) and .backward(): the values are predictive's bits, the gradients the raw call's bits (per-step or
    packed C); a shared [p,n] C gets the sum over the items (against float64 under n_obs x bar); an output nobody differentiates
    costs nothing (seq_ll alone: g_ll is NULL)."""
    from kvae.kalman import lgssm_ops
    case = pc.inputs(B, T, n, cmode)
    k = {name: t.to(DEV) for name, t in case["k"].items()}
    p = case["p"]
    g_ll, g_seq = (t.float().to(DEV) for t in upstream(case))
    leaf = lambda t: t.clone().requires_grad_(True)
    mp, Sp, Y = leaf(k["mp"]), leaf(k["Sp"]), leaf(k["Y"])
    packed, slots = None, lgssm_ops.Slots()
    if cmode == "packed":
        packed = leaf(torch.cat([torch.zeros(B, T, 4, device=DEV), k["C"].flatten(2), torch.zeros(B, T, 4, device=DEV)], -1).contiguous())
        slots = lgssm_ops.Slots(C=4)
        Cm = packed[..., 4:4 + p * n].unflatten(-1, (p, n))
    else:
        Cm = leaf(k["C"])
    out = lgssm_ops.log_marginal(mp, Sp, Cm, k["R"], Y, k["mask"], packed=packed, slots=slots, impl="kernel")
    fwd = pc.run(DEV, case, True, want=("ll", "seq_ll", "levels"))
    for name in ("ll", "seq_ll", "levels"):
        assert torch.equal(out[name], fwd[name]), name
    assert not out["levels"].requires_grad and out["ll"].requires_grad and out["seq_ll"].requires_grad
    _objective(out, g_ll, g_seq, "both").backward()
    ref_raw = raw(lib, DEV, case, True)
    assert torch.equal(mp.grad, ref_raw["g_mu"]) and torch.equal(Sp.grad, ref_raw["g_Sigma"]) and torch.equal(Y.grad, ref_raw["gY"])
    if cmode == "packed":
        assert torch.equal(packed.grad[..., 4:4 + p * n].unflatten(-1, (p, n)), ref_raw["gC"])
        assert not bool(packed.grad[..., :4].any()) and not bool(packed.grad[..., 4 + p * n:].any())
    else:
        ref = reference(case, True)
        n_obs = int(case["mask"].sum())
        want = ref["gC"].sum((0, 1))
        bar = n_obs * TOL["gC"] * max(1.0, float(ref["gC"].abs().amax()))
        assert Cm.grad.shape == (p, n) and float((Cm.grad.cpu().double() - want).abs().max()) <= bar
    # seq_ll alone, Y alone: the other outputs are not computed (need flags), ll's upstream is NULL
    mp2, Y2 = k["mp"].clone(), leaf(k["Y"])
    out2 = lgssm_ops.log_marginal(mp2, k["Sp"], k["C"] if cmode == "shared" else Cm.detach(), k["R"], Y2, k["mask"], impl="kernel")
    out2["seq_ll"].sum().backward()
    only = raw(lib, DEV, dict(case, g_ll=case["g_ll"], g_seq=torch.ones(B, dtype=torch.float64)), True, which="seq", want=("gY",))
    assert torch.equal(Y2.grad, only["gY"])


# ---- the ladder -----------------------------------------------------------------------------------------------------------------
def ladder(lib, DEV, n, b=1, t=3, b5=2, t5=1, B=3, T=6):
    """The construction of pred_cases.ladder: item (b, t) with S_t of eigenvalues (-1e-4, 2e-3) sits at level 3; item (b5, t5) with
    S_t = [[-0.05, 1e-3], [1e-3, 2e-3]] fails levels 0..4 (s_00 + 1e-2 < 0) and takes the clamped diagonal: no gradient reaches
    s_00 (clamped) nor s_01, s_11 >= 1e-6 gets its own.  Both in kernel and float64 reference; gradients under the same bars; the
    neighbours stay at level 0."""
    base = pc.inputs(B, T, n, "packed", mask=torch.ones(B, T))
    case = dict(base, k={name: v.clone() for name, v in base["k"].items()})
    case.pop("g_ll", None), case.pop("g_seq", None)
    R = case["k"]["R"].double()
    g = torch.Generator().manual_seed(7)
    V, _ = torch.linalg.qr(torch.randn(2, 2, generator=g, dtype=torch.float64))
    Cm = case["k"]["C"][b, t].double()
    W = torch.linalg.pinv(Cm) @ V                                        # C W = V
    target = V @ torch.diag(torch.tensor([pc.LADDER_EIG, 2e-3], dtype=torch.float64)) @ V.T - R
    Sp = W @ (V.T @ target @ V) @ W.T
    case["k"]["Sp"][b, t] = (0.5 * (Sp + Sp.T)).float()
    C5 = case["k"]["C"][b5, t5].double()
    W5 = torch.linalg.pinv(C5)                                           # C W5 = I
    S5 = torch.tensor([[-0.05, 1e-3], [1e-3, 2e-3]], dtype=torch.float64)
    Sp5 = W5 @ (S5 - R) @ W5.T
    case["k"]["Sp"][b5, t5] = (0.5 * (Sp5 + Sp5.T)).float()
    ref = reference(case, False)
    lv_ref = ref["levels"]
    assert int(lv_ref[b, t]) == 3 and int(lv_ref[b5, t5]) == 5, (int(lv_ref[b, t]), int(lv_ref[b5, t5]))
    S64 = case["k"]["C"][b5, t5].double() @ case["k"]["Sp"][b5, t5].double() @ case["k"]["C"][b5, t5].double().T + R
    assert float(S64[0, 0]) + 1e-2 < 0 and float(S64[1, 1]) >= 1e-6 and abs(float(S64[0, 1])) > 1e-4   # levels 0..4 fail in float64
    lv = kernel_levels(DEV, case, False).cpu()
    assert int(lv[b, t]) == 3 and int(lv[b5, t5]) == 5, (int(lv[b, t]), int(lv[b5, t5]))
    others = torch.ones(B, T, dtype=torch.bool)
    others[b, t] = others[b5, t5] = False
    assert not bool(lv[others].any()) and not bool(lv_ref[others].any())
    got = raw(lib, DEV, case, False)
    figs = ratios(got, ref)
    print("ladder_bwd", DEV, n, figs)
    for name, v in figs.items():
        assert v < TOL[name], (name, v, TOL[name])
    # the clamp rule read off the kernel's own output: G = W5^T g_Sigma W5 / w (C W5 = I)
    w = float(case["g_ll"][b5, t5] + case["g_seq"][b5])
    for grads in (got, ref):
        G = W5.T @ grads["g_Sigma"][b5, t5].cpu().double() @ W5 / w
        scale = float(G.abs().max())
        assert scale > 1.0 and abs(float(G[0, 0])) <= 1e-4 * scale and abs(float(G[0, 1])) <= 1e-4 * scale, G
        assert abs(float(G[1, 1])) > 0.5 * scale


# ---- independent of the restatement: the gradient of the joint Gaussian of the stacked observed a_t -------------------------
def joint_gaussian_grad(DEV, B, T, n):
    """d/dY of the float64 joint-Gaussian log-density of the stacked observed a_t (the construction of pred_cases.joint_gaussian,
    differentiable) against the chain LgssmSmooth(with_rts=False) -> PredictiveLogLik -> seq_ll.sum().backward() on DEV, under
    the gY bar x T_obs.  First the float64 identity itself: the gradient of the exact decomposition (nothing rounded, no
    jitter) equals the joint gradient to 1e-7 relative."""
    from kvae.kalman import lgssm_ops
    mask = torch.ones(B, T)
    mask[0, 0] = 0
    mask[-1, -1] = 0
    d = pc.inputs(B, T, n, "packed", mask=mask)
    p = d["p"]
    eye = torch.eye(n, dtype=torch.float64)
    Y = d["Y"].clone().requires_grad_(True)
    total = 0.0
    for b in range(B):
        m, P, mz, Pz = d["mu0"], d["S0"], [], []
        for t in range(T):
            m = d["A"][b, t] @ m + d["Bm"][b, t] @ d["U"][b, t]
            P = d["A"][b, t] @ P @ d["A"][b, t].mT + d["Q"][b, t]
            mz.append(m), Pz.append(P)
        obs = [t for t in range(T) if d["mask"][b, t] > 0]
        kk = len(obs)
        mean = torch.cat([d["C"][b, t] @ mz[t] for t in obs])
        cov = torch.zeros(kk * p, kk * p, dtype=torch.float64)
        for (i, s), (j, t) in itertools.product(enumerate(obs), enumerate(obs)):
            if s <= t:
                F = eye
                for q in range(s + 1, t + 1):
                    F = d["A"][b, q] @ F
                blk = d["C"][b, s] @ Pz[s] @ F.mT @ d["C"][b, t].mT + (d["R"] if s == t else 0)
                cov[i * p:(i + 1) * p, j * p:(j + 1) * p] = blk
                cov[j * p:(j + 1) * p, i * p:(i + 1) * p] = blk.mT
        y = torch.cat([Y[b, t] for t in obs])
        total = total + torch.distributions.MultivariateNormal(mean, 0.5 * (cov + cov.mT)).log_prob(y)
    joint, = torch.autograd.grad(total, Y)
    # the exact decomposition in float64, differentiated through the filter
    Y2 = d["Y"].clone().requires_grad_(True)
    mp, Sp = pc.filter64(d["A"], d["Bm"], d["C"], d["Q"], d["R"], d["mu0"], d["S0"], Y2, d["U"], d["mask"])
    S = d["C"] @ Sp @ d["C"].mT + d["R"]
    Lc = torch.linalg.cholesky(0.5 * (S + S.mT))
    w = torch.linalg.solve_triangular(Lc, (Y2 - (d["C"] @ mp.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1), upper=False).squeeze(-1)
    exact = -0.5 * ((w * w).sum(-1) + 2 * Lc.diagonal(dim1=-2, dim2=-1).log().sum(-1) + p * math.log(2 * math.pi)) * d["mask"]
    dec, = torch.autograd.grad(exact.sum(), Y2)
    assert float((dec - joint).abs().max()) <= 1e-7 * float(joint.abs().max()), (dec, joint)
    assert not bool(joint[d["mask"] == 0].any())
    # the product's chain on DEV
    f = lambda t: t.float().to(DEV)
    Yk = f(d["Y"]).requires_grad_(True)
    mk = f(d["mask"])
    mf, Sf, mpk, Spk = lgssm_ops.LgssmSmooth.apply(Yk, f(d["U"]), mk, None, f(d["A"]), f(d["Bm"]), f(d["C"]), f(d["Q"]), f(d["R"]),
                                                  f(d["mu0"]), f(d["S0"]), lgssm_ops.Slots(), False)
    out = lgssm_ops.log_marginal(mpk, Spk, f(d["C"]), f(d["R"]), Yk, mk, impl="kernel")
    out["seq_ll"].sum().backward()
    got = Yk.grad.cpu().double()
    for b in range(B):
        t_obs = int(d["mask"][b].sum())
        bar = t_obs * TOL["gY"] * max(1.0, float(joint[b].abs().max()))
        err = float((got[b] - joint[b]).abs().max())
        print("joint_grad", DEV, (B, T, n, b), err, bar)
        assert err <= bar, (b, err, bar)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """The error codes of include/kvae_lgssm.h through raw pointers."""
    from kvae import _native as N
    buf = torch.zeros(4096, device=DEV)
    ptr = buf.data_ptr()

    def prob(**kw):
        pr = N.PredProblem()
        pr.B, pr.T, pr.n, pr.p = 2, 3, 4, 2
        for k in ("mus_pred", "Sigmas_pred", "R", "y", "mask"):
            setattr(pr, k, ptr)
        pr.seq_ll = ptr                                                       # the forward's outputs are ignored: seq_ll without ll
        pr.C = N.Stack(ptr, 0, 0)
        for k, v in kw.items():
            setattr(pr, k, v)
        return pr

    def grads(**kw):
        g = N.PredGrads()
        g.g_ll, g.g_seq = ptr, ptr
        g.g_mus_pred, g.g_Sigmas_pred, g.gY = ptr + 1024, ptr + 2048, ptr + 4096
        g.gC = N.Stack(ptr + 8192, 24, 8)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    call = lambda pr, g: lib.dll.kvae_lgssm_predictive_bwd(C.byref(pr), C.byref(g) if g is not None else None, None)
    assert call(prob(), grads()) == 0
    for kw in (dict(B=0), dict(T=0), dict(B=-1), dict(n=0), dict(n=17), dict(p=0), dict(p=17), dict(p=3)):
        assert call(prob(**kw), grads()) == 1, kw                                # KVAE_ERR_DIMS
    for kw in (dict(mus_pred=None), dict(Sigmas_pred=None), dict(R=None), dict(y=None), dict(C=N.Stack(None, 0, 0))):
        assert call(prob(**kw), grads()) == 2, kw                                # KVAE_ERR_NULL
    assert lib.dll.kvae_lgssm_predictive_bwd(None, C.byref(grads()), None) == 2 and call(prob(), None) == 2
    assert call(prob(), grads(g_ll=None, g_seq=None)) == 2                       # both upstreams NULL
    for kw in (dict(C=N.Stack(ptr, -1, 0)), dict(C=N.Stack(ptr, 0, -8))):
        assert call(prob(**kw), grads()) == 4, kw                                # KVAE_ERR_ARG
    for st in (N.Stack(ptr + 8192, -24, 8), N.Stack(ptr + 8192, 24, -8)):
        assert call(prob(), grads(gC=st)) == 4                                   # negative gC strides
    assert call(prob(mask=None), grads(g_ll=None)) == 0 and call(prob(), grads(g_seq=None)) == 0
    assert call(prob(), grads(g_mus_pred=None, g_Sigmas_pred=None, gY=None, gC=N.Stack(None, 0, 0))) == 0   # nothing asked: no launch
    if DEV != "cpu":
        torch.cuda.synchronize()


def unsupported_takes_torch(DEV):
    """a_dim 3 and float64 tensors are outside the kernel: log_marginal takes log_marginal_torch (differentiable); forcing the
    kernel raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    case = pc.inputs(2, 5, 4, "shared", p=3)
    k = {name: t.to(DEV) for name, t in case["k"].items()}
    Y = k["Y"].clone().requires_grad_(True)
    out = lgssm_ops.log_marginal(k["mp"], k["Sp"], k["C"], k["R"], Y, k["mask"])
    out["seq_ll"].sum().backward()
    upstream(case)
    want = reference(dict(case, g_seq=torch.ones(2, dtype=torch.float64)), True, which="seq")
    assert float((Y.grad.cpu().double() - want["gY"]).abs().max() / want["gY"].abs().max()) < 1e-3
    with pytest.raises(RuntimeError):
        lgssm_ops.log_marginal(k["mp"], k["Sp"], k["C"], k["R"], k["Y"], k["mask"], impl="kernel")
    d = pc.inputs(2, 5, 4, "shared")
    k64 = {name: t.double().to(DEV) for name, t in d["k"].items()}
    Y64 = k64["Y"].clone().requires_grad_(True)
    out = lgssm_ops.log_marginal(k64["mp"], k64["Sp"], k64["C"], k64["R"], Y64, k64["mask"])
    assert out["ll"].dtype == torch.float64 and float((out["ll"].detach().cpu() - pc.reference(d)["ll"]).abs().max()) < 1e-9
    out["seq_ll"].sum().backward()
    want = reference(dict(d, g_ll=torch.zeros(2, 5, dtype=torch.float64), g_seq=torch.ones(2, dtype=torch.float64)), True, which="seq")
    assert float((Y64.grad.cpu() - want["gY"]).abs().max()) < 1e-9 * max(1.0, float(want["gY"].abs().max()))


def torch_values_are_predictive_torch():
    """log_marginal_torch gives predictive_torch's values exactly, at every level of the ladder, and finite gradients."""
    from kvae.kalman import lgssm_ops
    for n in (4, 16, 5):
        base = pc.inputs(3, 6, n, "packed", mask=torch.ones(3, 6))
        k = {name: v.clone().double() for name, v in base["k"].items()}
        C5 = k["C"][2, 1]
        W5 = torch.linalg.pinv(C5)
        Sp5 = W5 @ (torch.tensor([[-0.05, 1e-3], [1e-3, 2e-3]], dtype=torch.float64) - k["R"]) @ W5.T
        k["Sp"][2, 1] = 0.5 * (Sp5 + Sp5.T)
        k["Sp"][0, 2] = -k["Sp"][0, 2]
        Sp = k["Sp"].clone().requires_grad_(True)
        a = lgssm_ops.log_marginal_torch(k["mp"], Sp, k["C"], k["R"], k["Y"])
        b = lgssm_ops.predictive_torch(k["mp"], k["Sp"], k["C"], k["R"], k["Y"])
        assert torch.equal(a["ll"].detach(), b["ll"]) and torch.equal(a["levels"], b["levels"]) and int(a["levels"].max()) == 5
        a["seq_ll"].sum().backward()
        assert bool(torch.isfinite(Sp.grad).all())


# ---------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------
MODELS = [("lstm", 3), ("switching", 3)]
# Yardsticks of the model level: the float32 run of the restatement below (plain torch on the host, autograd) against its float64
# run, same injected Gumbel draws, per entry the largest |f32 - f64| / max(1, max|f64|) (max-norm over the tensor) over MODELS
# (rerun: the CPU tier's test_model_yardsticks prints them).  Bars = 4 x.  What the product reaches: DESIGN.md section 13.
MODEL_YARDSTICK = {"a": 3.12e-7, "params": 1.86e-5, "seq_ll": 1.94e-7}
MODEL_TOL = {k: 4.0 * v for k, v in MODEL_YARDSTICK.items()}


def marginal_restated(model, a, u, mask, dtype, gumbel):
    """seq_ll.sum() (+ the regime chain's log_p - log_q where the caller wants it) of KalmanFilter.log_marginal in TRAINING mode over
    the model's state_dict in `dtype`, plain torch on the host: the oracle's filter, log_marginal_torch; autograd gives the
    gradient w.r.t. a and every LGSSM / dynamics parameter.  Returns (seq_ll, extra, a leaf, {name: parameter leaf})."""
    from kvae.kalman import lgssm_ops
    from oracle import torch_oracle as O
    sd = pc._state(model, dtype)
    names = [k for k, v in model.named_parameters() if k.startswith("kalman_filter.")]
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    kind = model.config.dynamics_model.lower()
    dyn = O.split_dyn(sd)
    Qb, R, mu0, S0 = pc._kf(sd)
    a = a.detach().cpu().to(dtype).clone().requires_grad_(True)
    u, mk = u.cpu().to(dtype), mask.cpu().to(dtype)
    dynp = model.kalman_filter.dyn_params
    out = O.lgssm_filter(a, u, mk, dyn, kind, Qb, R, mu0, S0, tau=float(getattr(dynp, "tau", 1.0)), is_training=True,
                         gumbel=None if gumbel is None else gumbel.cpu().to(dtype),
                         trans_matrix=dynp.prior.transition_matrix.detach().cpu().to(dtype) if kind == "switching" else None)
    pred = lgssm_ops.log_marginal_torch(out["mus_pred"].squeeze(-1), out["Sigmas_pred"], out["C_list"], R, a, mk)
    extra = (out["log_pseq"].sum() - out["log_qseq"].sum()) if kind == "switching" else None
    return pred, extra, a, {k: sd[k] for k in names}


def _tensor_ratio(got, ref):
    ref = ref.detach().double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1.0))


def _restated_grads(model, a, u, mask, dtype, gumbel):
    pred, _, leaf, params = marginal_restated(model, a, u, mask, dtype, gumbel)
    pred["seq_ll"].sum().backward()
    return pred, leaf.grad, {k: v.grad for k, v in params.items()}


def _model_case(DEV, kind, K):
    model = pc.small_model(kind, K).to(DEV)
    model.train()
    d = pc.model_inputs(model, K)
    g = torch.Generator().manual_seed(31 + K)
    a = torch.randn(2, 10, model.a_dim, generator=g)
    return model, d, a


def model_yardsticks():
    worst = {k: 0.0 for k in MODEL_YARDSTICK}
    for kind, K in MODELS:
        model, d, a = _model_case("cpu", kind, K)
        runs = {dt: _restated_grads(model, a, d["u"], d["mask"], dt, d["gumbel"]) for dt in (torch.float32, torch.float64)}
        (p32, a32, g32), (p64, a64, g64) = runs[torch.float32], runs[torch.float64]
        worst["seq_ll"] = max(worst["seq_ll"], _tensor_ratio(p32["seq_ll"], p64["seq_ll"]))
        worst["a"] = max(worst["a"], _tensor_ratio(a32, a64))
        for k in g64:
            if g64[k] is not None:
                worst["params"] = max(worst["params"], _tensor_ratio(g32[k], g64[k]))
    return worst


def model_log_marginal(DEV, kind, K):
    """KalmanFilter.log_marginal(...)["seq_ll"].sum().backward() in training mode: the gradient w.r.t. a and every LGSSM / dynamics
    parameter against float64 autograd of the restatement, the same Gumbel draws."""
    from kvae import noise
    model, d, a = _model_case(DEV, kind, K)
    kf = model.kalman_filter
    u, mask = d["u"].to(DEV), d["mask"].to(DEV)
    ak = a.to(DEV).requires_grad_(True)
    kf.dyn_params.reset_state()
    with noise.inject(gumbel=d["gumbel"].to(DEV)):
        out = kf.log_marginal(ak, u, mask)
    assert out["ll"].shape == (2, 10) and out["seq_ll"].shape == (2,) and out["levels"].shape == (2, 10) and len(out["filter"]) == 7
    assert int(out["levels"].abs().max()) == 0 and not bool(out["ll"][:, 4:8].any()) and out["state_probs"].shape == (2, 10, K)
    model.zero_grad()
    out["seq_ll"].sum().backward()
    pred, ga, gp = _restated_grads(model, a, d["u"], d["mask"], torch.float64, d["gumbel"])
    figs = {"seq_ll": _tensor_ratio(out["seq_ll"], pred["seq_ll"]), "a": _tensor_ratio(ak.grad, ga), "params": 0.0}
    got = dict(model.named_parameters())
    for k, ref in gp.items():
        if ref is None:
            continue
        assert got[k].grad is not None, k
        figs["params"] = max(figs["params"], _tensor_ratio(got[k].grad, ref))
    print("log_marginal", DEV, kind, K, figs)
    for k, v in figs.items():
        assert v < MODEL_TOL[k], (k, v, MODEL_TOL[k])
    return figs


def model_compute_loss(DEV, kind, K):
    """compute_loss(kf_objective="marginal"): elbo_kf is the formula over score-style outputs; loss.backward() gives finite
    gradients to every trainable parameter; training-mode forward returns no smoothed stacks, eval mode does; "elbo" and the
    default are bit-identical under injected noise."""
    from kvae import noise
    model = pc.small_model(kind, K).to(DEV)
    model.train()
    d = pc.model_inputs(model, K)
    x, u, mask = d["x"].to(DEV), d["u"].to(DEV), d["mask"].to(DEV)
    B, T = x.shape[:2]
    g = torch.Generator().manual_seed(3)
    eps_z = torch.randn(B, T, model.z_dim, generator=g)
    nz = lambda: dict(eps_a=d["eps_a"].to(DEV), gumbel=d["gumbel"].to(DEV), eps_z=eps_z.to(DEV))
    assert type(model).kf_objective == "elbo"

    def step(objective, via):
        model.zero_grad()
        model.kalman_filter.dyn_params.reset_state()
        saved = model.kf_objective
        if via == "attr":
            model.kf_objective = objective
        try:
            with noise.inject(**nz()):
                out = model(x, u=u, mask=mask)
                kw = {} if via != "arg" else dict(kf_objective=objective)
                losses = model.compute_loss(x, out, mask=mask, with_metrics=False, **kw)
        finally:
            model.kf_objective = saved
        losses["loss"].backward()
        return out, losses, {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}

    out_d, l_d, g_d = step(None, "default")
    out_e, l_e, g_e = step("elbo", "arg")
    assert torch.equal(l_d["loss"], l_e["loss"]) and torch.equal(l_d["elbo_kf"], l_e["elbo_kf"])
    for k in g_d:
        assert (g_d[k] is None and g_e[k] is None) or torch.equal(g_d[k], g_e[k]), k
    assert out_d["mus_smooth"] is not None and out_d["Sigmas_smooth"] is not None
    out_m, l_m, g_m = step("marginal", "attr")
    assert out_m["mus_smooth"] is None and out_m["Sigmas_smooth"] is None and out_m["mus_pred"] is not None
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert g_m[k] is not None and bool(torch.isfinite(g_m[k]).all()), k
    # the formula, from score-style outputs of the same filter pass
    from kvae.kalman import lgssm_ops
    with torch.no_grad():
        pred = lgssm_ops.predictive(out_m["mus_pred"], out_m["Sigmas_pred"], out_m["ABC"][2], model.kalman_filter.R,
                                    out_m["a_samples"], mask, want=("seq_ll",))
        total = pred["seq_ll"].double().sum()
        if kind == "switching":
            log_q, log_p = model.kalman_filter.dyn_params.elbo_terms()
            total = total + log_p.double().sum() - log_q.double().sum()
        want = total / mask.sum().double()
    assert abs(float(l_m["elbo_kf"]) - float(want)) <= 1e-5 * max(1.0, abs(float(want))), (float(l_m["elbo_kf"]), float(want))
    assert float(l_m["elbo_kf"]) != float(l_d["elbo_kf"])
    model.eval()
    with torch.no_grad(), noise.inject(**nz()):
        model.kf_objective = "marginal"
        try:
            ev = model(x, u=u, mask=mask)
        finally:
            del model.kf_objective
    assert ev["mus_smooth"] is not None and ev["mus_smooth"].shape[:2] == (B, T) and ev["Sigmas_smooth"] is not None
    model.train()


def model_errors(DEV):
    import pytest
    model = pc.small_model("lstm", 3).to(DEV)
    model.train()
    d = pc.model_inputs(model, 3)
    x = d["x"].to(DEV)
    out = model(x)
    with pytest.raises(ValueError, match="kf_objective"):
        model.compute_loss(x, out, kf_objective="exact", with_metrics=False)
    model.kf_objective = "joint"
    try:
        with pytest.raises(ValueError, match="kf_objective"):
            model(x)
    finally:
        del model.kf_objective
    from kvae.train.train import Trainer
    with pytest.raises(ValueError, match="kf_objective"):
        Trainer(model, use_graph=False, kf_objective="likelihood")


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "kalman-vae_amd"))
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    print({k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print({k: float(f"{v:.3g}") for k, v in model_yardsticks().items()})
