"""Device-agnostic parity cases: run against the host simulation (CPU tier) and the gfx950 library (GPU tier)."""
import math

import torch

from golden_util import rel_err

def _random_problem(B, T, n, m, p, K, seed, device):
    g = torch.Generator().manual_seed(seed)
    A = torch.eye(n).repeat(K, 1, 1) + 0.08 * torch.randn(K, n, n, generator=g)
    Bm = 0.1 * torch.randn(K, n, m, generator=g)
    Cm = 0.3 * torch.randn(K, p, n, generator=g)
    alpha = torch.softmax(torch.randn(B, T, K, generator=g), -1)
    Y = torch.randn(B, T, p, generator=g)
    U = 0.3 * torch.randn(B, T, m, generator=g)
    mask = (torch.rand(B, T, generator=g) > 0.2).float()
    eps = torch.randn(B, T, n, generator=g)
    return [t.to(device) for t in (A, Bm, Cm, alpha, Y, U, mask, eps)]


def vs_oracle_random(DEV, B, T, n, m, p, K, dense_q=False):
    """HIP path vs the CPU oracle (C restatement for values, torch oracle autograd for gradients) on seeded
    inputs, incl. BASELINE configs[1] (B=256,T=50,n=4) and a configs[4] shard slice (n=16,T=200); ragged
    sizes, masks, controls, T=1 and run-time dimensions.  dense_q: a full SPD process noise shared by the batch (the default
    0.02 I cannot tell a factor from its transpose - the n = 16 ELBO keeps chol(Q)^-1 AND its transpose on the lanes)."""
    from kvae.kalman.lgssm_ops import LgssmElbo, LgssmSmooth, mix_dynamics
    from oracle import c_oracle
    from oracle import torch_oracle as O
    A, Bm, Cm, alpha, Y, U, mask, eps = _random_problem(B, T, n, m, p, K, 100 + B + T, DEV)
    R = 0.03 * torch.eye(p, device=DEV)
    Q = 0.02 * torch.eye(n, device=DEV)
    if dense_q:
        Wq = torch.randn(n, n, generator=torch.Generator().manual_seed(7)).to(DEV)
        Q = Q + 0.004 * (Wq @ Wq.T)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    leaves = [t.clone().requires_grad_(True) for t in (A, Bm, Cm, alpha, Y, U)]
    rec, offs, (As, Bs, Cs) = mix_dynamics(leaves[3], leaves[:3])
    from kvae.kalman.lgssm_ops import Slots
    slots = Slots(A=offs[0], B=offs[1], C=offs[2])
    ms, Ss, mf, Sf, mp, Sp = LgssmSmooth.apply(leaves[4], leaves[5], mask, rec, None, None, None, Q, R, mu0, S0, slots, True)
    total, terms, levels_dev = LgssmElbo.apply(ms, Ss, eps, leaves[4], leaves[5], mask, rec, None, None, None, Q, R, mu0, S0, slots)
    # values: C oracle
    c = lambda t: t.detach().cpu()
    ref = c_oracle.smooth(c(Y), c(U), c(mask), c(As), c(Bs), c(Cs), c(Q), c(R), c(mu0), c(S0))
    # n = 16: two float32 implementations of a 200-step recursion with different summation orders (matrix cores vs scalar
    # loops) can sit 1e-3 apart while both are equally close to the truth; this first bar only catches gross errors there, the
    # real one follows below - against a FLOAT64 run, within max(1e-4, 2 x the float32 oracle's own distance from it).
    tol = 2e-4 if n < 16 else 2e-3
    for k, v in (("mus_smooth", ms), ("Sigmas_smooth", Ss), ("mus_filt", mf), ("Sigmas_filt", Sf), ("mus_pred", mp),
                 ("Sigmas_pred", Sp)):
        assert rel_err(c(v), ref[k]) < tol, k
    rterms, levels = c_oracle.elbo_terms(c(ms), c(Ss), c(eps), c(Y), c(U), c(mask), c(As), c(Bs), c(Cs), c(Q), c(R),
                                         c(mu0), c(S0))
    assert list(levels) == [0, 0]
    for i in range(4):
        assert abs(float(terms[i]) - rterms[i]) <= 2e-4 * abs(rterms[i]) + 1e-3, (i, float(terms[i]), rterms[i])
    if B * T * n * n > 450000:
        return  # gradients up to configs[1] size (256,50,4) and (8,200,16); beyond, the torch-oracle tape takes minutes
    # gradients: autograd over the torch oracle
    (total / (B * T)).backward()
    v32 = {}
    want = _torch_oracle_grads((A, Bm, Cm, alpha, Y, U, mask, eps), Q, R, mu0, S0, torch.float32, values=v32)
    for name, got, ref_g in zip("A B C alpha Y U".split(), leaves, want):
        assert rel_err(got.grad.cpu(), ref_g) < 3e-3, name
    if n >= 16:   # the value bar where float32 is the limit (see above)
        v64 = {}
        _torch_oracle_grads((A, Bm, Cm, alpha, Y, U, mask, eps), Q, R, mu0, S0, torch.float64, values=v64)
        for k, got in (("mus_smooth", ms), ("Sigmas_smooth", Ss), ("elbo_sum", total)):
            tape, mine = rel_err(v32[k].double(), v64[k]), rel_err(c(got).double(), v64[k])
            assert mine < max(1e-4, 4.0 * tape), (k, mine, tape)   # (4: see values_vs_fp64_oracle)


def _torch_oracle_grads(problem, Q, R, mu0, S0, dtype, values=None):
    """d(ELBO / (B T)) / d(A, B, C, alpha, Y, U) by autograd over oracle/torch_oracle.py, computed in `dtype` on the CPU.
    values: a dict that receives the forward results (mus_smooth [B,T,n], Sigmas_smooth, elbo_sum)."""
    from oracle import torch_oracle as O
    c = lambda t: t.detach().cpu().to(dtype)
    A, Bm, Cm, alpha, Y, U, mask, eps = problem
    B, T = Y.shape[:2]
    cl = [c(t).clone().requires_grad_(True) for t in (A, Bm, Cm, alpha, Y, U)]
    Ar = torch.einsum("btk,kij->btij", cl[3], cl[0])
    Br = torch.einsum("btk,kij->btij", cl[3], cl[1])
    Cr = torch.einsum("btk,kij->btij", cl[3], cl[2])
    mu, Sig = c(mu0).expand(B, -1).unsqueeze(-1), c(S0).expand(B, -1, -1)
    mfs, Sfs, mps, Sps = [], [], [], []
    for t in range(T):
        mu, Sig, mu_p, Sig_p = O.filter_step(mu, Sig, cl[4][:, t], cl[5][:, t], Ar[:, t], Br[:, t], Cr[:, t], c(Q), c(R),
                                             c(mask)[:, t])
        mfs.append(mu), Sfs.append(Sig), mps.append(mu_p), Sps.append(Sig_p)
    mus, Sigs = [mfs[-1]], [Sfs[-1]]
    for t in range(T - 2, -1, -1):
        m_s, S_s = O.smooth_step(Sfs[t], Sps[t + 1], Sigs[0], mfs[t], mps[t + 1], mus[0], Ar[:, t + 1])
        mus.insert(0, m_s), Sigs.insert(0, S_s)
    tr, em, ini, ent = O.lgssm_elbo_terms(torch.stack(mus, 1), torch.stack(Sigs, 1), cl[4], cl[5], Ar, Br, Cr, c(Q), c(R),
                                          c(mu0), c(S0), c(mask), c(eps))
    if values is not None:
        values.update(mus_smooth=torch.stack(mus, 1).detach().squeeze(-1), Sigmas_smooth=torch.stack(Sigs, 1).detach(),
                      elbo_sum=(tr + em + ini + ent).detach())
    ((tr + em + ini + ent) / (B * T)).backward()
    return [t.grad for t in cl]


def values_vs_fp64_oracle(DEV, B, T, n, K):
    """north_star asks for ELBO and smoothed means within 1e-4 of the reference's CPU path.  At n = 16 over T = 200 float32 itself
    cannot promise that (the reference's own float32 run of stress_switch_z16_B2_T200 is 3.4e-4 from a float64 run of the same
    recursion), so here the float64 oracle is the truth and the bar is written as an assertion instead of a flat 2e-3: the HIP
    smoothed means, smoothed covariances and ELBO must lie within max(1e-4, 4 x the float32 oracle's own distance) of it.
    (Four, not two: that distance is ONE sample of amplified rounding - the same oracle lands at 0.8e-4 on one host CPU and at
    3.4e-4 on another for the same fixture - so the factor has to cover the spread between summation orders.)"""
    from kvae.kalman.lgssm_ops import LgssmElbo, LgssmSmooth, Slots, mix_dynamics
    problem = _random_problem(B, T, n, n, 2, K, 100 + B + T, DEV)
    A, Bm, Cm, alpha, Y, U, mask, eps = problem
    R, Q = 0.03 * torch.eye(2, device=DEV), 0.02 * torch.eye(n, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    with torch.no_grad():
        rec, offs, _ = mix_dynamics(alpha, [A, Bm, Cm])
        slots = Slots(A=offs[0], B=offs[1], C=offs[2])
        ms, Ss, *_ = LgssmSmooth.apply(Y, U, mask, rec, None, None, None, Q, R, mu0, S0, slots, True)
        total, _, _ = LgssmElbo.apply(ms, Ss, eps, Y, U, mask, rec, None, None, None, Q, R, mu0, S0, slots)
    v64, v32 = {}, {}
    _torch_oracle_grads(problem, Q, R, mu0, S0, torch.float64, values=v64)
    _torch_oracle_grads(problem, Q, R, mu0, S0, torch.float32, values=v32)
    report = {}
    for k, got in (("mus_smooth", ms), ("Sigmas_smooth", Ss), ("elbo_sum", total)):
        tape = rel_err(v32[k].double(), v64[k])
        mine = rel_err(got.cpu().double(), v64[k])
        report[k] = (mine, tape)
        assert mine < max(1e-4, 4.0 * tape), (k, mine, tape)
    return report


_FP64_CACHE = {}


def latent_fp64_budget(g, kind, name):
    """Float64 and float32 runs of the torch oracle on a latent golden's inputs: (outputs of the float64 run, per-key distance of
    the float32 run from it).  The fixture itself is a float32 run of the REFERENCE, so it sits at the same distance."""
    if name in _FP64_CACHE:
        return _FP64_CACHE[name]
    from golden_util import sub
    from oracle import torch_oracle as O

    def run(dt):
        c = lambda t: t.to(dt) if t.is_floating_point() else t
        dyn = {k: c(v) for k, v in sub(g, "dyn.").items()}
        kw = {}
        if kind == "switching":
            kw = dict(tau=float(g["tau"]), is_training=bool(g["train"]), gumbel=c(g["gumbel"]), trans_matrix=c(g["trans_matrix"]))
        with torch.no_grad():
            return O.smooth_and_elbo(dyn, kind, c(g["a"]), c(g["u"]), c(g["mask"]), c(g["Qbuf"]), c(g["R"]), c(g["mu0"]),
                                     c(g["Sigma0"]), c(g["eps_z"]), **kw)

    o64, o32 = run(torch.float64), run(torch.float32)
    dist = {k: rel_err(o32[k].double(), o64[k]) for k in o64 if torch.is_tensor(o64[k]) and o64[k].is_floating_point()}
    # the REFERENCE's own float32 run is the fixture: its distance from float64 is data, the same on every box (the oracle's
    # float32 run depends on the host's BLAS: 0.8e-4 on one CPU, 3.4e-4 on another for the same inputs) - the budget is the
    # larger of the two
    for k in list(dist):
        if k in g and g[k].shape == o64[k].shape:
            dist[k] = max(dist[k], rel_err(g[k].double(), o64[k]))
        elif k + "_every8" in g:
            dist[k] = max(dist[k], rel_err(g[k + "_every8"].double(), o64[k][:, ::8]))
    _FP64_CACHE[name] = (o64, dist)
    return o64, dist


def grads_vs_fp64_oracle(DEV, B, T, n, K):
    """Where float32 itself is the limit.  A SINGLE dynamics mode at n = 16 (every step multiplies by the same A, prior 20 I against
    R = 0.03 I) leaves the float32 torch oracle 0.8-1.3e-2 away from its own float64 run on the gradients of B and U, so the 3e-3
    bar of vs_oracle_random against the float32 tape would measure the tape.  Here the float64 oracle is the truth and the HIP path
    must stay within the larger of that bar and four times the float32 oracle's own distance from it."""
    from kvae.kalman.lgssm_ops import LgssmElbo, LgssmSmooth, Slots, mix_dynamics
    problem = _random_problem(B, T, n, n, 2, K, 100 + B + T, DEV)
    A, Bm, Cm, alpha, Y, U, mask, eps = problem
    R, Q = 0.03 * torch.eye(2, device=DEV), 0.02 * torch.eye(n, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    leaves = [t.clone().requires_grad_(True) for t in (A, Bm, Cm, alpha, Y, U)]
    rec, offs, _ = mix_dynamics(leaves[3], leaves[:3])
    slots = Slots(A=offs[0], B=offs[1], C=offs[2])
    ms, Ss, *_ = LgssmSmooth.apply(leaves[4], leaves[5], mask, rec, None, None, None, Q, R, mu0, S0, slots, True)
    total, _, levels_dev = LgssmElbo.apply(ms, Ss, eps, leaves[4], leaves[5], mask, rec, None, None, None, Q, R, mu0, S0, slots)
    (total / (B * T)).backward()
    g64 = _torch_oracle_grads(problem, Q, R, mu0, S0, torch.float64)
    g32 = _torch_oracle_grads(problem, Q, R, mu0, S0, torch.float32)
    worst = 0.0
    for name, got, w64, w32 in zip("A B C alpha Y U".split(), leaves, g64, g32):
        if float(w64.abs().max()) == 0.0:  # K = 1: softmax over one mode is constant
            assert float(got.grad.abs().max()) < 1e-6, name
            continue
        tape = rel_err(w32.double(), w64)
        mine = rel_err(got.grad.cpu().double(), w64)
        worst = max(worst, tape)
        assert mine < max(3e-3, 4.0 * tape), (name, mine, tape)
    return worst


def unaligned_fallback(DEV, n, m, p, B=3, T=9):
    """Operands that do NOT start on 16-byte boundaries take the run-time-dimension kernels instead of the specialised
    ones ((16,16,2): matrix cores; (4,4,2): sixteen sequences per wavefront - both move rows with 16-byte accesses):
    same values and same gradients either way.  B = 19 at n = 4 also leaves the last wavefront's quads ragged."""
    from kvae.kalman.lgssm_ops import LgssmSmooth, Slots
    A, Bm, Cm, alpha, Y, U, mask, _ = _random_problem(B, T, n, m, p, 1, 21, DEV)
    R, Q = 0.03 * torch.eye(p, device=DEV), 0.02 * torch.eye(n, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    Astack = A[0].expand(B, T, n, n).contiguous()
    odd = torch.empty(B * T * n * n + 1, device=DEV)[1:].view(B, T, n, n)   # same values, 4 bytes off a 16-byte boundary
    odd.copy_(Astack)
    assert odd.data_ptr() % 16 != 0 and Astack.data_ptr() % 16 == 0
    res = []
    for stack in (Astack, odd):
        leaf = stack.clone().requires_grad_(True) if stack is Astack else None
        if leaf is None:                      # .clone() would re-align it: take the gradient w.r.t. a view's base instead
            base = torch.empty(B * T * n * n + 1, device=DEV)
            base[1:].copy_(stack.reshape(-1))
            base.requires_grad_(True)
            leaf_in = base[1:].view(B, T, n, n)
            assert leaf_in.data_ptr() % 16 != 0
        else:
            base, leaf_in = leaf, leaf
        outs = LgssmSmooth.apply(Y, U, mask, None, leaf_in, Bm[0], Cm[0], Q, R, mu0, S0, Slots(), True)
        gen = torch.Generator().manual_seed(5)
        loss = sum((o * torch.randn(o.shape, generator=gen).to(DEV)).sum() for o in outs)
        loss.backward()
        gA = base.grad if base is leaf else base.grad[1:].view(B, T, n, n)
        res.append(([o.detach().cpu() for o in outs], gA.cpu()))
    (fast, gfast), (slow, gslow) = res
    for a, b in zip(fast, slow):
        assert rel_err(a, b) < 2e-4
    assert rel_err(gfast, gslow) < 5e-4


def n16_generic_fallback(DEV):
    unaligned_fallback(DEV, 16, 16, 2)


def n4_generic_fallback(DEV):
    unaligned_fallback(DEV, 4, 4, 2, B=19, T=11)


def n16_indefinite_q(DEV, B=3, T=12):
    """(16,16,2) with a process noise that is NOT positive semi-definite (the reference's stability recipe does this at
    n = 4): predicted covariances go indefinite, the natural-order elimination of the smoother gain meets a non-positive
    pivot and the kernels must fall back to the partially pivoted one (getrf's pivot sequence, which is what the C
    oracle's LU and torch.linalg.solve do).  Values vs the C oracle, gradients vs the torch oracle."""
    from kvae.kalman.lgssm_ops import LgssmSmooth, Slots
    from oracle import c_oracle
    from oracle import torch_oracle as O
    n, m, p = 16, 16, 2
    g = torch.Generator().manual_seed(77)
    A = 0.6 * torch.eye(n) + 0.15 * torch.randn(n, n, generator=g)
    Bm = 0.1 * torch.randn(n, m, generator=g)
    Cm = 0.3 * torch.randn(p, n, generator=g)
    Qh = 0.3 * torch.randn(n, n, generator=g)
    Q = 0.5 * (Qh + Qh.T)                                   # symmetric, indefinite
    assert float(torch.linalg.eigvalsh(Q).min()) < -0.1
    Y, U = torch.randn(B, T, p, generator=g), 0.3 * torch.randn(B, T, m, generator=g)
    R, mu0, S0 = 0.03 * torch.eye(p), torch.zeros(n), 0.5 * torch.eye(n)
    dev = lambda t: t.to(DEV)
    leaves = [dev(t).clone().requires_grad_(True) for t in (A, Bm, Cm, Y)]
    outs = LgssmSmooth.apply(leaves[3], dev(U), None, None, leaves[0], leaves[1], leaves[2], dev(Q), dev(R), dev(mu0), dev(S0),
                             Slots(), True)
    ref = c_oracle.smooth(Y, U, None, A, Bm, Cm, Q, R, mu0, S0)
    assert float(torch.linalg.eigvalsh(0.5 * (ref["Sigmas_pred"][0, -1] + ref["Sigmas_pred"][0, -1].T)).min()) < 0   # really indefinite
    for k, v in zip(("mus_smooth", "Sigmas_smooth", "mus_filt", "Sigmas_filt", "mus_pred", "Sigmas_pred"), outs):
        assert rel_err(v.detach().cpu(), ref[k]) < 2e-3, k
    w = [torch.randn(o.shape, generator=g) for o in outs[:2]]
    (sum((o * dev(wi)).sum() for o, wi in zip(outs[:2], w))).backward()
    def oracle_grads(dt):
        c = lambda t: t.to(dt)
        cl = [c(t).clone().requires_grad_(True) for t in (A, Bm, Cm, Y)]
        mu, Sig = c(mu0).expand(B, -1).unsqueeze(-1), c(S0).expand(B, -1, -1)
        ex = lambda M: M.expand(B, -1, -1)
        mfs, Sfs, mps, Sps = [], [], [], []
        for t in range(T):
            mu, Sig, mu_p, Sig_p = O.filter_step(mu, Sig, cl[3][:, t], c(U)[:, t], ex(cl[0]), ex(cl[1]), ex(cl[2]), c(Q), c(R),
                                                 torch.ones(B, dtype=dt))
            mfs.append(mu), Sfs.append(Sig), mps.append(mu_p), Sps.append(Sig_p)
        mus, Sigs = [mfs[-1]], [Sfs[-1]]
        for t in range(T - 2, -1, -1):
            m_s, S_s = O.smooth_step(Sfs[t], Sps[t + 1], Sigs[0], mfs[t], mps[t + 1], mus[0], ex(cl[0]))
            mus.insert(0, m_s), Sigs.insert(0, S_s)
        ((torch.stack(mus, 1).squeeze(-1) * c(w[0])).sum() + (torch.stack(Sigs, 1) * c(w[1])).sum()).backward()
        return [t.grad for t in cl]
    # Indefinite predicted covariances amplify rounding inside the recursion (the INPUT condition number is modest: an fp32-ulp
    # perturbation of the inputs moves the fp64 gradients by 1e-5).  Measured against the fp64 oracle: the fp32 oracle sits 7e-4
    # (A) and < 2.5e-3 (C) away; the kernels 3e-3 .. 6e-3 (A) and 6e-3 .. 1.4e-2 (C), and a recompilation that only
    # re-associates FMAs moves them inside those ranges.  This case pins the choice of path and sane values on a matrix no
    # Kalman filter should meet; the accuracy class of the kernels is pinned by latent_fp64_budget on the reference's own cases.
    g64, g32 = oracle_grads(torch.float64), oracle_grads(torch.float32)
    for name, got, w64, w32 in zip("A B C Y".split(), leaves, g64, g32):
        budget = max(4.0 * rel_err(w32.double(), w64), 2.5e-2)
        assert rel_err(got.grad.cpu().double(), w64) < budget, (name, budget)


def linearity(DEV, B=256, T=50):
    """Size-independent property at configs[1] size: the smoothed MEANS are linear in (y, u, mu0) for fixed
    dynamics, and the covariances do not depend on y at all."""
    from kvae.kalman.lgssm_ops import LgssmSmooth, Slots
    n, m, p = 4, 4, 2
    A, Bm, Cm, alpha, Y, U, mask, _ = _random_problem(B, T, n, m, p, 1, 7, DEV)
    R, Q = 0.03 * torch.eye(p, device=DEV), 0.02 * torch.eye(n, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    run = lambda y, u: LgssmSmooth.apply(y, u, mask, None, A[0], Bm[0], Cm[0], Q, R, mu0, S0, Slots(), True)
    with torch.no_grad():
        o1, o2, o12 = run(Y, U), run(2 * Y.flip(0), -U), run(Y + 2 * Y.flip(0), U - U)
    assert rel_err(o12[0], o1[0] + o2[0]) < 2e-4
    assert rel_err(o12[1], o1[1]) < 1e-5 and rel_err(o2[1], o1[1]) < 1e-5



def safe_cholesky_levels(DEV, n=4, B=2, T=4):
    """_safe_cholesky semantics: one bad Q_t forces the WHOLE batch up the jitter ladder / to the diagonal
    fallback, exactly like the oracle (kalman_filter.py:282-302).  n = 16: the matrix-core ELBO kernels resolve the
    level in their probe and hand levels > 0 to the generic main kernel on the device; (B, T) = (40, 10): more steps than
    one round of wavefronts of the four-steps-per-wavefront launch, ragged."""
    from kvae.kalman.lgssm_ops import LgssmElbo, Slots
    from oracle import c_oracle
    m, p = n, 2
    A, Bm, Cm, alpha, Y, U, mask, eps = _random_problem(B, T, n, m, p, 1, 5, DEV)
    R = 0.03 * torch.eye(p, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    mus = torch.randn(B, T, n, generator=torch.Generator().manual_seed(1)).to(DEV)
    Sig = (0.5 * torch.eye(n, device=DEV)).expand(B, T, n, n).contiguous()
    c = lambda t: t.cpu()
    for q00, want in ((0.02, 0), (-3e-6, 1), (-1.0, 5)):
        Q = (0.02 * torch.eye(n, device=DEV)).expand(B, T, n, n).contiguous()
        Q[1, 2, 0, 0] = q00
        total, terms, levels_dev = LgssmElbo.apply(mus, Sig, eps, Y, U, mask, None, A[0], Bm[0], Cm[0], Q, R, mu0, S0, Slots())
        rterms, levels = c_oracle.elbo_terms(c(mus), c(Sig), c(eps), c(Y), c(U), c(mask), c(A[0]), c(Bm[0]), c(Cm[0]), c(Q),
                                             c(R), c(mu0), c(S0))
        assert levels[1] == want, levels
        assert levels_dev.cpu().tolist()[:2] == list(levels[:2])
        if str(DEV).startswith("cuda"):   # which kernel family computed it: thread-per-step at n = 4, matrix cores at n = 16
            assert int(levels_dev[2]) in {4: (0, 1), 16: (2,)}.get(n, (0,)), (n, int(levels_dev[2]))
        for i in range(4):
            assert abs(float(terms[i]) - rterms[i]) <= 3e-4 * abs(rterms[i]) + 1e-3, (i, float(terms[i]), rterms[i])


def safe_cholesky_levels_shared_q(DEV, n=16, B=5, T=10):
    """The same ladder with ONE Q for the whole batch (lstm dynamics: a broadcast [n,n] operand) - at n = 16 the four-steps-per-
    wavefront kernels - and with the raised level coming from a smoothed covariance, so that the parked z_t have to be redone
    at the resolved level: (level of Sigma_s, level of Q) in {(0,0), (0,1), (3,0), (5,0), (2,5)}; values and every gradient
    against the C oracle / the torch oracle's autograd on the expanded stacks."""
    from kvae.kalman.lgssm_ops import LgssmElbo, Slots
    from oracle import c_oracle
    from oracle import torch_oracle as O
    m, p = n, 2
    A, Bm, Cm, alpha, Y, U, mask, eps = _random_problem(B, T, n, m, p, 1, 7, DEV)
    R = 0.03 * torch.eye(p, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)
    gen = torch.Generator().manual_seed(2)
    mus = torch.randn(B, T, n, generator=gen).to(DEV)
    W = torch.randn(B, T, n, n, generator=gen) * 0.1
    Sig0 = (W @ W.mT + 0.3 * torch.eye(n)).to(DEV)
    c = lambda t: t.detach().cpu()
    for sig_bad, q_bad, want in ((None, None, [0, 0]), (None, -3e-6, [0, 1]), (-4e-4, None, [3, 0]), (-1.0, None, [5, 0]),
                                 (-5e-5, -1.0, [2, 5])):
        Sig = Sig0.clone()
        if sig_bad is not None:
            Sig[B - 1, T - 3] = torch.diag(torch.tensor([sig_bad] + [0.2] * (n - 1))).to(DEV)
        Q = 0.02 * torch.eye(n, device=DEV)
        if q_bad is not None:
            Q[2, 2] = q_bad
        leaves = [t.clone().requires_grad_(True) for t in (mus, Sig, Y, A[0], Bm[0], Cm[0], Q)]
        total, terms, levels_dev = LgssmElbo.apply(leaves[0], leaves[1], eps, leaves[2], U, mask, None, leaves[3], leaves[4], leaves[5],
                                                   leaves[6], R, mu0, S0, Slots())
        assert levels_dev.cpu().tolist()[:2] == want, (levels_dev.cpu().tolist(), want)
        if str(DEV).startswith("cuda") and n == 16:
            assert int(levels_dev[2]) == 2, int(levels_dev[2])   # gQ is wanted here: one step per wavefront
        ex = lambda M: c(M).expand(B, T, *M.shape).contiguous()
        rterms, levels = c_oracle.elbo_terms(c(mus), c(Sig), c(eps), c(Y), c(U), c(mask), c(A[0]), c(Bm[0]), c(Cm[0]), ex(Q),
                                             c(R), c(mu0), c(S0))
        assert list(levels[:2]) == want
        for i in range(4):
            assert abs(float(terms[i]) - rterms[i]) <= 3e-4 * abs(rterms[i]) + 1e-3, (want, i, float(terms[i]), rterms[i])
        # gradients vs the torch oracle's autograd on the same problem
        ref = [c(t).clone().requires_grad_(True) for t in (mus, Sig, Y, A[0], Bm[0], Cm[0], Q)]
        e = lambda M: M.expand(B, T, *M.shape)
        want_total = O.lgssm_elbo(ref[0].unsqueeze(-1), ref[1], ref[2], c(U), e(ref[3]), e(ref[4]), e(ref[5]), e(ref[6]), c(R), c(mu0),
                                  c(S0), c(mask), c(eps)) * c(mask).sum().clamp(min=1.0)
        assert rel_err(total.detach().cpu(), want_total.detach()) < 1e-4, want
        total.backward()
        want_total.backward()
        for k, (got, r) in enumerate(zip(leaves, ref)):
            if r.grad is None or float(r.grad.abs().max()) == 0.0:
                assert got.grad is None or float(got.grad.abs().max()) < 1e-6, (want, k)
            else:
                assert rel_err(got.grad.cpu(), r.grad) < 3e-3, (want, k)
        # without gradients of Q the shared-Q call takes the four-steps-per-wavefront kernels (family 3): same value
        with torch.no_grad():
            tot4, _, lv4 = LgssmElbo.apply(mus, Sig, eps, Y, U, mask, None, A[0], Bm[0], Cm[0], Q, R, mu0, S0, Slots())
        assert lv4.cpu().tolist()[:2] == want and rel_err(tot4.cpu(), total.detach().cpu()) < 1e-5
        if str(DEV).startswith("cuda") and n == 16:
            assert int(lv4[2]) == 3, int(lv4[2])
        # ... and with gradients w.r.t. everything but Q (the training step of the lstm model, whose Q is a buffer)
        lv2 = [t.clone().requires_grad_(True) for t in (mus, Sig, Y, A[0], Bm[0], Cm[0])]
        tot5, _, lv5 = LgssmElbo.apply(lv2[0], lv2[1], eps, lv2[2], U, mask, None, lv2[3], lv2[4], lv2[5], Q, R, mu0, S0, Slots())
        tot5.backward()
        if str(DEV).startswith("cuda") and n == 16:
            assert int(lv5[2]) == 3, int(lv5[2])
        for k, (got, r) in enumerate(zip(lv2, ref[:6])):
            if r.grad is not None and float(r.grad.abs().max()) > 0.0:
                assert rel_err(got.grad.cpu(), r.grad) < 3e-3, (want, k, "four-step")


N16_ELBO_TOL = 1e-4   # per-(b,t) bar of n16_elbo_per_step (measured on gfx950: largest ratio 2.1e-6 over the GPU-tier cases)


def _per_step_ratio(got, ref):
    """Largest per-(b,t) error ratio max|got - ref| / max(max|ref| on the slice, 1e-2 max|ref| on the tensor) of a [B,T,...]
    gradient stack (float64 reference), and the (b,t) where it occurs."""
    B, T = ref.shape[:2]
    err = (got.double() - ref).abs().reshape(B, T, -1).amax(-1)
    scale = ref.abs().reshape(B, T, -1).amax(-1).clamp_min(1e-2 * float(ref.abs().max())).clamp_min(1e-30)
    ratio = err / scale
    k = int(ratio.argmax())
    return float(ratio.max()), divmod(k, T)


# ---- recurrent chain kernels (lstm_fast.h, gru_fast.h, regime_grid.h / regime_tpp.h / regime.h), one (b,t) slice at a time ----
# Bars = 4 x YARDSTICK (the factor values_vs_fp64_oracle uses for "as good as float32 can be"), where the yardstick of a quantity
# is the largest per-slice ratio of the FLOAT32 TORCH restatement of the operation (nn.LSTM, nn.GRU, regime_chain run in float32)
# against its float64 run, over the case lists of both tiers (tests/test_wave_emu_rnn.py, tests/test_wave_emu_reduce.py, tests/test_hostsim_ops.py,
# tests/test_gpu_parity.py; rerun: the case functions with yardstick=True).  Largest ratios the kernels reach against the same
# float64 run, emulated workgroups (expf, a division) | gfx950 (__expf, v_rcp):
#   lstm.h 4.3e-7 | 7.8e-7   lstm.gates 3.5e-7 | 5.8e-7   lstm.c_seq 4.1e-7 | 7.3e-7   lstm.dx 1.7e-6 | 6.1e-6   lstm.param 3.3e-7 | 3.5e-7
#   gru.h 2.6e-7 | 3.2e-7    gru.dx 1.2e-6 | 7.6e-6       gru.param 3.5e-7 | 3.0e-7
#   regime.y 4.2e-7 | 5.2e-7  log_q 2.4e-6 | 2.2e-6  log_p 6.5e-7 | 6.4e-7  g_logits 2.7e-5 | 3.3e-5  g_init 2.3e-5 | 1.5e-5
#   wgrad.wh / wx / b  4.8e-7 | 5.1e-7 / 1.9e-6 | 4.0e-6 / 1.2e-5 | 2.1e-5
#   mix.out / g_alpha / g_base  1.7e-7 | 2.4e-7 / 3.2e-6 | 4.5e-6 / 1.9e-7 | 2.9e-7
#   linear.y / dx / dw / db  6.9e-7 | 1.2e-6 / 1.1e-5 | 2.2e-5 / 2.0e-6 | 2.2e-6 / 7.7e-7 | 7.2e-7
#   (wgrad / mix / linear, emulated: the product's kernels on emulated workgroups, tests/test_wave_emu_reduce.py - every case of
#   that file; gfx950: the _ROW_CASES, _EDGE, _LARGE and batch lists of tests/test_gpu_parity.py)
# Less than a factor 2 under the bar: lstm.gates (1.16 x on gfx950, 1.9 x emulated), lstm.c_seq (1.45 x on gfx950), wgrad.b (1.86 x on
# gfx950); DESIGN section 2.
RNN_YARDSTICK = {   # float32 torch against float64 torch, largest per-slice ratio over the CPU and the GPU case lists
    "lstm.h": 3.96e-7, "lstm.gates": 1.69e-7, "lstm.c_seq": 2.65e-7, "lstm.dx": 6.61e-6, "lstm.param": 2.90e-6,
    "gru.h": 2.56e-7, "gru.dx": 8.04e-6, "gru.param": 6.16e-7,
    "mix.out": 2.42e-7, "mix.g_alpha": 8.74e-6, "mix.g_base": 6.11e-7,
    "linear.y": 1.65e-6, "linear.dx": 2.64e-5, "linear.dw": 1.24e-6, "linear.db": 8.09e-7,
    "wgrad.wh": 1.48e-6, "wgrad.wx": 1.01e-5, "wgrad.b": 9.78e-6,
    "regime.y": 9.32e-7, "regime.log_q": 2.43e-6, "regime.log_p": 6.48e-7, "regime.g_logits": 3.35e-5, "regime.g_init": 2.32e-5,
}
RNN_STEP_TOL = {k: 4.0 * v for k, v in RNN_YARDSTICK.items()}   # the bars of lstm_per_step / bigru_per_step / regime_per_step


def _check_steps(name, got, ref, bar, out):
    """Per-(b,t) comparison of one [B,T,...] stack against its float64 reference: every slice, none left out."""
    ratio, where = _per_step_ratio(got.detach().cpu(), ref.detach())
    out[name] = max(out.get(name, 0.0), ratio)
    assert ratio < bar, (name, ratio, where, bar)


def _check_whole(name, got, ref, bar, out):
    ratio = rel_err(got.detach().cpu(), ref.detach())
    out[name] = max(out.get(name, 0.0), ratio)
    assert ratio < bar, (name, ratio, bar)


def _upstream(w, steps):
    """The upstream gradient on every step ("all") or on one step only ("first": t = 0, "last": t = T - 1), the others zero:
    with a single step a dropped carry of the recurrence is the whole gradient of the other steps, not a small part of it."""
    if steps == "all":
        return w
    m = torch.zeros_like(w)
    t = 0 if steps == "first" else w.shape[1] - 1
    m[:, t] = w[:, t]
    return m


def _rnn_launches(lib):
    return [lib.dll.kvae_wemu_rnn_launches(i) for i in range(10)] if hasattr(lib.dll, "kvae_wemu_rnn_launches") else None


def _lstm_restated(mod, x):
    """gates [B,T,4H] (i, f, g, o after their nonlinearities), c_seq, h_seq of a single-layer nn.LSTM from a zero state, in
    the module's dtype: what LstmSequence saves for its backward."""
    B, T, _ = x.shape
    H = mod.hidden_size
    h, c = x.new_zeros(B, H), x.new_zeros(B, H)
    gs, cs, hs = [], [], []
    for t in range(T):
        pre = x[:, t] @ mod.weight_ih_l0.T + mod.bias_ih_l0 + h @ mod.weight_hh_l0.T + mod.bias_hh_l0
        i, f, g, o = pre.split(H, -1)
        i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
        c = f * c + i * g
        h = o * c.tanh()
        gs.append(torch.cat([i, f, g, o], -1)), cs.append(c), hs.append(h)
    return torch.stack(gs, 1), torch.stack(cs, 1), torch.stack(hs, 1)


def lstm_per_step(DEV, B, T, steps="all", yardstick=False):
    """kvae_lstm_fwd/bwd at (H, I) = (50, 2) (k_lstm_fwd_fast / k_lstm_bwd_fast) against torch.nn.LSTM in FLOAT64 on the same
    weights and inputs: h, the saved gates and c_seq, and dx per (b,t); the parameter gradients as whole tensors.  `steps`: see
    _upstream.  On the emulated backend the launch counters must show that the fast kernels ran.  Returns the largest ratios."""
    from kvae import _native
    from kvae.kalman.lgssm_ops import LstmSequence
    torch.manual_seed(1000 * B + 10 * T + len(steps))
    ref = torch.nn.LSTM(2, 50, batch_first=True).double()
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    x = torch.randn(B, T, 2, dtype=torch.float64)
    w = _upstream(torch.randn(B, T, 50, dtype=torch.float64), steps)
    xr = x.clone().requires_grad_(True)
    h64 = ref(xr)[0]
    (h64 * w).sum().backward()
    with torch.no_grad():
        gates64, c64, h_re = _lstm_restated(ref, x)
    assert float((h_re - h64.detach()).abs().max()) < 1e-12   # the restatement that supplies gates / c_seq IS nn.LSTM
    out = {}
    if yardstick:   # float32 torch in place of the kernels
        m32 = torch.nn.LSTM(2, 50, batch_first=True)
        m32.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        xd = x.float().requires_grad_(True)
        h = m32(xd)[0]
        (h * w.float()).sum().backward()
        with torch.no_grad():
            gates, c, _ = _lstm_restated(m32, x.float())
        pg = [getattr(m32, n).grad for n in names]
    else:
        lib = _native.lib_for(torch.zeros(1, device=DEV))
        before = _rnn_launches(lib) if DEV == "cpu" else None
        params = [getattr(ref, n).detach().float().to(DEV).requires_grad_(True) for n in names]
        xd = x.float().to(DEV).requires_grad_(True)
        h = LstmSequence.apply(xd, *params)
        _, _, _, _, gates, c = h.grad_fn.saved_tensors
        (h * w.float().to(DEV)).sum().backward()
        pg = [q.grad for q in params]
        if before is not None:
            after = _rnn_launches(lib)
            assert after[0] == before[0] + 1 and after[1] == before[1] + 1, (before, after)
    _check_steps("lstm.h", h, h64, RNN_STEP_TOL["lstm.h"], out)
    _check_steps("lstm.gates", gates, gates64, RNN_STEP_TOL["lstm.gates"], out)
    _check_steps("lstm.c_seq", c, c64, RNN_STEP_TOL["lstm.c_seq"], out)
    _check_steps("lstm.dx", xd.grad, xr.grad, RNN_STEP_TOL["lstm.dx"], out)
    for n, got in zip(names, pg):
        _check_whole("lstm.param", got, getattr(ref, n).grad, RNN_STEP_TOL["lstm.param"], out)
    return out


def bigru_per_step(DEV, B, T, steps="all", yardstick=False):
    """kvae_bigru_fwd/bwd (k_gru_fwd_fast / k_gru_bwd_fast, grid (B, 2)) against torch.nn.GRU(bidirectional=True) in FLOAT64:
    h (both directions' columns) and dx per (b,t), the eight parameter gradients as whole tensors."""
    from kvae import _native
    from kvae.kalman.lgssm_ops import BiGruSequence
    torch.manual_seed(2000 * B + 10 * T + len(steps))
    ref = torch.nn.GRU(2, 50, batch_first=True, bidirectional=True).double()
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
             "bias_ih_l0_reverse", "bias_hh_l0_reverse"]
    x = torch.randn(B, T, 2, dtype=torch.float64)
    w = _upstream(torch.randn(B, T, 100, dtype=torch.float64), steps)
    xr = x.clone().requires_grad_(True)
    h64 = ref(xr)[0]
    (h64 * w).sum().backward()
    out = {}
    if yardstick:
        m32 = torch.nn.GRU(2, 50, batch_first=True, bidirectional=True)
        m32.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        xd = x.float().requires_grad_(True)
        h = m32(xd)[0]
        (h * w.float()).sum().backward()
        pg = [getattr(m32, n).grad for n in names]
    else:
        lib = _native.lib_for(torch.zeros(1, device=DEV))
        before = _rnn_launches(lib) if DEV == "cpu" else None
        params = [getattr(ref, n).detach().float().to(DEV).requires_grad_(True) for n in names]
        xd = x.float().to(DEV).requires_grad_(True)
        h = BiGruSequence.apply(xd, *params)
        (h * w.float().to(DEV)).sum().backward()
        pg = [q.grad for q in params]
        if before is not None:
            after = _rnn_launches(lib)
            assert after[2] == before[2] + 1 and after[3] == before[3] + 1, (before, after)
    _check_steps("gru.h", h, h64, RNN_STEP_TOL["gru.h"], out)
    _check_steps("gru.dx", xd.grad, xr.grad, RNN_STEP_TOL["gru.dx"], out)
    for n, got in zip(names, pg):
        _check_whole("gru.param", got, getattr(ref, n).grad, RNN_STEP_TOL["gru.param"], out)
    return out


REGIME_FAMILIES = {"grid": (4, 5), "tpp": (6, 7), "lds": (8, 9)}   # indices of kvae_wemu_rnn_launches (forward, backward)
REGIME_HARD_GAP = 1e-3   # least top-two gap of (l + g) / tau in the float64 run for which a hard sample is compared


def regime_per_step(DEV, B, T, K, tau, hard, family=None, tau_dev=False, seed=0, yardstick=False):
    """kvae_regime_fwd/bwd against SwitchingDynamicsParameter.regime_chain in FLOAT64: y, log_q, log_p and g_logits per (b,t),
    g_init per b.  `family` ("grid", "tpp", "lds"): the kernel family that must run, asserted from the launch counters of the
    emulated backend (the GPU build has no counter: there the family is chosen by KVAE_REGIME_TPP in a fresh process).
    `tau_dev`: tau as a one-element device tensor the kernels read.  A hard sample is compared only where float32 and float64
    must agree on the arg-maximum: the float64 run's top-two gap of (l + g) / tau is ASSERTED above REGIME_HARD_GAP at every
    (b,t), so a seed that does not give that fails here.  T = 1 reads no transition logits: their gradient must be exactly 0."""
    from kvae import _native
    from kvae.kalman.lgssm_ops import RegimeChain
    from kvae.kalman.switch_dyn_param import StickyRegimePrior, SwitchingDynamicsParameter
    g = torch.Generator().manual_seed(10000 * seed + 1000 * B + 10 * T + K)
    logits = torch.randn(B, T, K, K, generator=g, dtype=torch.float64)
    init = torch.randn(B, K, generator=g, dtype=torch.float64)
    gum = -torch.empty(B, T, K, dtype=torch.float64).exponential_(generator=g).log()
    w_y, w_q, w_p = (torch.randn(*sh, generator=g, dtype=torch.float64) for sh in ((B, T, K), (B, T), (B, T)))
    # the values the kernels see are float32: the float64 run starts from the same numbers
    logits, init, gum, w_y, w_q, w_p = (t.float().double() for t in (logits, init, gum, w_y, w_q, w_p))
    tau = float(torch.tensor(tau, dtype=torch.float32))

    def chain(dtype):
        dyn = SwitchingDynamicsParameter(torch.eye(4).repeat(K, 1, 1), torch.zeros(K, 4, 4), torch.zeros(K, 2, 4),
                                         prior=StickyRegimePrior(K, 0.8))
        dyn.tau = tau
        lr, ir = logits.to(dtype).clone().requires_grad_(True), init.to(dtype).clone().requires_grad_(True)
        y, lq, lp = dyn.regime_chain(lr, ir, gum.to(dtype), hard)
        ((y * w_y.to(dtype)).sum() + (lq * w_q.to(dtype)).sum() + (lp * w_p.to(dtype)).sum()).backward()
        g_l = lr.grad if lr.grad is not None else torch.zeros_like(logits, dtype=dtype)   # T == 1: transition logits unused
        return dyn, y.detach(), lq.detach(), lp.detach(), g_l, ir.grad

    dyn, y64, lq64, lp64, gl64, gi64 = chain(torch.float64)
    if hard and K > 1:
        l = torch.cat([init[:, None], torch.einsum("bti,btij->btj", y64[:, :-1], logits[:, 1:])], 1)
        top = ((l + gum) / tau).topk(2, -1).values
        gap = float((top[..., 0] - top[..., 1]).min())
        assert gap > REGIME_HARD_GAP, ("seed gives a near-tie of the hard sample", B, T, K, seed, gap)
    out = {}
    if yardstick:
        _, y, lq, lp, g_l, g_i = chain(torch.float32)
    else:
        lib = _native.lib_for(torch.zeros(1, device=DEV))
        before = _rnn_launches(lib) if DEV == "cpu" else None
        ld, idv = logits.float().to(DEV).requires_grad_(True), init.float().to(DEV).requires_grad_(True)
        P = dyn.prior.transition_matrix.to(DEV)
        tau_arg = torch.tensor(tau, dtype=torch.float32, device=DEV) if tau_dev else tau
        y, lq, lp = RegimeChain.apply(ld, idv, gum.float().to(DEV), P, tau_arg, hard)
        ((y * w_y.float().to(DEV)).sum() + (lq * w_q.float().to(DEV)).sum() + (lp * w_p.float().to(DEV)).sum()).backward()
        g_l, g_i = ld.grad, idv.grad
        if before is not None and family is not None:
            after = _rnn_launches(lib)
            delta = [a - b for a, b in zip(after, before)][4:]
            want = [1 if 4 + i in REGIME_FAMILIES[family] else 0 for i in range(6)]
            assert delta == want, (family, delta)
    _check_steps("regime.y", y, y64, RNN_STEP_TOL["regime.y"], out)
    _check_steps("regime.log_q", lq, lq64, RNN_STEP_TOL["regime.log_q"], out)
    _check_steps("regime.log_p", lp, lp64, RNN_STEP_TOL["regime.log_p"], out)
    if T == 1:
        assert float(g_l.abs().max()) == 0.0, "T = 1: the gradient of the transition logits is exactly zero"
    else:
        assert float(g_l[:, 0].abs().max()) == 0.0, "the transition logits of t = 0 are never read"
        _check_steps("regime.g_logits", g_l, gl64, RNN_STEP_TOL["regime.g_logits"], out)
    _check_steps("regime.g_init", g_i[:, None], gi64[:, None], RNN_STEP_TOL["regime.g_init"], out)
    return out


def n16_elbo_per_step(DEV, B, T, family, levels=(0, 0), grads=True, q_shared=False):
    """The (16,16,2) ELBO kernels (csrc/lgssm_n16_elbo.h) step by step against a FLOAT64 run of the torch oracle.
    family 2: per-step A, B, C and Q, one wavefront per (b,t) (k_elbo_n16<GRADS, HAS_GQ>) - with q_shared, ONE Q for the batch
    whose gradient is wanted, which keeps the call on one step per wavefront; family 3: a Q shared by the batch and no gradient
    of Q, four steps per wavefront (k_elbo4_n16<GRADS>).  `levels` = (level of Sigma_s, level of Q) of _safe_cholesky, forced by poisoning one
    matrix.  The mask is zero at t = 0, at t = T-1, at the first step of the last four-step group and, when B > 1, for a whole
    sequence.  Checks: the resolved levels and the family that ran (the launch reports it, so no tier passes on the generic
    kernels); the total within 1e-4 of float64; and every gradient stack per (b,t) - max|got - ref| on the slice within
    N16_ELBO_TOL of max(max|ref| on the slice, 1e-2 max|ref| on the tensor) - so a wrong tail group, step 0 (the only step whose
    row-group 3 factorises Sigma0) or a masked step cannot hide behind the tensor's largest entry.  g mus / g Sigma_s must be
    finite everywhere; a broadcast Q is compared as a whole tensor at the same bar.  Returns {name: (largest per-slice ratio, (b, t))}."""
    from kvae.kalman.lgssm_ops import LgssmElbo, Slots
    from oracle import c_oracle
    from oracle import torch_oracle as O
    assert family in (2, 3)
    n, m, p = 16, 16, 2
    assert not (q_shared and family == 3)
    shared = family == 3 or q_shared
    g = torch.Generator().manual_seed(1000 + 37 * B + T)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    mus = 0.5 * rn(B, T, n)
    W = 0.1 * rn(B, T, n, n)
    Sig = W @ W.mT + 0.3 * eye                                 # dense SPD
    eps, Y, U = rn(B, T, n), rn(B, T, p), 0.3 * rn(B, T, m)
    A = 0.9 * eye + 0.08 * rn(B, T, n, n)
    Bm, Cm = 0.1 * rn(B, T, n, m), 0.3 * rn(B, T, p, n)
    Wq = rn(*(() if shared else (B, T)), n, n)
    Q = 0.02 * eye + 0.0005 * (Wq @ Wq.mT)                      # dense SPD: a factor and its transpose differ
    R = torch.tensor([[0.03, 0.01], [0.01, 0.05]], dtype=torch.float64)
    mu0 = 0.1 * rn(n)
    W0 = 0.2 * rn(n, n)
    S0 = W0 @ W0.T + 0.5 * eye                                  # dense: row-group 3 factorises a real matrix at t = 0
    mask = torch.ones(B, T, dtype=torch.float64)
    mask[:, 0] = 0.0
    mask[:, T - 1] = 0.0
    mask[:, 4 * ((T - 1) // 4)] = 0.0
    if B > 1:
        mask[1] = 0.0
    lvS, lvQ = levels
    sig_bad = {0: None, 2: -5e-5, 3: -4e-4, 5: -1.0}[lvS]
    q_bad = {0: None, 1: -3e-6, 5: -1.0}[lvQ]
    if sig_bad is not None:
        Sig[B - 1, max(T - 3, 0)] = torch.diag(torch.tensor([sig_bad] + [0.2] * (n - 1), dtype=torch.float64))
    if q_bad is not None:
        assert T >= 2, "Q_t is factorised for t >= 1 only"
        bad = torch.diag(torch.tensor([0.02] * 2 + [q_bad] + [0.02] * (n - 3), dtype=torch.float64))
        if not shared:
            Q[0, T - 1] = bad
        else:
            Q = bad
    # the float32 operands are the problem; the float64 reference runs on exactly their values
    f32 = [t.float() for t in (mus, Sig, eps, Y, U, mask, A, Bm, Cm, Q, R, mu0, S0)]
    mus, Sig, eps, Y, U, mask, A, Bm, Cm, Q, R, mu0, S0 = [t.double() for t in f32]
    d = [t.to(DEV) for t in f32]
    names = ["mus", "Sigmas", "Y", "U", "A", "B", "C"] + (["Q"] if family == 2 else [])
    idx = {"mus": 0, "Sigmas": 1, "Y": 3, "U": 4, "A": 6, "B": 7, "C": 8, "Q": 9}
    leaves = [d[idx[k]].clone().requires_grad_(grads) for k in names]
    lv = dict(zip(names, leaves))
    args = [lv.get(k, d[i]) for i, k in enumerate(("mus", "Sigmas", "eps", "Y", "U", "mask", "A", "B", "C", "Q"))]
    with torch.set_grad_enabled(grads):
        total, terms, levels_dev = LgssmElbo.apply(*args[:6], None, *args[6:], d[10], d[11], d[12], Slots())
    c = lambda t: t.detach().cpu()
    Qx = Q.expand(B, T, n, n)
    _, rlevels = c_oracle.elbo_terms(*(t.float() for t in (mus, Sig, eps, Y, U, mask, A, Bm, Cm, Qx, R, mu0, S0)))
    assert list(rlevels[:2]) == list(levels), (list(rlevels), levels)
    got_lv = c(levels_dev).tolist()
    assert got_lv[:2] == list(levels), (got_lv, levels)
    assert got_lv[2] == family, ("kernel family", got_lv[2], family)
    # float64 reference
    ref = {k: v.clone().requires_grad_(grads) for k, v in (("mus", mus), ("Sigmas", Sig), ("Y", Y), ("U", U), ("A", A), ("B", Bm),
                                                            ("C", Cm), ("Q", Q))}
    with torch.set_grad_enabled(grads):
        rterms = O.lgssm_elbo_terms(ref["mus"], ref["Sigmas"], ref["Y"], ref["U"], ref["A"], ref["B"], ref["C"], ref["Q"], R, mu0,
                                    S0, mask, eps)
        rtotal = sum(rterms)
    total_f, rtotal_f = float(total.detach()), float(rtotal.detach())
    assert abs(total_f - rtotal_f) <= 1e-4 * abs(rtotal_f), (total_f, rtotal_f)
    for i in range(4):
        assert abs(float(terms[i]) - float(rterms[i].detach())) <= 1e-4 * abs(float(rterms[i].detach())) + 1e-3, (i, float(terms[i]), float(rterms[i].detach()))
    if not grads:
        return {}
    total.backward()
    rtotal.backward()
    out = {}
    for k in names:
        got = c(lv[k].grad)
        assert got is not None and bool(torch.isfinite(got).all()), (k, "non-finite gradient")
        want = ref[k].grad
        if want.dim() == 2:   # a broadcast Q: the whole tensor
            out[k] = (float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30)), None)
        else:
            out[k] = _per_step_ratio(got, want)
        assert out[k][0] <= N16_ELBO_TOL, (k, out[k], levels, family)
    return out


def n16_elbo_unaligned(DEV, B=2, T=5):
    """The (16,16,2) ELBO with a Sigma_s stack that starts 4 bytes off a 16-byte boundary: the gate of kvae_lgssm_elbo
    (16-byte row loads / stores) sends it to the generic kernels (family 0), the aligned call to the matrix-core ones (family 2):
    same total, same gradients (per (b,t), see n16_elbo_per_step)."""
    from kvae.kalman.lgssm_ops import LgssmElbo, Slots
    n, m, p = 16, 16, 2
    g = torch.Generator().manual_seed(31)
    rn = lambda *s: torch.randn(*s, generator=g)
    mus, eps, Y, U = 0.5 * rn(B, T, n), rn(B, T, n), rn(B, T, p), 0.3 * rn(B, T, m)
    W = 0.1 * rn(B, T, n, n)
    Sig = W @ W.mT + 0.3 * torch.eye(n)
    A, Bm, Cm = torch.eye(n) + 0.08 * rn(B, T, n, n), 0.1 * rn(B, T, n, m), 0.3 * rn(B, T, p, n)
    Wq = rn(B, T, n, n)
    Q = 0.02 * torch.eye(n) + 0.0005 * (Wq @ Wq.mT)
    R, mu0, S0 = 0.03 * torch.eye(p), 0.1 * rn(n), 2.0 * torch.eye(n)
    mask = (torch.rand(B, T, generator=g) > 0.3).float()
    d = lambda t: t.to(DEV)
    res = []
    for odd in (False, True):
        leaves = [d(t).clone().requires_grad_(True) for t in (mus, Y, U, A, Bm, Cm, Q)]
        base = torch.zeros(B * T * n * n + (1 if odd else 0), device=DEV)
        base[(1 if odd else 0):].copy_(d(Sig).reshape(-1))
        base.requires_grad_(True)
        Sig_in = base[(1 if odd else 0):].view(B, T, n, n)        # (a .clone() would re-align it)
        assert (Sig_in.data_ptr() % 16 != 0) == odd
        total, _, levels = LgssmElbo.apply(leaves[0], Sig_in, d(eps), leaves[1], leaves[2], d(mask), None, leaves[3], leaves[4],
                                           leaves[5], leaves[6], d(R), d(mu0), d(S0), Slots())
        total.backward()
        gS = base.grad[(1 if odd else 0):].view(B, T, n, n)
        res.append((float(total.detach()), int(levels[2]), [gS.cpu()] + [t.grad.cpu() for t in leaves]))
    (t_fast, fam_fast, g_fast), (t_slow, fam_slow, g_slow) = res
    assert (fam_fast, fam_slow) == (2, 0), (fam_fast, fam_slow)
    assert abs(t_fast - t_slow) <= 2e-5 * abs(t_slow), (t_fast, t_slow)
    for k, a, b in zip(("Sigmas", "mus", "Y", "U", "A", "B", "C", "Q"), g_fast, g_slow):
        r = _per_step_ratio(a, b.double())
        assert r[0] <= 1e-3, (k, r)


def jitter_golden(DEV, name, levels, family=None):
    """The product's ELBO (probe + atomicMax level + terms + gradients, csrc/lgssm_elbo.h) against fixtures that drive the
    REFERENCE's own elbo past level 0 of _safe_cholesky (tests/golden/make_goldens_r2.py): resolved levels, value
    (1e-4 rel, north_star) and every gradient the reference's autograd produced (3e-3 rel)."""
    from golden_util import JITTER_GRADS, load
    from kvae.kalman.lgssm_ops import LgssmElbo, Slots
    g = load(name)
    d = {k: v.to(DEV) for k, v in g.items()}
    leaves = {k: d[k].clone().requires_grad_(True) for k in JITTER_GRADS}
    total, _, levels_dev = LgssmElbo.apply(leaves["mu_s"], leaves["Sig_s"], d["eps_z"], leaves["a"], d["u"], d["mask"], None,
                               leaves["A_list"], leaves["B_list"], leaves["C_list"], leaves["Q_list"], d["R"], d["mu0"],
                               d["Sigma0"], Slots())
    assert levels_dev.cpu().tolist()[:2] == levels
    if family is not None:   # (the CPU tier on emulated wavefronts: tests/test_wave_emu_elbo.py)
        assert int(levels_dev[2]) == family, int(levels_dev[2])
    if str(DEV).startswith("cuda") and d["Sig_s"].shape[-1] == 16:
        # the (16,16,2) matrix-core kernels computed this call at a RAISED level themselves (no generic backup launch):
        # family 2 = one step per wavefront (a per-step Q_list)
        assert int(levels_dev[2]) == 2, int(levels_dev[2])
    elbo = total / d["mask"].sum().clamp(min=1.0)
    assert rel_err(elbo.detach().cpu(), g["elbo"]) < 1e-4
    (-elbo).backward()
    for k, leaf in leaves.items():
        assert rel_err(leaf.grad.cpu(), g["grad." + k]) < 3e-3, k


def lstm_vs_torch(DEV, B, T, I, H):
    """kvae_lstm_fwd/bwd vs torch.nn.LSTM on the CPU (values and all gradients)."""
    from kvae.kalman.lgssm_ops import LstmSequence
    torch.manual_seed(B * 100 + T)
    ref = torch.nn.LSTM(I, H, batch_first=True)
    x = torch.randn(B, T, I)
    w = torch.randn(B, T, H)
    xr = x.clone().requires_grad_(True)
    (ref(xr)[0] * w).sum().backward()
    params = [p.detach().clone().to(DEV).requires_grad_(True) for p in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0,
                                                                        ref.bias_hh_l0)]
    xd = x.clone().to(DEV).requires_grad_(True)
    h = LstmSequence.apply(xd, *params)
    (h * w.to(DEV)).sum().backward()
    assert rel_err(h.detach().cpu(), ref(x)[0].detach()) < 2e-5
    assert rel_err(xd.grad.cpu(), xr.grad) < 1e-4
    for got, want in zip(params, (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)):
        assert rel_err(got.grad.cpu(), want.grad) < 1e-4


def vae_epilogue_vs_torch(DEV, N, C, H, W, r, relu):
    """kvae_bias_shuffle_act_fwd/bwd vs conv-bias + nn.PixelShuffle + nn.ReLU of torch (values and gradients)."""
    import torch.nn.functional as F
    from kvae.vae.fused import BiasShuffleAct
    g = torch.Generator().manual_seed(N + C + H)
    x = torch.randn(N, C * r * r, H, W, generator=g)
    b = torch.randn(C * r * r, generator=g)
    w = torch.randn(N, C, H * r, W * r, generator=g)
    xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.pixel_shuffle(xr + br.view(1, -1, 1, 1), r) if r > 1 else xr + br.view(1, -1, 1, 1)
    ref = F.relu(ref) if relu else ref
    (ref * w).sum().backward()
    xd, bd = x.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    out = BiasShuffleAct.apply(xd, bd, r, relu)
    (out * w.to(DEV)).sum().backward()
    assert torch.equal(out.detach().cpu(), ref.detach())
    assert torch.equal(xd.grad.cpu(), xr.grad)
    assert rel_err(bd.grad.cpu(), br.grad) < 1e-5


def regime_vs_torch(DEV, B, T, K, tau, hard):
    """kvae_regime_fwd/bwd vs the step-by-step torch restatement of switch_dyn_param.py:52-79 (values and grads)."""
    from kvae.kalman.lgssm_ops import RegimeChain
    from kvae.kalman.switch_dyn_param import StickyRegimePrior, SwitchingDynamicsParameter
    g = torch.Generator().manual_seed(B + T + K)
    logits = torch.randn(B, T, K, K, generator=g)
    init = torch.randn(B, K, generator=g)
    gum = -torch.empty(B, T, K).exponential_(generator=g).log()
    w_y, w_q, w_p = torch.randn(B, T, K, generator=g), torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)
    dyn = SwitchingDynamicsParameter(torch.eye(4).repeat(K, 1, 1), torch.zeros(K, 4, 4), torch.zeros(K, 2, 4),
                                     prior=StickyRegimePrior(K, 0.8))
    dyn.tau = tau
    lr, ir = logits.clone().requires_grad_(True), init.clone().requires_grad_(True)
    y, lq, lp = dyn.regime_chain(lr, ir, gum, hard)
    ((y * w_y).sum() + (lq * w_q).sum() + (lp * w_p).sum()).backward()
    ld, idv = logits.clone().to(DEV).requires_grad_(True), init.clone().to(DEV).requires_grad_(True)
    P = dyn.prior.transition_matrix.to(DEV)
    y2, lq2, lp2 = RegimeChain.apply(ld, idv, gum.to(DEV), P, tau, hard)
    ((y2 * w_y.to(DEV)).sum() + (lq2 * w_q.to(DEV)).sum() + (lp2 * w_p.to(DEV)).sum()).backward()
    assert rel_err(y2.detach().cpu(), y.detach()) < 2e-5
    assert rel_err(lq2.detach().cpu(), lq.detach()) < 2e-5 and rel_err(lp2.detach().cpu(), lp.detach()) < 2e-5
    ref_lg = lr.grad if lr.grad is not None else torch.zeros_like(logits)   # T == 1: transition logits unused
    assert (ld.grad.cpu() - ref_lg).abs().max() <= 2e-4 * ref_lg.abs().max() + 1e-12
    assert rel_err(idv.grad.cpu(), ir.grad) < 2e-4


def bce_frames_vs_torch(DEV, B, T, C, H, W):
    import torch.nn.functional as F
    from kvae.vae.fused import BernoulliFrameLogLik
    g = torch.Generator().manual_seed(B + T + H)
    logits = 3 * torch.randn(B, T, C, H, W, generator=g)
    x = (torch.rand(B, T, C, H, W, generator=g) < 0.2).float()
    w = torch.randn(B, T, generator=g)
    lr = logits.clone().requires_grad_(True)
    ref = -F.binary_cross_entropy_with_logits(lr, x, reduction="none").sum(dim=(2, 3, 4))
    (ref * w).sum().backward()
    ld = logits.clone().to(DEV).requires_grad_(True)
    out = BernoulliFrameLogLik.apply(ld, x.to(DEV))
    (out * w.to(DEV)).sum().backward()
    assert rel_err(out.detach().cpu(), ref.detach()) < 1e-5
    assert rel_err(ld.grad.cpu(), lr.grad) < 1e-5


def conv_edge_vs_torch(DEV, N):
    """Direct decoder-head / encoder-stem kernels == conv2d (+ pixel_shuffle / relu) of torch, values and gradients.
    Tolerance 2e-5 relative (fp32, different summation order over 288 / 9 taps and over the frames)."""
    import torch.nn.functional as F
    from kvae.vae.fused import DecoderHead, EncoderStem
    g = torch.Generator().manual_seed(N)
    h = torch.relu(torch.randn(N, 32, 16, 16, generator=g))
    W = 0.1 * torch.randn(4, 32, 3, 3, generator=g)
    b = torch.randn(4, generator=g)
    up = torch.randn(N, 1, 32, 32, generator=g)
    hr, Wr, br = (t.clone().requires_grad_(True) for t in (h, W, b))
    ref = F.pixel_shuffle(F.conv2d(hr, Wr, br, padding=1), 2)
    (ref * up).sum().backward()
    hd, Wd, bd = (t.clone().to(DEV).requires_grad_(True) for t in (h, W, b))
    out = DecoderHead.apply(hd, Wd, bd)
    (out * up.to(DEV)).sum().backward()
    assert rel_err(out.detach().cpu(), ref.detach()) < 2e-5
    for a, r in ((hd, hr), (Wd, Wr), (bd, br)):
        assert rel_err(a.grad.cpu(), r.grad) < 2e-5

    x = torch.rand(N, 1, 32, 32, generator=g)
    W = 0.3 * torch.randn(32, 1, 3, 3, generator=g)
    b = 0.1 * torch.randn(32, generator=g)
    up = torch.randn(N, 32, 16, 16, generator=g)
    Wr, br = (t.clone().requires_grad_(True) for t in (W, b))
    pre = F.conv2d(x, Wr, br, stride=2, padding=1)
    up = up * (pre.detach().abs() > 1e-5)   # no upstream gradient where rounding picks the ReLU mask (see dec_up_vs_torch)
    ref = torch.relu(pre)
    (ref * up).sum().backward()
    Wd, bd = (t.clone().to(DEV).requires_grad_(True) for t in (W, b))
    out = EncoderStem.apply(x.to(DEV), Wd, bd)
    (out * up.to(DEV)).sum().backward()
    assert rel_err(out.detach().cpu(), ref.detach()) < 2e-5
    for a, r in ((Wd, Wr), (bd, br)):
        assert rel_err(a.grad.cpu(), r.grad) < 2e-5


def enc_mid_vs_torch(DEV, N, side):
    """MFMA stride-2 encoder layers == relu(conv2d(stride 2)) of torch, values and all three gradients.  Tolerance 3e-5
    relative: exact-f32 MFMA is a k-ordered fmaf chain, torch's conv sums the 288 taps in another order."""
    import torch.nn.functional as F
    from kvae.vae.fused import EncoderMid
    g = torch.Generator().manual_seed(N * side)
    x = torch.relu(torch.randn(N, 32, side, side, generator=g))
    W = 0.08 * torch.randn(32, 32, 3, 3, generator=g)
    b = 0.1 * torch.randn(32, generator=g)
    up = torch.randn(N, 32, side // 2, side // 2, generator=g)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    pre = F.conv2d(xr, Wr, br, stride=2, padding=1)
    up = up * (pre.detach().abs() > 1e-5)   # no upstream gradient where rounding picks the ReLU mask (see dec_up_vs_torch)
    ref = torch.relu(pre)
    (ref * up).sum().backward()
    xd, Wd, bd = (t.clone().to(DEV).requires_grad_(True) for t in (x, W, b))
    out = EncoderMid.apply(xd, Wd, bd)
    (out * up.to(DEV)).sum().backward()
    assert rel_err(out.detach().cpu(), ref.detach()) < 3e-5
    for a, r in ((xd, xr), (Wd, Wr), (bd, br)):
        assert rel_err(a.grad.cpu(), r.grad) < 3e-5


def dec_up_vs_torch(DEV, N, side):
    """Register-stationary MFMA decoder blocks == relu(pixel_shuffle(conv2d)) of torch, values and all three gradients.
    Tolerance 3e-5 relative (fp32; different summation order over 288 / 1152 taps and over the frames)."""
    import torch.nn.functional as F
    from kvae.vae.fused import DecoderUp
    g = torch.Generator().manual_seed(N * side + 1)
    x = torch.relu(torch.randn(N, 32, side, side, generator=g))
    W = 0.08 * torch.randn(128, 32, 3, 3, generator=g)
    b = 0.1 * torch.randn(128, generator=g)
    up = torch.randn(N, 32, 2 * side, 2 * side, generator=g)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    pre = F.pixel_shuffle(F.conv2d(xr, Wr, br, padding=1), 2)
    # a pre-activation within rounding of 0 may land on either side of the ReLU depending on the summation order (direct /
    # Winograd / torch's): such pixels carry no upstream gradient here, so the mask they pick cannot decide the comparison
    up = up * (pre.detach().abs() > 1e-5)
    ref = torch.relu(pre)
    (ref * up).sum().backward()
    xd, Wd, bd = (t.clone().to(DEV).requires_grad_(True) for t in (x, W, b))
    out = DecoderUp.apply(xd, Wd, bd)
    (out * up.to(DEV)).sum().backward()
    assert rel_err(out.detach().cpu(), ref.detach()) < 3e-5
    for a, r in ((xd, xr), (Wd, Wr), (bd, br)):
        assert rel_err(a.grad.cpu(), r.grad) < 3e-5


def vae_heads_vs_torch(DEV, N):
    """Fused encoder heads (+ reparameterisation), decoder fc and latent regulariser == the torch expressions of the
    reference, values and gradients.  Tolerance 2e-5 relative (fp32, different summation order over 512 features / N rows)."""
    import torch.nn.functional as F
    from kvae.vae.fused import DecoderFc, EncoderHead, LatentReg
    g = torch.Generator().manual_seed(N + 7)
    feat = torch.relu(torch.randn(N, 512, generator=g))
    Wm, bm = 0.05 * torch.randn(2, 512, generator=g), 0.1 * torch.randn(2, generator=g)
    Wv, bv = 0.05 * torch.randn(2, 512, generator=g), 0.1 * torch.randn(2, generator=g)
    eps = torch.randn(N, 2, generator=g)
    ups = [torch.randn(N, 2, generator=g) for _ in range(3)]
    ne = 0.03
    ref_in = [t.clone().requires_grad_(True) for t in (feat, Wm, bm, Wv, bv)]
    mu = F.linear(ref_in[0], ref_in[1], ref_in[2])
    var = ne * torch.sigmoid(F.linear(ref_in[0], ref_in[3], ref_in[4]))
    a = mu + eps * torch.sqrt(var + 1e-6)
    (a * ups[0] + mu * ups[1] + var * ups[2]).sum().backward()
    dev_in = [t.clone().to(DEV).requires_grad_(True) for t in (feat, Wm, bm, Wv, bv)]
    a_d, mu_d, var_d = EncoderHead.apply(*dev_in, eps.to(DEV), ne)
    (a_d * ups[0].to(DEV) + mu_d * ups[1].to(DEV) + var_d * ups[2].to(DEV)).sum().backward()
    for got, want in ((a_d, a), (mu_d, mu), (var_d, var)):
        assert rel_err(got.detach().cpu(), want.detach()) < 2e-5
    for got, want in zip(dev_in, ref_in):
        assert rel_err(got.grad.cpu(), want.grad) < 2e-5

    lat = torch.randn(N, 2, generator=g)
    W, b = 0.3 * torch.randn(512, 2, generator=g), 0.1 * torch.randn(512, generator=g)
    up = torch.randn(N, 512, generator=g)
    ref_in = [t.clone().requires_grad_(True) for t in (lat, W, b)]
    (F.linear(*ref_in) * up).sum().backward()
    dev_in = [t.clone().to(DEV).requires_grad_(True) for t in (lat, W, b)]
    h = DecoderFc.apply(*dev_in)
    (h * up.to(DEV)).sum().backward()
    assert rel_err(h.detach().cpu(), F.linear(lat, W, b)) < 2e-5
    for got, want in zip(dev_in, ref_in):
        assert rel_err(got.grad.cpu(), want.grad) < 2e-5

    B, T = 3, max(N // 3, 1)
    a0, m0 = torch.randn(B, T, 2, generator=g), torch.randn(B, T, 2, generator=g)
    v0 = 0.01 + 0.05 * torch.rand(B, T, 2, generator=g)
    w = torch.randn(B, T, generator=g)
    ref_in = [t.clone().requires_grad_(True) for t in (a0, m0, v0)]
    lg = lambda x, mean, var: -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(var) - (x - mean) ** 2 / (2 * var)
    ref = (lg(ref_in[0], torch.zeros(()), torch.ones(())) - lg(*ref_in)).sum(-1)
    (ref * w).sum().backward()
    dev_in = [t.clone().to(DEV).requires_grad_(True) for t in (a0, m0, v0)]
    reg = LatentReg.apply(*dev_in)
    (reg * w.to(DEV)).sum().backward()
    assert rel_err(reg.detach().cpu(), ref.detach()) < 2e-5
    for got, want in zip(dev_in, ref_in):
        assert rel_err(got.grad.cpu(), want.grad) < 2e-5

    # scalar head of the objective
    from kvae.vae.fused import LossHead
    lpx, rg = torch.randn(B, T, generator=g) * 50, torch.randn(B, T, generator=g)
    kf = torch.randn((), generator=g)
    for mk in (None, (torch.rand(B, T, generator=g) < 0.7).float()):
        ref_in = [t.clone().requires_grad_(True) for t in (lpx, rg, kf)]
        m = torch.ones(B, T) if mk is None else mk
        denom = m.sum().clamp(min=1.0)
        recon, reg = (ref_in[0] * m).sum() / denom, (ref_in[1] * m).sum() / denom
        vae = 0.3 * recon + 0.7 * reg
        tot = 1.5 * vae + 0.8 * ref_in[2]
        (-tot * 2.0).backward()
        dev_in = [t.clone().to(DEV).requires_grad_(True) for t in (lpx, rg, kf)]
        out = LossHead.apply(dev_in[0], dev_in[1], dev_in[2], None if mk is None else mk.to(DEV), torch.tensor(0.7).to(DEV), 0.3, 1.5, 0.8)
        (out[0] * 2.0).backward()
        for got, want in zip(out, (-tot, tot, kf, vae, recon, reg)):
            assert rel_err(got.detach().cpu(), want.detach()) < 2e-5
        for got, want in zip(dev_in, ref_in):
            assert rel_err(got.grad.cpu(), want.grad) < 2e-5
        # the same through DEVICE scalars for (vae_weight, kf_weight): the by-value floats are then ignored
        dev_w = [t.clone().to(DEV).requires_grad_(True) for t in (lpx, rg, kf)]
        out_w = LossHead.apply(dev_w[0], dev_w[1], dev_w[2], None if mk is None else mk.to(DEV), torch.tensor(0.7).to(DEV), 0.3, 0.0, 0.0,
                               torch.tensor([1.5, 0.8]).to(DEV))
        (out_w[0] * 2.0).backward()
        for got, want in zip(out_w, out):
            assert torch.equal(got.detach().cpu(), want.detach().cpu())
        for got, want in zip(dev_w, dev_in):
            assert torch.equal(got.grad.cpu(), want.grad.cpu())


def colsum_pair_vs_torch(DEV):
    """_native.colsum_pair: short partials (one launch), tall partials of equal height (two launches, both tensors folded
    [64, rows/64 * cols] -> [rows/64, cols] in each) and unequal heights (two separate colsum calls) against torch's sum."""
    from kvae import _native
    g = torch.Generator().manual_seed(5)
    for ra, ca, rb, cb in [(100, 36, 100, 4), (2048, 36, 2048, 4), (1024, 288, 1024, 32), (2048, 36, 1024, 4), (1088, 7, 1088, 3),
                           (1030, 36, 1030, 4)]:
        a, b = torch.randn(ra, ca, generator=g).to(DEV), torch.randn(rb, 2, cb // 2 if cb % 2 == 0 else cb, generator=g).to(DEV)
        sa, sb = _native.colsum_pair(a, b)
        assert sa.shape == a.shape[1:] and sb.shape == b.shape[1:]
        assert rel_err(sa.cpu(), a.cpu().double().sum(0).float()) < 2e-6
        assert rel_err(sb.cpu(), b.cpu().double().sum(0).float()) < 2e-6


def dec_up_workgroup_cap(DEV):
    """kvae_dec_up_set_workgroups: fewer persistent workgroups than column sets (a stride loop with a ragged last round, fewer
    rows of weight-gradient partials) give the same block as the default; the previous value comes back and 0 restores it."""
    from kvae import _native
    lib = _native.lib_for(torch.zeros(1, device=DEV))
    default = lib.dll.kvae_dec_up_set_workgroups(7)
    try:
        assert lib.dll.kvae_dec_up_partial_rows(100, 8) == 7 and lib.dll.kvae_dec_up_partial_rows(5, 4) == 1
        dec_up_vs_torch(DEV, 100, 8)
        dec_up_vs_torch(DEV, 45, 4)
        assert lib.dll.kvae_dec_up_set_workgroups(1000) == 7   # out of range: back to the default
        assert lib.dll.kvae_dec_up_partial_rows(12800, 8) == 256
    finally:
        lib.dll.kvae_dec_up_set_workgroups(0 if default == 256 else default)


def check_phases(g, set_phase, run_step, params_now, adam_steps, value_tol=1e-4, param_tol=1e-3):
    """One implementation of the training step against the reference's three phases as recorded in phases_*.npz
    (tests/golden/make_goldens_r3.py: the reference's own set_training_phase and train_one_epoch, two steps per phase in the
    order vae -> warmup -> all, ONE Adam over all parameters).
      set_phase(phase); run_step(phase, i, kf_weight) -> dict(loss, elbo_kf, elbo_vae_total); params_now() -> {name: tensor};
      adam_steps() -> per-parameter step counts in .parameters() order."""
    buffers = ("kalman_filter.Q", "kalman_filter.R", "kalman_filter.I", "kalman_filter.mu0", "kalman_filter.Sigma0")
    names = [k[3:] for k in g if k.startswith("sd.") and k[3:] not in buffers]   # .parameters() order (the generator asserts it)
    prev = {k: v.clone() for k, v in params_now().items()}
    for phase in ("vae", "warmup", "all"):
        set_phase(phase)
        kf_w = float(g[f"{phase}.kf_weight"])
        outs = [run_step(phase, i, kf_w) for i in range(2)]
        for k in ("loss", "elbo_kf", "elbo_vae_total"):
            mean = sum(float(o[k]) for o in outs) / 2
            want = float(g[f"{phase}.mean_{k}"])
            assert abs(mean - want) <= value_tol * abs(want), (phase, k, mean, want)
        now = {k: v.clone() for k, v in params_now().items()}
        for i, k in enumerate(names):
            unchanged = bool(g[f"{phase}.unchanged"][i])
            if unchanged:   # frozen by the phase (or a zero gradient on zero moments): bit-identical, as in the reference
                assert torch.equal(now[k].cpu(), prev[k].cpu()), (phase, k, "moved but the reference left it bit-identical")
            else:
                assert not torch.equal(now[k].cpu(), prev[k].cpu()), (phase, k, "did not move")
                dn, want = float((now[k].cpu() - prev[k].cpu()).norm()), float(g[f"{phase}.delta_norm.{k}"])
                # Adam's normalised update: every entry moves by ~lr whatever its gradient, so the norm of the change is tight
                assert abs(dn - want) <= 2e-2 * want + 1e-7, (phase, k, dn, want)
            if f"{phase}.after.{k}" in g:
                # entries whose gradient is O(1e-8) are rounding-sensitive under Adam (lr*g/(|g|+eps)): 1e-3 of max|param|
                assert rel_err(now[k].cpu(), g[f"{phase}.after.{k}"]) < param_tol, (phase, k)
        prev = now
    assert [float(s) for s in adam_steps()] == [float(s) for s in g["adam_steps"]]


def rnn_wgrad_vs_torch(DEV):
    """kvae_rnn_wgrad (dW_hh | dW_ih | db of a recurrence, dW | db of a head; f32 matrix cores, split over the rows, fixed-order
    second stage) against the products torch would form: LSTM-shaped (200 x [50 | 2 | 1], h_{t-1}), both GRU directions in one
    batched call (h_{t-1} / h_{t+1} on the two halves of a [.., 2H] sequence), a head (K x [H | 1]), ragged row counts."""
    from kvae.kalman.lgssm_ops import rnn_wgrad
    g = torch.Generator().manual_seed(17)
    for Bsz, T, H, I, R in [(3, 7, 50, 2, 200), (256, 50, 50, 2, 200), (5, 1, 50, 2, 200), (2, 9, 13, 3, 37)]:
        d = torch.randn(Bsz * T, R, generator=g)
        h = torch.randn(Bsz, T, H, generator=g)
        x = torch.randn(Bsz * T, I, generator=g)
        hp = torch.cat([torch.zeros(Bsz, 1, H), h[:, :-1]], 1).reshape(Bsz * T, H)
        (gwh, gwx, gb), = rnn_wgrad(d.to(DEV), [dict(d=d.to(DEV), h=h.reshape(Bsz * T, H).to(DEV), shift=-1, T=T, x=x.to(DEV))])
        dd = d.double()
        for got, want in ((gwh, dd.t() @ hp.double()), (gwx, dd.t() @ x.double()), (gb, dd.sum(0))):
            assert rel_err(got.cpu(), want.float()) < 2e-5
    Bsz, T, H, I = 4, 11, 50, 2
    h2 = torch.randn(Bsz, T, 2 * H, generator=g)
    x = torch.randn(Bsz * T, I, generator=g)
    dpi, dph = torch.randn(2, Bsz * T, 3 * H, generator=g), torch.randn(2, Bsz * T, 3 * H, generator=g)
    zero = torch.zeros(Bsz, 1, H)
    hp = (torch.cat([zero, h2[:, :-1, :H]], 1), torch.cat([h2[:, 1:, H:], zero], 1))
    h2d = h2.reshape(Bsz * T, 2 * H).to(DEV)
    probs = []
    for dr in (0, 1):
        probs.append(dict(d=dpi[dr].to(DEV), x=x.to(DEV)))
        probs.append(dict(d=dph[dr].to(DEV), h=h2d[:, dr * H:(dr + 1) * H], shift=-1 if dr == 0 else 1, T=T))
    res = rnn_wgrad(h2d, probs)
    for dr in (0, 1):
        (_, gwx, gbi), (gwh, _, gbh) = res[2 * dr], res[2 * dr + 1]
        assert rel_err(gwx.cpu(), (dpi[dr].double().t() @ x.double()).float()) < 2e-5
        assert rel_err(gwh.cpu(), (dph[dr].double().t() @ hp[dr].reshape(Bsz * T, H).double()).float()) < 2e-5
        assert rel_err(gbi.cpu(), dpi[dr].double().sum(0).float()) < 2e-5 and rel_err(gbh.cpu(), dph[dr].double().sum(0).float()) < 2e-5
    run1 = rnn_wgrad(h2d, probs)   # fixed summation order: bit-identical from run to run
    assert all(torch.equal(a, b) for r0, r1 in zip(res, run1) for a, b in zip(r0, r1) if a is not None)


# (Bsz, T, H, I, R, shift): every k_rnn_wgrad_partial<RT> instance (RT = 1, 4, 10, 13, 16 row tiles) with a ragged last 16-row
# tile, C = H + I + 1 = 53 or 17 columns (not a multiple of 16), N = 21 / 18 / 5 rows (not a multiple of 32), h_{t-1} and h_{t+1}
# with T = 1 (every row is a sequence boundary: the hidden operand is zero everywhere), a problem without x and one without h
WGRAD_ROW_CASES = [(3, 7, 50, 2, R, -1) for R in (5, 37, 150, 200, 250)] + [
    (3, 7, 50, 2, 150, 1), (3, 7, 50, 2, 250, 1), (5, 1, 50, 2, 200, -1), (5, 1, 50, 2, 150, 1), (2, 9, 13, 3, 37, 0),
    (3, 7, 50, 0, 150, 1), (4, 11, 0, 2, 150, 0)]
# GPU tier only.  The last four: ~26000 rows are 256 chunks of 104 rows - three full 32-row stages and a partial one, the step index
# advanced by 32 % T = 32 (T = 37) and 0 (T = 32) per stage, chunk starts inside a sequence, the first and the last step masked
WGRAD_ROW_CASES_LARGE = [(256, 50, 50, 2, 200, -1), (256, 50, 50, 2, 150, 1)] + [
    (Bsz, T, 13, 3, 37, shift) for Bsz, T in ((703, 37), (813, 32)) for shift in (-1, 1)]

# Batches (a list of (Bsz, T, H, I, R, shift) per call), both tiers:
#   the product's default path (lgssm_ops.py, the coupled alpha-LSTM backward): the 200 gate rows of the LSTM with the K = 3 rows of
#     its head, so the head runs under k_rnn_wgrad_partial<13> with D columns 3 .. 207 clamped to column 2;
#   four problems with R = 5 / 60 / 150 / 250 (one, four, ten and sixteen row tiles under <16>), C = 17 (one column group) next to
#     C = 101 (two: the second group's blocks of the narrow problems have four dead wavefronts that still load) and N = 21 / 44 / 5 /
#     70 in one call (three chunks: the second and third of the N = 5 problem start at or past its end);
#   the ABI limits R = 256, C = 256.
WGRAD_BATCH_CASES = [
    [(3, 7, 50, 2, 200, -1), (3, 7, 50, 0, 3, 0)],
    [(3, 7, 13, 3, 5, -1), (4, 11, 100, 0, 60, 1), (5, 1, 13, 3, 150, 0), (10, 7, 98, 2, 250, -1)],
    [(3, 3, 200, 55, 256, 1)],
]
# (Bsz, T, H, I, R, shift, chunk cap): chunks of four or five stages, the last one partial, the second (and third) chunk starting
# inside a sequence, for every shift and T = 1, 3 (32 % T = 2), 32 (0), 33 (32), 64 (32).  The emulated tier runs them through the
# chunk-cap setter (N = 198 .. 320); the cap is the number of chunks the same shapes get on the card from N = 8192 rows on.
WGRAD_STAGE_CASES = [(Bsz, T, 13, 3, 37, shift, cap) for Bsz, T, cap in ((198, 1, 2), (66, 3, 2), (7, 32, 2), (6, 33, 2), (5, 64, 3))
                     for shift in (-1, 0, 1)]


def wgrad_instance(batch):
    """RT of the k_rnn_wgrad_partial instance a batch of (Bsz, T, H, I, R, shift) runs under (rnn_wgrad.h: wg_rt_instance)."""
    tiles = max((c[4] + 15) // 16 for c in batch)
    return next(rt for rt in (1, 4, 10, 13, 16) if tiles <= rt)


def _wgrad_problem(DEV, Bsz, T, H, I, R, shift, yardstick):
    """One problem of rnn_wgrad_per_row: (problem dict | float32 torch result, float64 reference)."""
    g = torch.Generator().manual_seed(100 * R + 10 * T + shift + 1)
    n = Bsz * T
    d = torch.randn(n, R, generator=g)
    h2 = torch.randn(Bsz, T, 2 * max(H, 1), generator=g)
    x = torch.randn(n, max(I, 1), generator=g)
    col = H if shift > 0 else 0                     # which half of the [.., 2H] sequence is the hidden operand
    h = h2[..., col:col + H]
    zero = torch.zeros(Bsz, 1, H)
    hs = {-1: torch.cat([zero, h[:, :-1]], 1), 0: h, 1: torch.cat([h[:, 1:], zero], 1)}[shift].reshape(n, H)
    dd = d.double()
    want = (dd.t() @ hs.double(), dd.t() @ x[:, :I].double(), dd.sum(0))
    if yardstick:
        return (d.t() @ hs, d.t() @ x[:, :I], d.sum(0)), want
    prob = dict(d=d.to(DEV))
    if H:
        prob.update(h=h2.reshape(n, -1).to(DEV)[:, col:col + H], shift=shift, T=T)
    if I:
        prob.update(x=x[:, :I].contiguous().to(DEV))
    return prob, want


def rnn_wgrad_batch_per_row(DEV, batch, yardstick=False):
    """kvae_rnn_wgrad on up to four problems in ONE call against the float64 products D^T [h_shifted | x | 1], one OUTPUT ROW at a
    time (a gate row of dW_hh, dW_ih and db; the floor of _per_step_ratio applies per row).  The hidden operand is a column slice
    of a wider [N, 2H] sequence when shift = +1 (the reverse GRU direction's layout: row stride 2H)."""
    from kvae.kalman.lgssm_ops import rnn_wgrad
    made = [_wgrad_problem(DEV, *c, yardstick) for c in batch]
    got = [m[0] for m in made] if yardstick else rnn_wgrad(made[0][0]["d"], [m[0] for m in made])
    out = {}
    for c, res, (_, want) in zip(batch, got, made):
        R = c[4]
        for name, a, b in zip(("wgrad.wh", "wgrad.wx", "wgrad.b"), res, want):
            if a is not None and b.numel():
                _check_steps(name, a.reshape(R, 1, -1), b.reshape(R, 1, -1), RNN_STEP_TOL[name], out)
    return out


def rnn_wgrad_per_row(DEV, Bsz, T, H, I, R, shift, yardstick=False):
    """rnn_wgrad_batch_per_row on one problem."""
    return rnn_wgrad_batch_per_row(DEV, [(Bsz, T, H, I, R, shift)], yardstick)


def rnn_wgrad_refusals(DEV):
    """One past each ABI limit: R = 257 rows, C = H + I + 1 = 257 columns, a row count that is not whole sequences - refused with an
    error code (RuntimeError from the bridge), nothing launched."""
    import pytest
    from kvae.kalman.lgssm_ops import rnn_wgrad
    for Bsz, T, H, I, R, bad_n in [(1, 3, 13, 3, 257, False), (1, 3, 200, 56, 5, False), (1, 3, 13, 3, 5, True)]:
        prob, _ = _wgrad_problem(DEV, Bsz, T, H, I, R, -1, False)
        if bad_n:
            prob["T"] = 2
        with pytest.raises(RuntimeError):
            rnn_wgrad(prob["d"], [prob])


def small_linear_vs_torch(DEV):
    """SmallLinear (+ fused softmax) forward, input gradient and parameter gradients against torch.nn.functional.linear /
    softmax autograd: the alpha head (K x 50, softmax), the regime posterior's heads (K^2 x 100 on [B,T,100], K x 100 on the
    strided rows h_seq[:, 0])."""
    from kvae.kalman.lgssm_ops import SmallLinear, small_linear_supported
    g = torch.Generator().manual_seed(23)
    for lead, F, O, softmax, strided in [((6, 9), 50, 3, True, False), ((256, 50), 50, 7, True, False), ((5, 8), 100, 9, False, False),
                                         ((3, 4), 100, 49, False, False), ((7,), 100, 7, False, True), ((2, 3), 17, 5, False, False)]:
        if strided:   # rows T*F apart, as h_seq[:, 0]
            base = torch.randn(lead[0], 6, F, generator=g)
            x_ref = base[:, 0].clone().requires_grad_(True)
            base_dev = base.to(DEV).requires_grad_(True)
            x_dev = base_dev[:, 0]
        else:
            x0 = torch.randn(*lead, F, generator=g)
            x_ref, x_dev = x0.clone().requires_grad_(True), x0.to(DEV).requires_grad_(True)
        w0, b0 = torch.randn(O, F, generator=g) * 0.3, torch.randn(O, generator=g)
        up = torch.randn(*lead, O, generator=g)
        w_ref, b_ref = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y_ref = torch.nn.functional.linear(x_ref, w_ref, b_ref)
        if softmax:
            y_ref = torch.softmax(y_ref, -1)
        (y_ref * up).sum().backward()
        w_dev, b_dev = w0.to(DEV).requires_grad_(True), b0.to(DEV).requires_grad_(True)
        assert small_linear_supported(x_dev, w_dev, softmax)
        y = SmallLinear.apply(x_dev, w_dev, b_dev, softmax)
        (y * up.to(DEV)).sum().backward()
        assert rel_err(y.detach().cpu(), y_ref.detach()) < 1e-5
        gx = base_dev.grad[:, 0] if strided else x_dev.grad
        assert rel_err(gx.cpu(), x_ref.grad) < 2e-5
        assert rel_err(w_dev.grad.cpu(), w_ref.grad) < 2e-5 and rel_err(b_dev.grad.cpu(), b_ref.grad) < 2e-5


def backward_shard_vs_slices(DEV, B, T, n, slice_b):
    """The LGSSM forward + ELBO + backward on B sequences in one launch against the same on B / slice_b launches of slice_b
    sequences each: per-sequence gradients (Y, U, alpha) bit-identical; the summed base-matrix gradients (A, B, C: reduced over
    the batch in a different grouping) to rounding.  Runs under no host-side oracle: the slices ARE the oracle-checked size."""
    from kvae.kalman.lgssm_ops import LgssmElbo, LgssmSmooth, Slots, mix_dynamics
    A, Bm, Cm, alpha, Y, U, mask, eps = _random_problem(B, T, n, n, 2, 3, 100 + B + T, DEV)
    R, Q = 0.03 * torch.eye(2, device=DEV), 0.02 * torch.eye(n, device=DEV)
    mu0, S0 = torch.zeros(n, device=DEV), 20.0 * torch.eye(n, device=DEV)

    def run(sl):
        leaves = [t.clone().requires_grad_(True) for t in (A, Bm, Cm, alpha[sl], Y[sl], U[sl])]
        rec, offs, _ = mix_dynamics(leaves[3], leaves[:3])
        slots = Slots(A=offs[0], B=offs[1], C=offs[2])
        mk = None if mask is None else mask[sl]
        ms, Ss, *_ = LgssmSmooth.apply(leaves[4], leaves[5], mk, rec, None, None, None, Q, R, mu0, S0, slots, True)
        total, _, _ = LgssmElbo.apply(ms, Ss, eps[sl], leaves[4], leaves[5], mk, rec, None, None, None, Q, R, mu0, S0, slots)
        total.backward()
        return [t.grad for t in leaves], rec.detach(), ms.detach()

    big, rec_big, ms_big = run(slice(0, B))
    assert all(torch.isfinite(g).all() for g in big)
    acc = [torch.zeros_like(g) for g in big[:3]]
    for b0 in range(0, B, slice_b):
        sl = slice(b0, b0 + slice_b)
        small, _, ms_small = run(sl)
        assert torch.equal(ms_small, ms_big[sl])
        for k, name in ((3, "alpha"), (4, "Y"), (5, "U")):
            assert torch.equal(small[k], big[k][sl]), (name, b0)
        for k in range(3):
            acc[k] += small[k]
    for k, name in enumerate("ABC"):
        assert rel_err(acc[k].cpu(), big[k].cpu()) < 1e-4, name


def mix_vs_torch(DEV):
    """kvae_mix_fwd / kvae_mix_bwd (mixture-of-K step records, reference dyn_param.py:58-60 / switch_dyn_param.py:82-84) against
    torch.einsum and its autograd: the streaming kernels' shapes (E = 40 / 48 at n = 4, 544 / 768 at n = 16, K = 3, 7, 8), ragged row
    counts, a K above their limit (element-wise fallback), and the accumulate flag of the C ABI."""
    import ctypes as C
    from kvae import _native as N
    from kvae.kalman.lgssm_ops import MixDynamics
    g = torch.Generator().manual_seed(31)
    for Bsz, T, K, E in [(256, 50, 3, 40), (3, 7, 3, 48), (32, 100, 7, 48), (5, 9, 3, 768), (64, 33, 3, 544), (2, 5, 8, 768),
                         (4, 6, 9, 40), (1, 1, 2, 12), (2, 3, 3, 42)]:
        alpha = torch.softmax(torch.randn(Bsz, T, K, generator=g), -1)
        base = torch.randn(K, E, generator=g)
        up = torch.randn(Bsz, T, E, generator=g)
        ar, br = alpha.clone().requires_grad_(True), base.clone().requires_grad_(True)
        ref = torch.einsum("btk,ke->bte", ar, br)
        (ref * up).sum().backward()
        ad, bd = alpha.to(DEV).requires_grad_(True), base.to(DEV).requires_grad_(True)
        out = MixDynamics.apply(ad, bd)
        (out * up.to(DEV)).sum().backward()
        assert rel_err(out.detach().cpu(), ref.detach()) < 1e-6, (K, E)
        assert rel_err(ad.grad.cpu(), ar.grad) < 2e-5 and rel_err(bd.grad.cpu(), br.grad) < 2e-5, (K, E)
    # accumulate_alpha = 1 through the raw C ABI: g_alpha += ...
    Bsz, T, K, E = 7, 5, 3, 768
    alpha = torch.softmax(torch.randn(Bsz * T, K, generator=g), -1).to(DEV)
    base, gout = torch.randn(K, E, generator=g).to(DEV), torch.randn(Bsz * T, E, generator=g).to(DEV)
    lib = N.lib_for(alpha)
    nblk = lib.dll.kvae_mix_bwd_partials(Bsz * T)
    partials = torch.empty(nblk, K, E, device=alpha.device)
    g_alpha0 = torch.randn(Bsz * T, K, generator=g).to(DEV)
    g_alpha, g_base = g_alpha0.clone(), torch.empty_like(base)
    assert lib.dll.kvae_mix_bwd(N.ptr(alpha), N.ptr(base), N.ptr(gout), N.ptr(g_alpha), N.ptr(g_base), N.ptr(partials), Bsz * T, K, E,
                                1, N.stream_for(alpha)) == 0
    assert rel_err((g_alpha - g_alpha0).cpu(), (gout @ base.T).cpu()) < 2e-5
    assert rel_err(g_base.cpu(), (alpha.T @ gout).cpu()) < 2e-5


# (Bsz, T, K, E): the streaming kernels' widths with row counts that are not a multiple of the 16 rows per block of the second
# stage (21, 37, 17, 45) and K below the instance's KMAX (2, 5, 6), a K above their limit, and the large cases of mix_vs_torch
MIX_ROW_CASES = [(3, 7, 3, 48), (3, 7, 2, 40), (37, 1, 5, 768), (1, 17, 6, 48), (5, 9, 3, 768), (2, 5, 8, 768), (4, 6, 9, 40),
                 (1, 1, 2, 12), (2, 3, 3, 42), (3, 7, 7, 544)]
# GPU tier only.  The last one: 33000 rows are above 32768, where both slab caps bind (forward 4096 slabs of 9 rows; backward 2048
# slabs of 17 rows - more than the 16 the partials buffer allows below that, and not a multiple of the four rows of an RB group)
MIX_ROW_CASES_LARGE = [(256, 50, 3, 40), (32, 100, 7, 48), (64, 33, 3, 544), (33, 1000, 2, 128)]
# both tiers: one row; 1041 rows = 66 slabs of 16 rows (k_mix_bwd_fold takes a second round of 64 slabs, the last slab holds one row)
MIX_ROW_CASES_EDGE = [(1, 1, 3, 128), (1, 1041, 2, 128)]
# (Bsz, T, K, E, forward slab cap, backward slab cap) for the emulated tier's setters: 37 rows in 2 slabs of 19 rows, 75 rows in 3
# slabs of 25 (more than 16 rows per slab, not a multiple of 4: the last RB group of every slab is ragged), K above 4 once
MIX_CAPPED_CASES = [(37, 1, 2, 128, 2, 2), (3, 25, 5, 260, 3, 3)]


def mix_instance(K, E):
    """(KMAX, EJ) of the streaming instance (mix_wave.h: KVAE_MIXW_DISPATCH), or None where the gate sends the call to the
    element-wise kernels (pointers of torch allocations are 16-byte aligned)."""
    if E % 4 or E < 128 or E > 768 or K > 8:
        return None
    return (4 if K <= 4 else 8, (E + 255) // 256)


def mix_per_row(DEV, Bsz, T, K, E, yardstick=False):
    """kvae_mix_fwd / kvae_mix_bwd against the float64 products: the mixed records and g_alpha per (b,t) row, g_base per mode."""
    from kvae.kalman.lgssm_ops import MixDynamics
    g = torch.Generator().manual_seed(1000 * K + E + Bsz * T)
    alpha = torch.softmax(torch.randn(Bsz, T, K, generator=g), -1)
    base, up = torch.randn(K, E, generator=g), torch.randn(Bsz, T, E, generator=g)
    a64, b64, u64 = alpha.double(), base.double(), up.double()
    want = (torch.einsum("btk,ke->bte", a64, b64), torch.einsum("bte,ke->btk", u64, b64), torch.einsum("btk,bte->ke", a64, u64))
    if yardstick:
        got = (torch.einsum("btk,ke->bte", alpha, base), torch.einsum("bte,ke->btk", up, base), torch.einsum("btk,bte->ke", alpha, up))
    else:
        ad, bd = alpha.to(DEV).requires_grad_(True), base.to(DEV).requires_grad_(True)
        o = MixDynamics.apply(ad, bd)
        (o * up.to(DEV)).sum().backward()
        got = (o, ad.grad, bd.grad)
    out = {}
    _check_steps("mix.out", got[0], want[0], RNN_STEP_TOL["mix.out"], out)
    _check_steps("mix.g_alpha", got[1], want[1], RNN_STEP_TOL["mix.g_alpha"], out)
    _check_steps("mix.g_base", got[2][:, None], want[2][:, None], RNN_STEP_TOL["mix.g_base"], out)
    return out


def mix_accumulate_guarded(DEV, rows, K, E, misalign=None):
    """kvae_mix_bwd through the C ABI with accumulate_alpha = 1 and then 0, g_alpha / g_base / partials in guarded buffers of exactly
    the sizes the ABI states (partials: kvae_mix_bwd_partials(rows) x K x E): g_alpha += on the first call, overwritten on the
    second, per row against float64; no guard element written.  misalign = "partials" / "g_out" puts that buffer 4 bytes past a
    16-byte boundary: the gate then sends the call to the element-wise kernels, same results."""
    from kvae import _native as N
    from step_cases import Guarded
    g = torch.Generator().manual_seed(7 * rows + K + E)
    alpha = torch.softmax(torch.randn(rows, K, generator=g), -1)
    base, gout, ga0 = torch.randn(K, E, generator=g), torch.randn(rows, E, generator=g), torch.randn(rows, K, generator=g)
    al, bs = Guarded(DEV, rows * K, init=alpha), Guarded(DEV, K * E, init=base)
    go = Guarded(DEV, rows * E, off=1 if misalign == "g_out" else 0, init=gout)
    lib = N.lib_for(al.t)
    part = Guarded(DEV, lib.dll.kvae_mix_bwd_partials(rows) * K * E, off=1 if misalign == "partials" else 0)
    g_alpha, g_base = Guarded(DEV, rows * K, init=ga0), Guarded(DEV, K * E)
    want_a, want_b = gout.double() @ base.double().T, alpha.double().T @ gout.double()
    out = {}
    for acc in (1, 0):
        rc = lib.dll.kvae_mix_bwd(al.ptr, bs.ptr, go.ptr, g_alpha.ptr, g_base.ptr, part.ptr, rows, K, E, acc, N.stream_for(al.t))
        assert rc == 0, rc
        got_a = g_alpha.cpu().view(rows, K).double() - (ga0.double() if acc else 0.0)
        _check_steps("mix.g_alpha", got_a.view(1, rows, K), want_a.view(1, rows, K), RNN_STEP_TOL["mix.g_alpha"], out)
        _check_steps("mix.g_base", g_base.cpu().view(K, 1, E), want_b.view(K, 1, E), RNN_STEP_TOL["mix.g_base"], out)
        for name, buf in (("alpha", al), ("base", bs), ("g_out", go), ("g_alpha", g_alpha), ("g_base", g_base), ("partials", part)):
            assert buf.guards_intact(), (name, "guard written", acc)
    return out


# (leading shape, F, O, softmax, strided): the heads of small_linear_vs_torch, single rows, and a row count of one
LINEAR_ROW_CASES = [((6, 9), 50, 3, True, False), ((5, 8), 100, 9, False, False), ((3, 4), 100, 49, False, False),
                    ((7,), 100, 7, False, True), ((2, 3), 17, 5, False, False), ((1, 1), 50, 7, True, False),
                    ((3,), 100, 16, True, True)]
# GPU tier only.  The last two: 16500 >= 16384 rows take 64 rows per block (u up to 15 in sl_stage_rows), the last block has 52
LINEAR_ROW_CASES_LARGE = [((256, 50), 50, 7, True, False), ((256, 50), 100, 49, False, False), ((16500,), 17, 5, False, False),
                          ((33, 500), 50, 7, True, False)]
# both tiers: F = 128 with the largest O that fits SL_MAX_W (96 x 129 floats of W leave room for 16 rows), the softmax at O = 1
# and at its limit O = 16, O = 5 (not a multiple of the 4 outputs per thread) on strided rows, one block
LINEAR_ROW_CASES_EDGE = [((5,), 128, 96, False, False), ((3,), 50, 1, True, False), ((21,), 50, 16, True, False),
                         ((13,), 17, 5, False, True)]
# (leading shape, F, O, softmax, strided, least block count, rows per block it gives) for the emulated tier's setter: 70 rows at
# 64 (2 blocks, 6 rows in the last), 32 (3 blocks) and 16 (5 blocks) rows per block; 40 rows in ONE block of 64
LINEAR_BLOCK_CASES = [((70,), 17, 5, False, False, 1, 64), ((70,), 17, 5, False, False, 2, 32), ((70,), 17, 5, False, False, -1, 16),
                      ((70,), 50, 7, True, True, 1, 64), ((70,), 50, 7, True, False, 2, 32), ((40,), 17, 5, False, True, 0, 64)]


def small_linear_per_row(DEV, lead, F, O, softmax, strided, yardstick=False):
    """SmallLinear (+ fused softmax) against float64 torch: y and dx one input row at a time, dW one output row at a time, db."""
    from kvae.kalman.lgssm_ops import SmallLinear
    g = torch.Generator().manual_seed(100 * F + O + len(lead))
    base = torch.randn(*lead, 6, F, generator=g)      # strided: rows 6 F apart, as h_seq[:, 0]
    x0 = base.select(-2, 0)
    w0, b0, up = torch.randn(O, F, generator=g) * 0.3, torch.randn(O, generator=g), torch.randn(*lead, O, generator=g)

    def run(dtype, dev, kernel):
        bs = base.to(dtype).to(dev).requires_grad_(True)
        x = bs.select(-2, 0) if strided else bs.select(-2, 0).contiguous()
        w, b = w0.to(dtype).to(dev).requires_grad_(True), b0.to(dtype).to(dev).requires_grad_(True)
        if kernel:
            y = SmallLinear.apply(x, w, b, softmax)
        else:
            y = torch.nn.functional.linear(x, w, b)
            y = torch.softmax(y, -1) if softmax else y
        (y * up.to(dtype).to(dev)).sum().backward()
        return y.detach().reshape(-1, 1, O), bs.grad.select(-2, 0).reshape(-1, 1, F), w.grad[:, None], b.grad[None, None]

    want = run(torch.float64, "cpu", False)
    got = run(torch.float32, "cpu", False) if yardstick else run(torch.float32, DEV, True)
    out = {}
    for name, a, b in zip(("linear.y", "linear.dx", "linear.dw", "linear.db"), got, want):
        _check_steps(name, a, b, RNN_STEP_TOL[name], out)
    return out


# ---- frame-VAE kernels (vae_conv_edge.h, vae_conv_mid.h, vae_conv_up_wino.h / vae_conv_up.h, vae_heads.h, vae_loss.h), one
# (frame, channel) plane / one row at a time against float64 ----
# Bars = 4 x VAE_YARDSTICK, the rule of RNN_STEP_TOL.  The yardstick of a quantity is the largest ratio of FLOAT32 TORCH ON THE CPU
# (F.conv2d, F.pixel_shuffle, F.linear, ... run in float32 on the same inputs) against the float64 reference, over every case of both
# tiers with at most 4099 frames (VAE_SMALL_CASES, VAE_RESIDUE_N, VAE_GRID_CASES, VAE_SCALE_CASES, the probes, VAE_HEADS_N,
# VAE_BCE_CASES; rerun: the case functions with yardstick=True).  Ratios of the plain-loop twins and what is still unmeasured: DESIGN section 2.
# `x`: per (frame, channel) plane / per row (_per_step_ratio); `x.whole`: the tensor as a whole (rel_err).
VAE_LAYERS = {   # layer: (input channels, conv output channels, stride, PixelShuffle factor, ReLU, weight scale, bias scale)
    "stem": (1, 32, 2, 1, True, 0.3, 0.1), "enc_mid": (32, 32, 2, 1, True, 0.08, 0.1),
    "dec_up": (32, 128, 1, 2, True, 0.08, 0.1), "dec_head": (32, 4, 1, 2, False, 0.1, 1.0)}
VAE_SIDES = {"stem": (32,), "enc_mid": (16, 8), "dec_up": (8, 4), "dec_head": (16,)}
VAE_NEAR = 1e-5         # |float64 pre-activation| <= VAE_NEAR x frame scale: the ReLU mask is rounding's choice, no upstream gradient there
VAE_NEAR_SHARE = 1e-4   # ... and at most this share of a case's pixels may be left out that way
VAE_YARDSTICK = {   # float32 torch on the CPU against float64, largest ratio over the cases of both tiers with N <= 4099
    "stem.out": 3.45e-06, "stem.out.whole": 1.75e-07, "stem.dw": 1.14e-05, "stem.dw.whole": 3.80e-06, "stem.db": 4.28e-06,
    "enc_mid.out": 1.69e-05, "enc_mid.out.whole": 4.82e-07, "enc_mid.dx": 6.13e-07, "enc_mid.dx.whole": 3.55e-07,
    "enc_mid.dw": 3.27e-06, "enc_mid.dw.whole": 7.72e-07, "enc_mid.db": 1.62e-06,
    "dec_up.out": 1.73e-06, "dec_up.out.whole": 4.40e-07, "dec_up.dx": 1.04e-06, "dec_up.dx.whole": 3.07e-07,
    "dec_up.dw": 4.81e-06, "dec_up.dw.whole": 1.16e-06, "dec_up.db": 4.62e-06,
    "dec_head.out": 6.29e-07, "dec_head.out.whole": 4.50e-07, "dec_head.dx": 6.02e-07, "dec_head.dx.whole": 3.18e-07,
    "dec_head.dw": 8.86e-06, "dec_head.dw.whole": 2.21e-06, "dec_head.db": 4.81e-06,
    "enc_head.a": 2.40e-05, "enc_head.mu": 7.23e-06, "enc_head.var": 7.08e-07, "enc_head.dfeat": 1.94e-07, "enc_head.param": 7.12e-07,
    "dec_fc.h": 1.62e-07, "dec_fc.da": 1.44e-05, "dec_fc.dw": 1.16e-05, "dec_fc.db": 1.41e-07,
    "latent_reg.reg": 3.18e-07, "latent_reg.da": 1.95e-07, "latent_reg.dmu": 1.49e-07, "latent_reg.dvar": 2.68e-07,
    "bce.ll": 1.66e-07, "bce.dlogits": 1.43e-07,
}
VAE_STEP_TOL = {k: 4.0 * v for k, v in VAE_YARDSTICK.items()}


def _conv_ref64(x, W, b, stride, shuffle, relu):
    """(out, pre-activation) of act(pixel_shuffle(conv3x3(x, W, padding 1, stride) + b)) WITHOUT torch's convolution: zero-pad, nine
    shifted (strided) slices, one einsum over the input channels per tap; frames in slices of at most 4096.  Gradients: autograd."""
    pres = []
    for lo in range(0, x.shape[0], 4096):
        xs = x[lo:lo + 4096]
        n, ci, H, Wd = xs.shape
        xp = xs.new_zeros(n, ci, H + 2, Wd + 2)
        xp[:, :, 1:H + 1, 1:Wd + 1] = xs
        Ho, Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
        acc = b.view(1, -1, 1, 1).expand(n, W.shape[0], Ho, Wo)
        for ky in range(3):
            for kx in range(3):
                tap = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
                acc = acc + torch.einsum("nchw,oc->nohw", tap, W[:, :, ky, kx])
        pres.append(acc)
    pre = torch.cat(pres)
    if shuffle > 1:   # PixelShuffle: channel c r^2 + i r + j at (h, w) -> channel c at (h r + i, w r + j)
        n, c, H, Wd = pre.shape
        pre = pre.view(n, c // shuffle ** 2, shuffle, shuffle, H, Wd).permute(0, 1, 4, 2, 5, 3).reshape(
            n, c // shuffle ** 2, H * shuffle, Wd * shuffle)
    return (torch.relu(pre) if relu else pre), pre


def _conv_torch(x, W, b, stride, shuffle, relu):
    """The same layer through torch's own convolution, in the dtype of its arguments (the float32 yardstick; float64: the pin of
    _conv_ref64)."""
    import torch.nn.functional as F
    pre = F.conv2d(x, W, b, stride=stride, padding=1)
    pre = F.pixel_shuffle(pre, shuffle) if shuffle > 1 else pre
    return (torch.relu(pre) if relu else pre), pre


def _vae_fn(layer):
    from kvae.vae import fused
    return {"stem": fused.EncoderStem, "enc_mid": fused.EncoderMid, "dec_up": fused.DecoderUp, "dec_head": fused.DecoderHead}[layer]


def _frame_sample(N, chunk=16384, seed=0):
    """The frames of a large case that go to the host: the first one, the last 17 (the ragged tail and both sides of the last full
    iteration / column set of every kernel: at most 8 frames each), both sides of every launch boundary, 256 seeded random ones."""
    s = {0} | set(range(max(N - 17, 0), N))
    for k in range(chunk, N, chunk):
        s.update((k - 1, k))
    s.update(torch.randint(0, N, (256,), generator=torch.Generator().manual_seed(seed)).tolist())
    return torch.tensor(sorted(s))


def _vae_inputs(layer, N, side, seed, gdev, scales):
    """x [N,cin,side,side] on `gdev` (float32, non-negative like the activations the layers see, frame i scaled by
    (1e-3, 1, 1e+2)[i % 3] with `scales`), the frame scales [N] (host), W, b (host, float32)."""
    cin, cout, _, _, _, ws, bs = VAE_LAYERS[layer]
    g = torch.Generator(device=gdev).manual_seed(7919 * seed + 31 * N + side)
    x = torch.rand(N, cin, side, side, generator=g, device=gdev) if layer == "stem" else \
        torch.relu(torch.randn(N, cin, side, side, generator=g, device=gdev))
    s = torch.ones(N)
    if scales:
        s = torch.tensor([1e-3, 1.0, 1e2])[torch.arange(N) % 3]
        x = x * s.to(gdev).view(-1, 1, 1, 1)
    gh = torch.Generator().manual_seed(104729 * seed + 17 * N + side)
    return x, s, ws * torch.randn(cout, cin, 3, 3, generator=gh), bs * torch.randn(cout, generator=gh), gh


def _vae_compare(layer, got, want, out, S=None):
    """got = (out, g_x or None, g_W, g_b) of the kernels (frames S of out / g_x), want = the float64 ones."""
    tol = lambda k: VAE_STEP_TOL[f"{layer}.{k}"]
    sel = (lambda t: t.detach()[S.to(t.device)].cpu()) if S is not None else (lambda t: t.detach().cpu())
    for k, a, r, cut in (("out", got[0], want[0], True), ("dx", got[1], want[1], True), ("dw", got[2], want[2], False)):
        if r is None:
            assert a is None
            continue
        a = sel(a) if cut else a.detach().cpu()
        _check_steps(f"{layer}.{k}", a, r, tol(k), out)
        _check_whole(f"{layer}.{k}.whole", a, r, tol(k + ".whole"), out)
    _check_whole(f"{layer}.db", got[3], want[3], tol("db"), out)


def _vae_reference(layer, xs, scale_s, W, b, up_of):
    """Float64 run on the frames xs (float32 values).  up_of(near) -> the upstream gradient (float32) given the near-threshold
    mask.  Returns (out64, g_x64 or None, g_W64, g_b64), up, near, share."""
    _, _, stride, shuf, relu, _, _ = VAE_LAYERS[layer]
    xr = xs.double().requires_grad_(layer != "stem")
    Wr, br = W.double().requires_grad_(True), b.double().requires_grad_(True)
    out64, pre64 = _conv_ref64(xr, Wr, br, stride, shuf, relu)
    near = (pre64.detach().abs() <= VAE_NEAR * scale_s.double().view(-1, 1, 1, 1)) if relu else torch.zeros_like(pre64, dtype=torch.bool)
    up = up_of(near)
    out64.backward(up.double())
    return (out64.detach(), xr.grad, Wr.grad, br.grad), up, near


def _vae_kernels(DEV, layer, x, W, b, up, want_dx=True):
    """The fused Function on float32 operands already on DEV."""
    xd = x.requires_grad_(layer != "stem" and want_dx)
    Wd, bd = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = _vae_fn(layer).apply(xd, Wd, bd)
    out.backward(up)
    return out.detach(), xd.grad, Wd.grad, bd.grad


def _vae_check_mask(out, out64, near, S=None):
    """Outside the near-threshold pixels the kernel's ReLU mask IS the reference's: a difference is a failure."""
    got = out.detach()[S.to(out.device)].cpu() if S is not None else out.detach().cpu()
    diff = ((got > 0) != (out64 > 0)) & ~near
    assert not bool(diff.any()), ("ReLU mask differs from float64 away from the threshold", int(diff.sum()), diff.nonzero()[:4].tolist())


def conv_layer_per_frame(DEV, layer, N, side, frames=None, seed=0, yardstick=False, scales=False):
    """One convolution layer of the frame VAE (`layer` in VAE_LAYERS, through its kvae.vae.fused Function) against _conv_ref64:
    the output and the data gradient per (frame, channel) plane, the weight gradient per (output channel, input channel), the bias
    gradient as a whole; out / dx / dW also as whole tensors at bars of their own (a plane at the 1e-2 floor of _per_step_ratio turns
    1e-7 of the tensor's maximum into 1e-5, so only the whole-tensor bar holds the full-scale values to float32's own accuracy).
    ReLU: the upstream gradient is zero where the float64 pre-activation is within VAE_NEAR x frame scale of 0 - at most
    VAE_NEAR_SHARE of the pixels, asserted; a case of a few frames whose first draw has more (one pixel of 2048 is 5e-4) redraws its
    inputs, which depends on the float64 reference alone - and everywhere else the kernel's mask must equal the reference's.
    `frames` (given, or N > 4099): x is drawn on the device, only the frames of _frame_sample reach the host; out and dx are compared
    on them, the upstream gradient is non-zero ONLY on them - so the float64 weight / bias gradient needs no other frame, a frame the
    kernel drops or reads from elsewhere is a whole term of it, and dx of every other frame must be exactly zero (checked on the
    device over the whole tensor).  yardstick: float32 torch on the CPU in place of the kernels.  Returns the largest ratios."""
    _, _, stride, shuf, relu, _, _ = VAE_LAYERS[layer]
    assert side in VAE_SIDES[layer]
    if frames is None and N > 4099:
        frames = _frame_sample(N, getattr(_vae_fn(layer), "CHUNK", 16384), seed)
    sampled = frames is not None
    assert not (sampled and yardstick)
    gdev = DEV if sampled else "cpu"
    for draw in range(8):
        x, s, W, b, gh = _vae_inputs(layer, N, side, seed + 1000 * draw, gdev, scales)
        S = frames if sampled else torch.arange(N)
        xs = x[S.to(x.device)].cpu()
        want, up_s, near = _vae_reference(layer, xs, s[S], W, b, lambda near: torch.randn(near.shape, generator=gh) * ~near)
        share = float(near.double().mean())
        if share <= VAE_NEAR_SHARE:
            break
    assert share <= VAE_NEAR_SHARE, ("too many pixels at the ReLU threshold", share)
    res = {}
    if yardstick:
        xr = xs.clone().requires_grad_(layer != "stem")
        Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out, _ = _conv_torch(xr, Wr, br, stride, shuf, relu)
        out.backward(up_s)
        got = (out.detach(), xr.grad, Wr.grad, br.grad)
    else:
        if sampled:
            up = torch.zeros(N, *up_s.shape[1:], device=DEV)
            up[S.to(DEV)] = up_s.to(DEV)
        else:
            up = up_s.to(DEV)
        got = _vae_kernels(DEV, layer, x.to(DEV), W, b, up)
        del up
        if sampled and got[1] is not None:
            other = got[1].abs().amax(dim=(1, 2, 3))
            other[S.to(DEV)] = 0.0
            assert float(other.max()) == 0.0, ("dx of a frame without upstream gradient", int(other.argmax()))
    if relu:
        _vae_check_mask(got[0], want[0], near, S if (sampled and not yardstick) else None)
    _vae_compare(layer, got, want, res, S if (sampled and not yardstick) else None)
    res["near_share"] = share
    return res


def _probe_positions(n):
    """Four corners, one pixel of each edge, one interior pixel of an n x n grid (n >= 4)."""
    h = n // 2
    return [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (0, h), (n - 1, h), (h, 0), (h, n - 1), (1, h)]


def probe_frames(layer, side):
    """(N, frames): the first and the last frame of an iteration / column set and the last frame of a ragged one, for every kernel
    of the layer (frames per iteration: enc_mid 2 | 8; dec_up Winograd 1 | 4, direct 2 | 8; edge layers one frame per workgroup)."""
    return {("stem", 32): (3, (0, 2)), ("dec_head", 16): (3, (0, 2)), ("enc_mid", 16): (3, (0, 1, 2)), ("enc_mid", 8): (13, (0, 7, 12)),
            ("dec_up", 8): (3, (0, 1, 2)), ("dec_up", 4): (13, (0, 3, 7, 12))}[(layer, side)]


def conv_probe(DEV, layer, side, kind, frame, pos, N=None, seed=0, yardstick=False):
    """Structured inputs.  kind "upstream": dense frames, the upstream gradient on ONE output pixel `pos` of ONE frame (all channels):
    the data gradient must match float64 inside that pixel's receptive field and be EXACTLY zero everywhere else, other frames
    included; weight and bias gradients are that frame's term alone.  kind "input": every frame zero except the input pixel `pos` of
    one frame (all channels): every other frame's output must be act(bias), broadcast, exactly (a zero patch gives a zero Winograd
    product), the frame itself matches float64; dense upstream gradient."""
    _, cout, stride, shuf, relu, _, _ = VAE_LAYERS[layer]
    N = N or probe_frames(layer, side)[0]
    x, s, W, b, gh = _vae_inputs(layer, N, side, seed + 50, "cpu", False)
    so = ((side - 1) // stride + 1) * shuf
    py, px = pos
    if kind == "input":
        imp = x[frame, :, py, px].clone() + 0.25
        x = torch.zeros_like(x)
        x[frame, :, py, px] = imp

    def up_of(near):
        up = torch.randn(near.shape, generator=gh)
        if kind == "upstream":
            keep = torch.zeros_like(near)
            keep[frame, :, py, px] = True
            up = up * keep
        return up * ~near
    want, up, near = _vae_reference(layer, x, s, W, b, up_of)
    if yardstick:
        xr = x.clone().requires_grad_(layer != "stem")
        Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out, _ = _conv_torch(xr, Wr, br, stride, shuf, relu)
        out.backward(up)
        got = (out.detach(), xr.grad, Wr.grad, br.grad)
    else:
        got = _vae_kernels(DEV, layer, x.to(DEV), W, b, up.to(DEV))
    res = {}
    if relu:
        _vae_check_mask(got[0], want[0], near)
    _vae_compare(layer, got, want, res)
    if kind == "upstream" and got[1] is not None:
        cy, cx = py // shuf, px // shuf
        field = torch.zeros(N, 1, side, side, dtype=torch.bool)
        field[frame, 0, max(stride * cy - 1, 0):stride * cy + 2, max(stride * cx - 1, 0):stride * cx + 2] = True
        outside = ~field.expand(N, x.shape[1], side, side)
        assert float(want[1][outside].abs().max()) == 0.0   # the geometry above is the reference's
        leak = got[1].detach().cpu()[outside]
        assert float(leak.abs().max()) == 0.0, ("data gradient outside the receptive field", float(leak.abs().max()))
    if kind == "input" and not yardstick:
        flat = b.view(1, -1, 1, 1).expand(1, cout, so // shuf, so // shuf)
        flat = torch.nn.functional.pixel_shuffle(flat, shuf) if shuf > 1 else flat
        flat = torch.relu(flat) if relu else flat
        others = [i for i in range(N) if i != frame]
        if others:
            o = got[0].detach().cpu()[others]
            assert torch.equal(o, flat.expand_as(o).contiguous()), "a frame of zeros does not give act(bias) exactly"
    return res


def conv_no_input_grad(DEV, layer, N, side):
    """needs_input_grad[0] == False (the `g_x is None` branch of the backward): the same weight and bias gradients, bit for bit."""
    x, s, W, b, gh = _vae_inputs(layer, N, side, 3, "cpu", False)
    _, _, stride, shuf, _, _, _ = VAE_LAYERS[layer]
    so = ((side - 1) // stride + 1) * shuf
    up = torch.randn(N, VAE_LAYERS[layer][1] // shuf ** 2, so, so, generator=gh).to(DEV)
    with_dx = _vae_kernels(DEV, layer, x.clone().to(DEV), W, b, up, want_dx=True)
    without = _vae_kernels(DEV, layer, x.clone().to(DEV), W, b, up, want_dx=False)
    assert with_dx[1] is not None and without[1] is None
    assert torch.equal(with_dx[0], without[0]) and torch.equal(with_dx[2], without[2]) and torch.equal(with_dx[3], without[3])


def _iters_cases(fpis):
    """Frame counts that give 255, 256, 257 and 513 iterations / column sets (the last one ragged) of kernels with `fpis` frames each."""
    return sorted({(it - 1) * f + 1 for f in fpis for it in (255, 256, 257, 513)})


# (layer, side, N): every residue of every kernel's frames per iteration (N = 1 ... 17), and the persistent grids (256 workgroups
# for enc_mid / dec_up, 1024 weight-gradient rows for the edge layers) one short, full, one over and past two rounds
VAE_RESIDUE_N = list(range(1, 18))
VAE_GRID_CASES = ([("enc_mid", 16, n) for n in _iters_cases((2,))] + [("enc_mid", 8, n) for n in _iters_cases((8,))] +
                  [("dec_up", 8, n) for n in _iters_cases((1, 2))] + [("dec_up", 4, n) for n in _iters_cases((4, 8))] +
                  [(l, sd, n) for l, sd in (("stem", 32), ("dec_head", 16)) for n in (1023, 1024, 1025, 2049)])
VAE_LAYER_SIDES = [(l, sd) for l in VAE_LAYERS for sd in VAE_SIDES[l]]
VAE_CHUNK_N = (16383, 16384, 16385, 20000)
VAE_C5_N = 512 * 200
# CPU tier (plain-loop twins): residues, and sampled cases of a few frames (CHUNK patched down to 16 there: three launches)
VAE_SMALL_CASES = [(l, sd, n) for l, sd in VAE_LAYER_SIDES for n in (1, 2, 3, 5, 8, 9, 13, 17)] + [("enc_mid", 8, 64), ("dec_up", 4, 64)]


def _rows(t):
    return t.detach().cpu().reshape(t.shape[0], 1, -1)


def _row_sample(N, seed=0):
    return _frame_sample(N, 1 << 40, seed)


def vae_heads_per_row(DEV, N, rows=None, seed=0, yardstick=False):
    """EncoderHead (+ reparameterisation), DecoderFc and LatentReg against the float64 form of the torch expressions of
    vae_heads_vs_torch: every output and every per-row gradient one row at a time, parameter gradients as whole tensors.  `rows`
    (given, or N > 4099): inputs drawn on the device, the rows of _row_sample compared, upstream gradients non-zero on them alone and
    the per-row gradients of every other row exactly zero."""
    import torch.nn.functional as F
    from kvae.vae.fused import DecoderFc, EncoderHead, LatentReg
    if rows is None and N > 4099:
        rows = _row_sample(N, seed)
    sampled = rows is not None
    assert not (sampled and yardstick)
    gdev = DEV if sampled else "cpu"
    S = rows if sampled else torch.arange(N)
    g = torch.Generator(device=gdev).manual_seed(11 * N + seed)
    gh = torch.Generator().manual_seed(13 * N + seed)
    rd = lambda *sh: torch.randn(*sh, generator=g, device=gdev)
    rh = lambda *sh: torch.randn(*sh, generator=gh)
    ne = 0.03
    res = {}
    tol = VAE_STEP_TOL

    def full(up_s):   # the sampled rows' upstream gradient inside zeros
        if not sampled:
            return up_s.to(DEV)
        up = torch.zeros(N, *up_s.shape[1:], device=DEV)
        up[S.to(DEV)] = up_s.to(DEV)
        return up

    def cut(t):
        return t.detach()[S.to(t.device)].cpu() if sampled else t.detach().cpu()

    def zero_elsewhere(t, name):
        if sampled:
            other = t.detach().abs().reshape(N, -1).amax(-1)
            other[S.to(t.device)] = 0.0
            assert float(other.max()) == 0.0, (name, int(other.argmax()))

    # encoder head
    feat, eps = torch.relu(rd(N, 512)), rd(N, 2)
    par = [0.05 * rh(2, 512), 0.1 * rh(2), 0.05 * rh(2, 512), 0.1 * rh(2)]
    ups = [rh(len(S), 2) for _ in range(3)]

    def enc(dt, f, e, p):
        mu = F.linear(f, p[0], p[1])
        var = ne * torch.sigmoid(F.linear(f, p[2], p[3]))
        return mu + e * torch.sqrt(var + 1e-6), mu, var
    f64 = feat[S.to(gdev)].cpu().double().requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in par]
    o64 = enc(torch.float64, f64, eps[S.to(gdev)].cpu().double(), p64)
    sum((o * u.double()).sum() for o, u in zip(o64, ups)).backward()
    if yardstick:
        fd, pd = feat.clone().requires_grad_(True), [t.clone().requires_grad_(True) for t in par]
        od = enc(torch.float32, fd, eps, pd)
        sum((o * u).sum() for o, u in zip(od, ups)).backward()
    else:
        fd, pd = feat.to(DEV).requires_grad_(True), [t.to(DEV).requires_grad_(True) for t in par]
        od = EncoderHead.apply(fd, *pd, eps.to(DEV), ne)
        torch.autograd.backward(od, [full(u) for u in ups])
        zero_elsewhere(fd.grad, "enc_head.dfeat")
    for k, a, r in zip(("a", "mu", "var"), od, o64):
        _check_steps("enc_head." + k, _rows(cut(a)), _rows(r), tol["enc_head." + k], res)
    _check_steps("enc_head.dfeat", _rows(cut(fd.grad)), _rows(f64.grad), tol["enc_head.dfeat"], res)
    for a, r in zip(pd, p64):
        _check_whole("enc_head.param", a.grad, r.grad, tol["enc_head.param"], res)

    # decoder fc
    lat, W, b, up_s = rd(N, 2), 0.3 * rh(512, 2), 0.1 * rh(512), rh(len(S), 512)
    l64, W64, b64 = lat[S.to(gdev)].cpu().double().requires_grad_(True), W.double().requires_grad_(True), b.double().requires_grad_(True)
    h64 = F.linear(l64, W64, b64)
    h64.backward(up_s.double())
    if yardstick:
        ld, Wd, bd = lat.clone().requires_grad_(True), W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        h = F.linear(ld, Wd, bd)
        h.backward(up_s)
    else:
        ld, Wd, bd = lat.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        h = DecoderFc.apply(ld, Wd, bd)
        h.backward(full(up_s))
        zero_elsewhere(ld.grad, "dec_fc.da")
    _check_steps("dec_fc.h", _rows(cut(h)), _rows(h64), tol["dec_fc.h"], res)
    _check_steps("dec_fc.da", _rows(cut(ld.grad)), _rows(l64.grad), tol["dec_fc.da"], res)
    _check_steps("dec_fc.dw", Wd.grad.detach().cpu()[:, None], W64.grad[:, None], tol["dec_fc.dw"], res)
    _check_whole("dec_fc.db", bd.grad, b64.grad, tol["dec_fc.db"], res)

    # latent regulariser
    a0, m0 = rd(N, 2), rd(N, 2)
    v0 = 0.01 + 0.05 * torch.rand(N, 2, generator=g, device=gdev)
    w = rh(len(S))
    lg = lambda x, mean, var: -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(var) - (x - mean) ** 2 / (2 * var)
    reg_of = lambda a, m, v: (lg(a, torch.zeros((), dtype=a.dtype), torch.ones((), dtype=a.dtype)) - lg(a, m, v)).sum(-1)
    i64 = [t[S.to(gdev)].cpu().double().requires_grad_(True) for t in (a0, m0, v0)]
    r64 = reg_of(*i64)
    r64.backward(w.double())
    if yardstick:
        idv = [t.clone().requires_grad_(True) for t in (a0, m0, v0)]
        reg = reg_of(*idv)
        reg.backward(w)
    else:
        idv = [t.to(DEV).requires_grad_(True) for t in (a0, m0, v0)]
        reg = LatentReg.apply(*idv)
        reg.backward(full(w))
        for t, k in zip(idv, ("da", "dmu", "dvar")):
            zero_elsewhere(t.grad, "latent_reg." + k)
    _check_steps("latent_reg.reg", _rows(cut(reg)), _rows(r64), tol["latent_reg.reg"], res)
    for t, r, k in zip(idv, i64, ("da", "dmu", "dvar")):
        _check_steps("latent_reg." + k, _rows(cut(t.grad)), _rows(r.grad), tol["latent_reg." + k], res)
    return res


def bce_frames_per_row(DEV, B, T, C=1, H=32, W=32, rows=None, seed=0, yardstick=False):
    """BernoulliFrameLogLik against float64 -BCEWithLogits summed over the pixels: log p(x_t | a_t) and the gradient of the logits
    one frame at a time.  `rows` (given, or B T > 4099): as in vae_heads_per_row."""
    import torch.nn.functional as F
    from kvae.vae.fused import BernoulliFrameLogLik
    N = B * T
    if rows is None and N > 4099:
        rows = _row_sample(N, seed)
    sampled = rows is not None
    assert not (sampled and yardstick)
    gdev = DEV if sampled else "cpu"
    S = rows if sampled else torch.arange(N)
    g = torch.Generator(device=gdev).manual_seed(17 * N + H + seed)
    logits = 3 * torch.randn(B, T, C, H, W, generator=g, device=gdev)
    x = (torch.rand(B, T, C, H, W, generator=g, device=gdev) < 0.2).float()
    w_s = torch.randn(len(S), generator=torch.Generator().manual_seed(19 * N + seed))
    l64 = logits.view(N, -1)[S.to(gdev)].cpu().double().requires_grad_(True)
    ll64 = -F.binary_cross_entropy_with_logits(l64, x.view(N, -1)[S.to(gdev)].cpu().double(), reduction="none").sum(-1)
    ll64.backward(w_s.double())
    res = {}
    if yardstick:
        ld = logits.clone().requires_grad_(True)
        ll = -F.binary_cross_entropy_with_logits(ld, x, reduction="none").sum(dim=(2, 3, 4))
        ll.backward(w_s.view(B, T))
        cut = lambda t: t.detach().reshape(N, -1)
    else:
        ld = logits.to(DEV).requires_grad_(True)
        ll = BernoulliFrameLogLik.apply(ld, x.to(DEV))
        w = torch.zeros(N, device=DEV)
        w[S.to(DEV)] = w_s.to(DEV)
        ll.backward(w.view(B, T))
        if sampled:
            other = ld.grad.abs().reshape(N, -1).amax(-1)
            other[S.to(DEV)] = 0.0
            assert float(other.max()) == 0.0, ("bce.dlogits of a frame without upstream gradient", int(other.argmax()))
        cut = lambda t: t.detach().reshape(N, -1)[S.to(t.device)].cpu()
    _check_steps("bce.ll", _rows(cut(ll)), _rows(ll64), VAE_STEP_TOL["bce.ll"], res)
    _check_steps("bce.dlogits", _rows(cut(ld.grad)), _rows(l64.grad), VAE_STEP_TOL["bce.dlogits"], res)
    return res


VAE_SCALE_CASES = [(l, sd, n) for l, sd in VAE_LAYER_SIDES for n in (13, 64)]   # frames scaled by 1e-3, 1, 1e+2 in turn
VAE_HEADS_N = (1, 2, 37, 1031, 4099)          # CPU tier: the first three
VAE_BCE_CASES = [(1, 1), (2, 3), (7, 9), (64, 50)]   # (B, T) of 32 x 32 frames; CPU tier: the first three


def vae_probe_cases(layer, side):
    """(kind, frame, pos) of every structured probe of one layer: nine positions x the frames of probe_frames x both kinds."""
    _, _, stride, shuf, _, _, _ = VAE_LAYERS[layer]
    so = ((side - 1) // stride + 1) * shuf
    _, frames = probe_frames(layer, side)
    return [(kind, f, pos) for kind, n in (("upstream", so), ("input", side)) for f in frames for pos in _probe_positions(n)]


def vae_variant_cases(DEV, layer):
    """Every small case of one layer, the grids and one two-launch case: what a process started with a kernel switch runs."""
    worst = {}

    def take(res):
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for side in VAE_SIDES[layer]:
        for N in VAE_RESIDUE_N:
            take(conv_layer_per_frame(DEV, layer, N, side))
        for l, sd, N in VAE_GRID_CASES + VAE_SCALE_CASES:
            if (l, sd) == (layer, side):
                take(conv_layer_per_frame(DEV, layer, N, side, scales=(l, sd, N) in VAE_SCALE_CASES))
        for kind, frame, pos in vae_probe_cases(layer, side):
            take(conv_probe(DEV, layer, side, kind, frame, pos))
        take(conv_layer_per_frame(DEV, layer, 16385, side))
    print(worst)
    return worst


# ---- the linear-Gaussian sweeps (LgssmSmooth) and the coupled alpha-network kernels, one (b,t) slice at a time ----
# Bars = 4 x YARDSTICK, as RNN_STEP_TOL: the yardstick of a quantity is the largest per-slice ratio (whole-tensor ratio for the
# summed gradients of broadcast operands, ".sum") of the FLOAT32 run of oracle/torch_oracle.py against its own float64 run over
# the case lists of both tiers (LGSSM_*_CASES, ALPHA_LSTM_CASES below; rerun: the case functions with yardstick=True).  Keys:
# "<family>.<quantity>", family n4 = (4,4,2), n16 = (16,16,2), rt = run-time dimensions, alpha = the coupled kernels.
# The largest ratios of the emulated / generic bodies and of gfx950 against the same float64 runs: the table of DESIGN section 2.
# Less than a factor 2 under the bar: n4.mus_smooth (1.5 x on the CPU tiers, 1.7 x on gfx950), n16.mus_smooth (1.9 x), n16.gQ
# (1.5 x on gfx950).
LGSSM_YARDSTICK = {   # float32 torch oracle against its float64 run, largest ratio over the case lists of both tiers
    "n4.Sigmas_filt": 1.88e-06, "n4.Sigmas_pred": 1.41e-06, "n4.Sigmas_smooth": 8.49e-06, "n4.gA": 4.71e-05, "n4.gB": 9.51e-06,
    "n4.gC": 5.88e-06, "n4.gC.sum": 2.16e-06, "n4.gQ": 3.48e-05, "n4.gQ.sum": 4.91e-07, "n4.gU": 1.28e-05, "n4.gY": 1.28e-05,
    "n4.g_Sigma0": 9.37e-05, "n4.g_Sigma0.sum": 2.13e-06, "n4.g_mu0": 9.54e-06, "n4.g_mu0.sum": 2.81e-06,
    "n4.mus_filt": 8.61e-06, "n4.mus_pred": 7.22e-06, "n4.mus_smooth": 1.01e-05,
    "n16.Sigmas_filt": 8.28e-07, "n16.Sigmas_pred": 9.37e-07, "n16.Sigmas_smooth": 4.69e-06, "n16.gA": 5.59e-06,
    "n16.gB": 3.42e-06, "n16.gC": 3.85e-06, "n16.gC.sum": 1.24e-06, "n16.gQ": 3.15e-05, "n16.gQ.sum": 2.12e-06,
    "n16.gU": 4.17e-06, "n16.gY": 1.05e-05, "n16.g_Sigma0": 2.37e-06, "n16.g_Sigma0.sum": 4.18e-06, "n16.g_mu0": 1.51e-06,
    "n16.g_mu0.sum": 2.58e-06, "n16.mus_filt": 2.01e-06, "n16.mus_pred": 2.01e-06, "n16.mus_smooth": 2.22e-06,
    "rt.Sigmas_filt": 1.18e-06, "rt.Sigmas_pred": 7.61e-07, "rt.Sigmas_smooth": 2.77e-06, "rt.gA": 3.03e-05, "rt.gB": 4.01e-06,
    "rt.gC": 3.51e-06, "rt.gC.sum": 1.78e-06, "rt.gQ": 9.19e-06, "rt.gU": 2.70e-06, "rt.gY": 1.79e-05, "rt.g_Sigma0": 2.31e-06,
    "rt.g_Sigma0.sum": 7.34e-06, "rt.g_mu0": 1.15e-06, "rt.g_mu0.sum": 2.55e-06, "rt.mus_filt": 2.75e-06,
    "rt.mus_pred": 2.70e-06, "rt.mus_smooth": 2.79e-06,
    "alpha.Sigmas_filt": 7.17e-06, "alpha.Sigmas_pred": 6.94e-06, "alpha.Sigmas_smooth": 4.27e-05, "alpha.alpha": 7.16e-06,
    "alpha.c_seq": 4.75e-06, "alpha.gU": 1.84e-04, "alpha.gY": 1.00e-03, "alpha.g_A": 4.89e-05, "alpha.g_B": 1.62e-05,
    "alpha.g_C": 1.32e-04, "alpha.g_S0": 5.61e-06, "alpha.g_head_w.bias": 2.54e-04, "alpha.g_head_w.weight": 2.79e-04,
    "alpha.g_lstm.bias_hh_l0": 3.45e-04, "alpha.g_lstm.bias_ih_l0": 3.45e-04, "alpha.g_lstm.weight_hh_l0": 4.92e-04,
    "alpha.g_lstm.weight_ih_l0": 6.38e-05, "alpha.g_mu0": 1.48e-05, "alpha.h_seq": 5.38e-06, "alpha.mus_filt": 3.09e-05,
    "alpha.mus_pred": 3.15e-05, "alpha.mus_smooth": 5.08e-05, "alpha.record": 7.16e-07,
}
LGSSM_STEP_TOL = {k: 4.0 * v for k, v in LGSSM_YARDSTICK.items()}
LGSSM_STACKS = ("mus_smooth", "Sigmas_smooth", "mus_filt", "Sigmas_filt", "mus_pred", "Sigmas_pred")


def _lgssm_family(n, m, p):
    return {(4, 4, 2): "n4", (16, 16, 2): "n16"}.get((n, m, p), "rt")


def _lgssm_bar(key, yardstick):
    return float("inf") if yardstick else LGSSM_STEP_TOL[key]


def _step_mask(kind, B, T, g):
    """[B,T] float64 mask (1 = observed) or None.  ones; t0_hidden: t = 0 of every sequence (odd sequences also t = 1);
    last_hidden: t = T-1 of every sequence (odd sequences also t = T-2); all_hidden: sequence B // 2 entirely, the others a
    seeded random pattern; block: the reference's t_init / t_steps block, t_init = 1 + b; alternating: (t + b) odd observed;
    random: seeded, per sequence.  Except for ones the patterns differ between the sequences of a batch."""
    if kind is None:
        return None
    mk = torch.ones(B, T, dtype=torch.float64)
    odd = torch.arange(B) % 2 == 1
    if kind == "t0_hidden":
        mk[:, 0] = 0.0
        if T > 2:
            mk[odd, 1] = 0.0
    elif kind == "last_hidden":
        mk[:, T - 1] = 0.0
        if T > 2:
            mk[odd, T - 2] = 0.0
    elif kind == "all_hidden":
        mk = (torch.rand(B, T, generator=g, dtype=torch.float64) > 0.3).double()
        mk[B // 2] = 0.0
    elif kind == "block":
        for b in range(B):
            t0 = min(T - 1, 1 + b)
            mk[b, t0:t0 + max(1, T // 3)] = 0.0
    elif kind == "alternating":
        mk = ((torch.arange(T)[None, :] + torch.arange(B)[:, None]) % 2).double()
    elif kind == "random":
        mk = (torch.rand(B, T, generator=g, dtype=torch.float64) > 0.4).double()
    else:
        assert kind == "ones", kind
    return mk


def _device_leaf(t, DEV, odd=False):
    """(tensor to pass, function returning its gradient): a float32 leaf on DEV - odd: the same values 4 bytes off a 16-byte
    boundary (a view of a leaf one float longer, as unaligned_fallback builds it; .clone() would re-align it)."""
    t = t.float().to(DEV)
    if not odd:
        leaf = t.clone().requires_grad_(True)
        return leaf, (lambda: leaf.grad)
    base = torch.empty(t.numel() + 1, device=DEV)
    with torch.no_grad():
        base[1:].copy_(t.reshape(-1))
    base.requires_grad_(True)
    view = base[1:].view(t.shape)
    assert view.data_ptr() % 16 != 0 and base.data_ptr() % 16 == 0
    return view, (lambda: None if base.grad is None else base.grad[1:].view(t.shape))


def _sweeps_oracle(ops, mask, w, with_rts, dtype):
    """The recursion of O.filter_step / O.smooth_step in `dtype` on the CPU over per-step operands ([B,T,r,c] stacks or one
    broadcast matrix; mu0 [n] or [B,n], S0 [n,n] or [B,n,n]); gradients of sum_i <w_i, stack_i> (w_i None: no upstream gradient)
    by autograd.  Returns (stacks, {operand: gradient})."""
    from oracle import torch_oracle as O
    c = lambda t: t.detach().cpu().to(dtype)
    lv = {k: c(ops[k]).clone().requires_grad_(True) for k in ("Y", "U", "A", "B", "C", "Q", "mu0", "S0")}
    R = c(ops["R"])
    B, T = lv["Y"].shape[:2]
    at = lambda M, t: M[:, t] if M.dim() == 4 else M
    mk = torch.ones(B, T, dtype=dtype) if mask is None else c(mask)
    mu, Sig = lv["mu0"].expand(B, -1).unsqueeze(-1), lv["S0"].expand(B, -1, -1)
    mfs, Sfs, mps, Sps = [], [], [], []
    for t in range(T):
        mu, Sig, mu_p, Sig_p = O.filter_step(mu, Sig, lv["Y"][:, t], lv["U"][:, t], at(lv["A"], t), at(lv["B"], t), at(lv["C"], t),
                                             at(lv["Q"], t), R, mk[:, t])
        mfs.append(mu), Sfs.append(Sig), mps.append(mu_p), Sps.append(Sig_p)
    st = lambda v: torch.stack(v, 1)
    outs = [st(mfs).squeeze(-1), st(Sfs), st(mps).squeeze(-1), st(Sps)]
    if with_rts:
        mus, Sigs = [mfs[-1]], [Sfs[-1]]
        for t in range(T - 2, -1, -1):
            m_s, S_s = O.smooth_step(Sfs[t], Sps[t + 1], Sigs[0], mfs[t], mps[t + 1], mus[0], at(lv["A"], t + 1))
            mus.insert(0, m_s), Sigs.insert(0, S_s)
        outs = [st(mus).squeeze(-1), st(Sigs)] + outs
    sum((o * c(wi)).sum() for o, wi in zip(outs, w) if wi is not None).backward()
    return [o.detach() for o in outs], {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}


def lgssm_sweeps_per_step(DEV, B, T, n, m, p, layout="plain", up="smooth", steps="all", mask_kind=None, prior="shared",
                          misalign=False, only_b=None, q_grad=False, single_launch=False, emulated=False, seed=0, yardstick=False):
    """LgssmSmooth (kvae_lgssm_filter_fwd / _smooth_fwd / _smooth_bwd) against a FLOAT64 run of O.filter_step / O.smooth_step on
    per-step operands that are leaves of their own, one (b,t) slice at a time (_per_step_ratio): the six stacks (up="filter": the
    four filter stacks, with_rts = 0), gY, gU, the per-step gradients gA, gB, gC and gQ, g_mu0 / g_Sigma0 per sequence with
    prior="per_seq"; the summed gradients of broadcast operands (a stride-0 Q or C, a shared mu0 / Sigma0) as whole tensors.
    layout: "abc" one packed record A|B|C and a Q shared by the batch (lstm layout; q_grad: with the gradient of that Q);
    "abq" one packed record A|B|Q and a broadcast C (switching layout, HAS_GQ); "plain" four [B,T,r,c] stacks.
    up: the upstream gradient on the smoothed stacks only ("smooth", HAS_FP off), on all six ("all", HAS_FP), or on the
    filtered and predicted stacks with with_rts = 0 ("filter"); steps: see _upstream; only_b: on ONE sequence only.
    mask_kind: None or a kind of _step_mask.  misalign: one operand (the record, or the A stack) 4 bytes off a 16-byte boundary,
    which sends (4,4,2) to k_smooth_*_n4 and (16,16,2) to k_smooth_*_wide / the one-wavefront bodies.  single_launch: the
    single-launch form of the (4,4,2) kernels (host tier: the split hook; GPU: B above the split or KVAE_M4_SPLIT_MAX_B=0).
    emulated: the host tier runs on emulated wavefronts - the launch counters must show which kernels ran.
    Exact, on the kernel's output: gY and a per-step gC are 0 at every hidden (b,t); with up="filter" and the upstream gradient on
    step s only, gY, gU and every per-step operand gradient are 0 at t > s; with only_b, they are 0 for every other sequence.
    Q is dense SPD (asserted on the float64 inputs: the natural-order solves).  Returns {quantity: largest ratio}."""
    from kvae import _native
    from kvae.kalman.lgssm_ops import LgssmSmooth, Slots
    assert layout in ("abc", "abq", "plain") and up in ("smooth", "all", "filter") and prior in ("shared", "per_seq")
    fam = _lgssm_family(n, m, p)
    with_rts = up != "filter"
    g = torch.Generator().manual_seed(7919 * seed + 1000 * B + 10 * T + n + len(layout) + len(up))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    per_b = (B,) if prior == "per_seq" else ()
    A, Bm = eye + 0.08 * rn(B, T, n, n), 0.1 * rn(B, T, n, m)          # as _random_problem draws its modes
    C = 0.3 * (rn(p, n) if layout == "abq" else rn(B, T, p, n))
    Wq = 0.05 * rn(*(() if layout == "abc" else (B, T)), n, n)
    Q = 0.02 * eye + Wq @ Wq.mT
    Y, U = rn(B, T, p), 0.3 * rn(B, T, m)
    R = 0.03 * torch.eye(p, dtype=torch.float64)
    mu0 = 0.1 * rn(*per_b, n)                                            # the finite prior of tests/test_wave_emu.py
    S0 = 2.0 * eye
    if per_b:
        W0 = 0.3 * rn(B, n, n)
        S0 = S0 + W0 @ W0.mT
    mask = _step_mask(mask_kind, B, T, g)
    shapes = [(B, T, n), (B, T, n, n)] * (3 if with_rts else 2)
    w = [_upstream(rn(*s), steps) for s in shapes]
    if only_b is not None:
        for wi in w:
            wi[torch.arange(B) != only_b] = 0.0
    if up == "smooth":
        w = w[:2] + [None] * 4
    # the float32 values are the problem: the float64 reference runs on exactly them
    r32 = lambda t: None if t is None else t.float().double()
    A, Bm, C, Q, Y, U, R, mu0, S0, mask = (r32(t) for t in (A, Bm, C, Q, Y, U, R, mu0, S0, mask))
    w = [r32(wi) for wi in w]
    assert float(torch.linalg.eigvalsh(Q).min()) > 0.0
    ops = dict(Y=Y, U=U, A=A, B=Bm, C=C, Q=Q, R=R, mu0=mu0, S0=S0)
    outs64, g64 = _sweeps_oracle(ops, mask, w, with_rts, torch.float64)
    if yardstick:
        outs, grads = _sweeps_oracle(ops, mask, w, with_rts, torch.float32)
        if layout == "abc" and not q_grad:
            grads["Q"] = None
    else:
        lib = _native.lib_for(torch.zeros(1, device=DEV))
        d = lambda t: None if t is None else t.float().to(DEV)
        before = [lib.dll.kvae_wemu_launches(i) for i in range(4)] if emulated else None
        Yl, gY = _device_leaf(Y, DEV)
        Ul, gU = _device_leaf(U, DEV)
        m0l, gm0 = _device_leaf(mu0, DEV)
        S0l, gS0 = _device_leaf(S0, DEV)
        nn, nm = n * n, n * m
        fl = lambda t: t.reshape(B, T, -1)
        if layout == "plain":
            Al, gA = _device_leaf(A, DEV, odd=misalign)
            (Bl, gB), (Cl, gC), (Ql, gQ) = (_device_leaf(t, DEV) for t in (Bm, C, Q))
            args, slots = (None, Al, Bl, Cl, Ql), Slots()
        else:
            third = C if layout == "abc" else Q
            rec, grec = _device_leaf(torch.cat([fl(A), fl(Bm), fl(third)], -1), DEV, odd=misalign)
            part = lambda lo, hi, sh: (lambda: grec()[..., lo:hi].reshape(B, T, *sh))
            gA, gB, g3 = part(0, nn, (n, n)), part(nn, nn + nm, (n, m)), part(nn + nm, None, (p, n) if layout == "abc" else (n, n))
            if layout == "abc":
                if q_grad:
                    Ql, gQ = _device_leaf(Q, DEV)
                else:
                    Ql, gQ = d(Q), (lambda: None)
                gC = g3
                args, slots = (rec, None, None, None, Ql), Slots(A=0, B=nn, C=nn + nm)
            else:
                Cl, gC = _device_leaf(C, DEV)
                gQ = g3
                args, slots = (rec, None, None, Cl, None), Slots(A=0, B=nn, Q=nn + nm)
        hook = DEV == "cpu" and single_launch and fam == "n4"
        if single_launch and DEV != "cpu":
            import os
            assert B > 2048 or os.environ.get("KVAE_M4_SPLIT_MAX_B") == "0", "the single-launch form was asked for"
        if hook:
            lib.dll.kvae_wemu_m4_split_max_b(0)
        try:
            outs = LgssmSmooth.apply(Yl, Ul, d(mask), *args, d(R), m0l, S0l, slots, with_rts)
            sum((o * d(wi)).sum() for o, wi in zip(outs, w) if wi is not None).backward()
        finally:
            if hook:
                lib.dll.kvae_wemu_m4_split_max_b(-1)
        grads = dict(Y=gY(), U=gU(), A=gA(), B=gB(), C=gC(), Q=gQ(), mu0=gm0(), S0=gS0())
        if emulated:
            after = [lib.dll.kvae_wemu_launches(i) for i in range(4)]
            delta = [a - b_ for a, b_ in zip(after, before)]
            f, bw = {"n4": (0, 1), "n16": (2, 3)}[fam]
            want = [0, 0, 0, 0]
            if not misalign:
                want[f], want[bw] = 1, (1 if with_rts else 0)   # (the filter-only adjoint is the one-wavefront body on every tier)
            assert delta == want, ("emulated launches", delta, want)
    out = {}
    names = LGSSM_STACKS if with_rts else LGSSM_STACKS[2:]
    for k, got, ref in zip(names, outs, outs64):
        _check_steps(f"{fam}.{k}", got, ref, _lgssm_bar(f"{fam}.{k}", yardstick), out)
    cpu = lambda t: t.detach().cpu()
    per_step = []   # (name, kernel's gradient [B,T,...]) for the exact assertions
    for k, name in (("Y", "gY"), ("U", "gU"), ("A", "gA"), ("B", "gB"), ("C", "gC"), ("Q", "gQ")):
        if grads[k] is None:
            assert k == "Q"
            continue
        key = f"{fam}.{name}"
        if g64[k].dim() == 2:   # a broadcast operand: the summed gradient
            _check_whole(key + ".sum", grads[k], g64[k], _lgssm_bar(key + ".sum", yardstick), out)
        else:
            _check_steps(key, grads[k], g64[k], _lgssm_bar(key, yardstick), out)
            per_step.append((name, cpu(grads[k])))
    for k, name in (("mu0", "g_mu0"), ("S0", "g_Sigma0")):
        key = f"{fam}.{name}"
        if per_b:
            _check_steps(key, grads[k][:, None], g64[k][:, None], _lgssm_bar(key, yardstick), out)
        else:
            _check_whole(key + ".sum", grads[k], g64[k], _lgssm_bar(key + ".sum", yardstick), out)
    # ---- exact zeros, on what the kernels wrote ----
    if mask is not None:
        hidden = mask == 0
        for name, got in per_step:
            if name in ("gY", "gC") and bool(hidden.any()):
                assert float(got[hidden].abs().max()) == 0.0, (name, "not exactly zero at a hidden step")
    if up == "filter" and steps in ("first", "last"):
        s = 0 if steps == "first" else T - 1
        for name, got in per_step:
            if s + 1 < T:
                assert float(got[:, s + 1:].abs().max()) == 0.0, (name, "not exactly zero after the only step with an upstream gradient")
    if only_b is not None and B > 1:
        others = torch.arange(B) != only_b
        for name, got in per_step:
            assert float(got[others].abs().max()) == 0.0, (name, "another sequence's gradient is not exactly zero", only_b)
    return out


def _lg(B, T, layout, up, steps, mask_kind, prior="shared", **kw):
    return dict(B=B, T=T, layout=layout, up=up, steps=steps, mask_kind=mask_kind, prior=prior, **kw)


# (4,4,2), aligned: k_smooth_fwd_m4 / k_smooth_bwd_m4 in the split form (B <= 2048) and k_rts_bwd_items_m4; up="filter" takes
# k_smooth_fwd_m4 forward and the one-wavefront k_smooth_bwd_n4 backward (with_rts = 0).  Every B with a short and a long T, every
# T = 1 ... 5 with B = 17 (one sequence in the ragged second wavefront).
LGSSM_N4_CASES = [
    _lg(1, 1, "abc", "smooth", "all", None),
    _lg(1, 24, "abq", "all", "first", "random", "per_seq"),
    _lg(15, 2, "plain", "filter", "first", "ones"),
    _lg(15, 24, "abc", "all", "last", "t0_hidden", "per_seq", q_grad=True),
    _lg(16, 3, "abq", "smooth", "first", "last_hidden"),
    _lg(16, 24, "plain", "all", "all", "all_hidden", "per_seq"),
    _lg(17, 1, "abq", "all", "all", "t0_hidden", "per_seq"),
    _lg(17, 2, "abc", "all", "last", "last_hidden"),
    _lg(17, 3, "plain", "smooth", "first", "random", "per_seq"),
    _lg(17, 4, "abq", "filter", "first", "all_hidden"),
    _lg(17, 5, "abc", "smooth", "last", "random", "per_seq"),
    _lg(17, 24, "abq", "smooth", "all", "random"),
    _lg(33, 4, "plain", "all", "last", None, "per_seq"),
    _lg(33, 24, "abc", "filter", "last", "random"),
    _lg(33, 5, "abq", "filter", "all", "last_hidden", "per_seq"),
]
# ... the single-launch form of the same kernels (host tier: the split hook; GPU tier: a fresh process with KVAE_M4_SPLIT_MAX_B=0)
LGSSM_N4_SINGLE_CASES = [
    _lg(17, 1, "abc", "all", "all", "t0_hidden", "per_seq", single_launch=True),
    _lg(17, 2, "abq", "smooth", "first", "last_hidden", single_launch=True),
    _lg(17, 3, "plain", "all", "last", "random", "per_seq", single_launch=True),
    _lg(33, 5, "abq", "all", "all", "all_hidden", single_launch=True),
    _lg(16, 24, "abc", "smooth", "first", None, single_launch=True, seed=1),
]
LGSSM_N4_LARGE_CASE = _lg(2049, 3, "abq", "all", "all", "random", "per_seq", single_launch=True)   # GPU tier: its natural size
# ... one operand 4 bytes off a 16-byte boundary: k_smooth_fwd_n4 / k_smooth_bwd_n4, one wavefront per sequence
LGSSM_N4_ODD_CASES = [
    _lg(17, 3, "abc", "all", "all", "random", "per_seq", misalign=True),
    _lg(3, 24, "abq", "smooth", "first", "t0_hidden", misalign=True),
    _lg(1, 1, "plain", "filter", "all", None, misalign=True),
    _lg(5, 2, "plain", "all", "last", "last_hidden", "per_seq", misalign=True),
    _lg(4, 5, "abq", "filter", "first", "all_hidden", misalign=True),
    _lg(2, 4, "abc", "smooth", "last", "ones", misalign=True, q_grad=True),
]
# the upstream gradient on ONE sequence: the first, the last, and both sides of the wavefront boundary at sixteen sequences
LGSSM_N4_ISOLATION_CASES = [
    _lg(33, 3, "abq", "all", "all", "random", "per_seq", only_b=0),
    _lg(33, 3, "abc", "smooth", "all", "random", only_b=32),
    _lg(33, 2, "plain", "all", "all", None, "per_seq", only_b=15),
    _lg(33, 2, "abq", "smooth", "all", "ones", only_b=16),
    _lg(17, 3, "plain", "filter", "all", "random", only_b=16),
    _lg(17, 1, "abc", "all", "all", "t0_hidden", only_b=15),
    _lg(17, 3, "abq", "all", "last", "random", "per_seq", only_b=16, single_launch=True),
]
# (16,16,2), aligned: k_smooth_fwd_n16 / k_smooth_bwd_n16 (up="filter": the 256-thread k_smooth_bwd<D> body backward)
LGSSM_N16_CASES = [
    _lg(1, 1, "abc", "smooth", "all", None),
    _lg(1, 2, "abq", "all", "first", "last_hidden", "per_seq"),
    _lg(1, 3, "plain", "filter", "first", "t0_hidden"),
    _lg(1, 5, "abq", "smooth", "last", "random"),
    _lg(1, 12, "abc", "all", "all", "random", "per_seq", q_grad=True),
    _lg(3, 1, "abq", "all", "all", "t0_hidden", "per_seq"),
    _lg(3, 2, "plain", "all", "last", "all_hidden"),
    _lg(3, 3, "abc", "smooth", "first", "ones", "per_seq"),
    _lg(3, 5, "abq", "filter", "last", "all_hidden", "per_seq"),
    _lg(3, 12, "plain", "smooth", "all", "last_hidden"),
    _lg(3, 3, "abq", "all", "all", "random", only_b=0),
    _lg(3, 2, "abc", "all", "all", None, "per_seq", only_b=2),
]
# ... misaligned: k_smooth_fwd_wide and the 256-thread k_smooth_bwd<D> body
LGSSM_N16_ODD_CASES = [
    _lg(1, 1, "plain", "all", "all", "t0_hidden", "per_seq", misalign=True),
    _lg(3, 2, "abc", "smooth", "first", "random", misalign=True),
    _lg(1, 3, "abq", "filter", "first", None, "per_seq", misalign=True),
    _lg(3, 5, "abq", "all", "last", "last_hidden", misalign=True),
    _lg(3, 12, "abc", "smooth", "all", "all_hidden", "per_seq", misalign=True, q_grad=True),
    _lg(1, 12, "plain", "all", "all", "ones", misalign=True, only_b=0),
]
# run-time dimensions: (2,1,1), (5,3,2), (8,8,3) on the one-wavefront bodies k_smooth_fwd<D> / k_smooth_bwd<D>; (12,12,2) and (16,8,2)
# on the 256-thread bodies (k_smooth_fwd_wide).  B = 3, T = 1, 2, 7.
_RT_OPTS = [("abc", "smooth", "all", None, "shared"), ("abq", "all", "first", "random", "per_seq"), ("plain", "filter", "first", "t0_hidden", "shared"),
            ("plain", "all", "last", "last_hidden", "per_seq"), ("abq", "filter", "all", "all_hidden", "shared"), ("abc", "smooth", "last", "ones", "per_seq")]
LGSSM_RT_CASES = [dict(n=n, m=m, p=p, **_lg(3, T, *_RT_OPTS[(2 * i + j) % 6], **({"only_b": 1} if (i + j) % 4 == 3 else {})))
                  for i, (n, m, p) in enumerate([(2, 1, 1), (5, 3, 2), (8, 8, 3), (12, 12, 2), (16, 8, 2)]) for j, T in enumerate((1, 2, 7))]
LGSSM_RT_CASES.append(dict(n=12, m=12, p=2, **_lg(3, 7, "abc", "all", "last", "ones", "per_seq")))   # (a mask of ones on the 256-thread bodies)


ALPHA_PARAMS = ("A", "B", "C", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "head_w.weight", "head_w.bias")
ALPHA_MARGIN = 0.25  # alpha's per-step maximum must exceed (1 + ALPHA_MARGIN) / K somewhere in every sequence of the float64 run


def _alpha_oracle(dyn, ops, mask, w, with_rts, dtype):
    """O.lgssm_filter / O.lgssm_smooth(kind="lstm") in `dtype` on the CPU, with the masked feedback into the cell.  Returns
    ([stacks..., record A|B|C, alpha], h_seq, c_seq, {name: gradient}) for the loss sum_i <w_i, out_i>."""
    from oracle import torch_oracle as O
    c = lambda t: t.detach().cpu().to(dtype)
    dl = {k: c(v).clone().requires_grad_(True) for k, v in dyn.items()}
    lv = {k: c(ops[k]).clone().requires_grad_(True) for k in ("Y", "U", "mu0", "S0")}
    mk = c(mask)
    o = (O.lgssm_smooth if with_rts else O.lgssm_filter)(lv["Y"], lv["U"], mk, dl, "lstm", c(ops["Q"]), c(ops["R"]), lv["mu0"], lv["S0"])
    keys = LGSSM_STACKS if with_rts else LGSSM_STACKS[2:]
    outs = [o[k].squeeze(-1) if k.startswith("mus") else o[k] for k in keys]
    outs += [torch.cat([o[k].flatten(2) for k in ("A_list", "B_list", "C_list")], -1), o["state_seq"]]
    sum((x * c(wi)).sum() for x, wi in zip(outs, w)).backward()
    with torch.no_grad():   # the cell over the inputs the filter fed it (kalman_filter.py:142, 183-185 of the reference)
        y_pred = (o["C_list"] @ o["mus_pred"]).squeeze(-1)
        y_dyn = mk.unsqueeze(-1) * lv["Y"] + (1.0 - mk.unsqueeze(-1)) * y_pred
        x = torch.cat([torch.zeros_like(y_dyn[:, :1]), y_dyn[:, :-1]], 1)
        state, hs, cs = None, [], []
        for t in range(x.shape[1]):
            _, state = O.lstm_cell(x[:, t], state, dl["lstm.weight_ih_l0"], dl["lstm.weight_hh_l0"], dl["lstm.bias_ih_l0"], dl["lstm.bias_hh_l0"])
            hs.append(state[0]), cs.append(state[1])
    grads = {k: v.grad for k, v in list(dl.items()) + list(lv.items())}
    return [x_.detach() for x_ in outs], torch.stack(hs, 1), torch.stack(cs, 1), grads


def alpha_lstm_per_step(DEV, B, T, n, m, K, mask_kind, steps, with_rts, yardstick=False):
    """AlphaLstmSmooth (k_filter_alpha_lstm + k_alpha_lstm_bwd: LSTM cell, head, softmax, mixing and a filter step in one time
    loop, the coupled adjoint in one launch; (n, m) = (4, 4): the SDims<4,4,2> instance, else RDims) against a FLOAT64 run of
    O.lgssm_filter / O.lgssm_smooth(kind="lstm") on the module's parameters.  Per (b,t): alpha, the record A|B|C, the six stacks
    (with_rts = False: the four filter stacks), h_seq and c_seq (a second, no-grad call with keep_cell=True), gY, gU; whole
    tensors: the gradients of the nine network and mode parameters and of mu0 / Sigma0.  The upstream gradient sits on the
    stacks, the record and alpha (`steps`: see _upstream); mask_kind: see _step_mask.  The model's modes are perturbed and its
    head scaled so that alpha is far from uniform - asserted on the float64 run.  mask_kind "ones": the same problem through the
    precomputed-alpha path of mask=None (kvae_lstm_fwd, the head, kvae_mix_fwd, LgssmSmooth) meets the same bars - no feedback
    term in gC.  with_rts = False and steps = "first": gY and gU of t = T-1 are exactly zero.
    ON A HOST DEVICE THIS DOES NOT CHECK THE KERNELS: the coupled kernels exist on the GPU only, and the product's per-step
    differentiable path (KalmanFilter._filter_stepwise on the host simulation) runs in their place - that checks this case
    function, the float64 reference and the yardstick before the card."""
    from kvae.kalman.lgssm_ops import AlphaLstmSmooth, LgssmSmooth, Slots
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    torch.manual_seed(100000 + 1000 * K + 10 * n + T)
    model = KVAE(KVAEConfig(dynamics_model="lstm", num_modes=K, z_dim=n, u_dim=m))
    kf = model.kalman_filter
    dyn = kf.dyn_params
    with torch.no_grad():   # as test_alpha_lstm_masked_matches_stepwise, the head scaled until the assertion below holds
        dyn.A.add_(0.05 * torch.randn_like(dyn.A))
        dyn.head_w.bias.zero_()
        dyn.head_w.weight.mul_(60.0)
    p = 2
    g = torch.Generator().manual_seed(31 * B + 7 * T + K + len(mask_kind) + len(steps))
    rn = lambda *s: torch.randn(*s, generator=g)
    Y, U = rn(B, T, p), 0.3 * rn(B, T, m)
    mask = _step_mask(mask_kind, B, T, g)
    E = n * n + n * m + p * n
    shapes = [(B, T, n), (B, T, n, n)] * (3 if with_rts else 2) + [(B, T, E), (B, T, K)]
    w = [_upstream(rn(*s), steps) for s in shapes]
    w[-2] *= 0.1   # (the record's entries are O(1): keep its share of the loss next to the stacks')
    params = {k: v.detach().clone() for k, v in dyn.named_parameters()}
    assert tuple(params) == ALPHA_PARAMS, tuple(params)
    ops = dict(Y=Y, U=U, Q=kf.Q.detach().clone(), R=kf.R.detach().clone(), mu0=kf.mu0.detach().clone(), S0=kf.Sigma0.detach().clone())
    outs64, h64, c64, g64 = _alpha_oracle(params, ops, mask, w, with_rts, torch.float64)
    peak = outs64[-1].amax(-1).amax(1)
    assert float(peak.min()) > (1.0 + ALPHA_MARGIN) / K, ("alpha is close to uniform in some sequence", peak.tolist(), K)
    gnames = ALPHA_PARAMS + ("mu0", "S0")
    nogC = None
    if yardstick:
        outs, h_seq, c_seq, grads = _alpha_oracle(params, ops, mask, w, with_rts, torch.float32)
    else:
        kf = kf.to(DEV).train()
        d = lambda t: t.float().to(DEV)
        Yl, Ul, mu0l, S0l = (d(ops[k]).clone().requires_grad_(True) for k in ("Y", "U", "mu0", "S0"))
        mk, wd = d(mask), [d(wi) for wi in w]
        plist = [dyn.get_parameter(k) for k in ALPHA_PARAMS]
        leaves = [Yl, Ul] + plist + [mu0l, S0l]
        if str(DEV).startswith("cuda"):
            net = [dyn.get_parameter(k) for k in ALPHA_PARAMS[3:]] + plist[:3]
            outs = AlphaLstmSmooth.apply(Yl, Ul, mk, *net, kf.Q, kf.R, mu0l, S0l, with_rts)
            with torch.no_grad():
                h_seq, c_seq = AlphaLstmSmooth.apply(Yl, Ul, mk, *net, kf.Q, kf.R, mu0l, S0l, with_rts, True)[-2:]
        else:   # the per-step differentiable path in the kernels' place (see the docstring)
            kf.mu0, kf.Sigma0 = mu0l, S0l
            dyn.reset_state()
            mf, Sf, mp, Sp, A_l, B_l, C_l = kf._filter_stepwise(Yl, Ul, mk)
            alpha = dyn.state_seq
            stacks = [mf.squeeze(-1), Sf, mp.squeeze(-1), Sp]
            if with_rts:
                stacks = list(LgssmSmooth.apply(Yl, Ul, mk, None, A_l, B_l, C_l, kf.Q, kf.R, mu0l, S0l, Slots(), True))
            outs = stacks + [torch.cat([A_l.flatten(2), B_l.flatten(2), C_l.flatten(2)], -1), alpha]
            with torch.no_grad():
                y_dyn = mk.unsqueeze(-1) * Yl + (1.0 - mk.unsqueeze(-1)) * (C_l @ mp).squeeze(-1)
                _, c_seq, h_seq = _lstm_restated(dyn.lstm, torch.cat([torch.zeros_like(y_dyn[:, :1]), y_dyn[:, :-1]], 1))
        gl = torch.autograd.grad(sum((o * wi).sum() for o, wi in zip(outs, wd)), leaves, allow_unused=True)
        grads = dict(zip(("Y", "U") + gnames, gl))
        if mask_kind == "ones":   # the same problem without a mask: precomputed alpha, no cell inside the filter
            dyn.reset_state()
            a_seq = dyn.alpha_sequence(Yl)
            rec, slots, _ = dyn.step_record(a_seq)
            o2 = LgssmSmooth.apply(Yl, Ul, None, rec, None, None, None, kf.Q, kf.R, mu0l, S0l, slots, with_rts)
            outs_nomask = list(o2) + [rec, a_seq]
            gl2 = torch.autograd.grad(sum((o * wi).sum() for o, wi in zip(outs_nomask, wd)), leaves, allow_unused=True)
            nogC = (outs_nomask, dict(zip(("Y", "U") + gnames, gl2)))
    out = {}
    bar = lambda k: _lgssm_bar("alpha." + k, yardstick)
    names = (LGSSM_STACKS if with_rts else LGSSM_STACKS[2:]) + ("record", "alpha")

    def compare(outs_, grads_):
        for k, got, ref in zip(names, outs_, outs64):
            _check_steps("alpha." + k, got, ref, bar(k), out)
        _check_steps("alpha.gY", grads_["Y"], g64["Y"], bar("gY"), out)
        _check_steps("alpha.gU", grads_["U"], g64["U"], bar("gU"), out)
        for k in gnames:
            ref = g64[k] if g64[k] is not None else torch.zeros_like(params.get(k, ops.get(k)), dtype=torch.float64)
            got = grads_[k] if grads_[k] is not None else torch.zeros_like(ref)
            if float(ref.abs().max()) == 0.0:   # (T = 1: the cell's input and previous state are zero vectors)
                assert float(got.abs().max()) == 0.0, (k, "the float64 gradient is exactly zero")
            else:
                _check_whole("alpha.g_" + k, got, ref, bar("g_" + k), out)

    compare(outs, grads)
    _check_steps("alpha.h_seq", h_seq, h64, bar("h_seq"), out)
    _check_steps("alpha.c_seq", c_seq, c64, bar("c_seq"), out)
    if nogC is not None:
        compare(*nogC)
    if not yardstick and not with_rts and steps == "first" and T > 1:
        for k in ("Y", "U"):
            assert float(g64[k][:, T - 1].abs().max()) == 0.0   # ... of the float64 run
            assert float(grads[k][:, T - 1].abs().max()) == 0.0, (k, "t = T-1 is not exactly zero")
    return out


# (B, T, n, m, K, mask_kind, steps, with_rts): (4,4) takes the SDims<4,4,2> instance, (5,3) and (16,16) RDims
ALPHA_LSTM_CASES = [
    (1, 1, 4, 4, 2, "ones", "all", True), (5, 1, 5, 3, 3, "t0_hidden", "all", False), (1, 1, 16, 16, 16, "all_hidden", "all", True),
    (5, 2, 4, 4, 3, "t0_hidden", "first", True), (1, 2, 5, 3, 16, "last_hidden", "first", False), (5, 2, 16, 16, 2, "alternating", "last", True),
    (5, 3, 4, 4, 16, "last_hidden", "first", False), (5, 3, 5, 3, 2, "all_hidden", "last", True), (1, 3, 16, 16, 3, "t0_hidden", "all", False),
    (5, 3, 4, 4, 2, "all_hidden", "all", True), (5, 3, 16, 16, 3, "block", "first", True), (1, 3, 4, 4, 3, "random", "last", False),
    (5, 20, 4, 4, 3, "t0_hidden", "all", True), (5, 20, 4, 4, 3, "all_hidden", "first", False), (5, 20, 4, 4, 2, "block", "last", True),
    (5, 20, 4, 4, 16, "alternating", "all", False), (1, 20, 4, 4, 3, "random", "first", True), (5, 20, 4, 4, 3, "ones", "all", False),
    (5, 20, 4, 4, 2, "last_hidden", "first", False), (5, 20, 4, 4, 3, "last_hidden", "last", True),
    (5, 20, 5, 3, 3, "all_hidden", "all", True), (5, 20, 5, 3, 16, "t0_hidden", "last", False), (1, 20, 5, 3, 2, "block", "all", False),
    (5, 20, 5, 3, 3, "ones", "first", True), (5, 20, 5, 3, 2, "random", "all", True), (5, 20, 5, 3, 3, "alternating", "first", False),
    (5, 20, 16, 16, 3, "all_hidden", "all", False), (5, 20, 16, 16, 2, "t0_hidden", "first", True), (1, 20, 16, 16, 16, "last_hidden", "all", True),
    (5, 20, 16, 16, 3, "random", "last", False), (5, 20, 16, 16, 3, "ones", "last", True), (5, 20, 16, 16, 2, "alternating", "all", False),
]


def lgssm_case_id(c):
    dims = "%d-%d-%d_" % (c["n"], c["m"], c["p"]) if "n" in c else ""
    extra = "".join("_%s%s" % (k, "" if v is True else v) for k, v in c.items() if k in ("misalign", "only_b", "q_grad", "single_launch", "seed"))
    return "%sB%d_T%d_%s_%s_%s_%s_%s%s" % (dims, c["B"], c["T"], c["layout"], c["up"], c["steps"], c["mask_kind"], c["prior"], extra)


def run_lgssm_case(DEV, case, dims=None, **kw):
    """One entry of the LGSSM_*_CASES lists through lgssm_sweeps_per_step ((n, m, p) from the entry, else `dims`)."""
    c = dict(case)
    n, m, p = (c.pop(k) for k in ("n", "m", "p")) if "n" in c else dims
    return lgssm_sweeps_per_step(DEV, c.pop("B"), c.pop("T"), n, m, p, **c, **kw)


def lgssm_single_launch_cases(DEV):
    """What a process started with KVAE_M4_SPLIT_MAX_B=0 runs: the single-launch form of the (4,4,2) kernels below the split."""
    worst = {}
    for c in LGSSM_N4_SINGLE_CASES + [x for x in LGSSM_N4_ISOLATION_CASES if x.get("single_launch")]:
        for k, v in run_lgssm_case(DEV, c, (4, 4, 2)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(worst)
    return worst


# ---- the ELBO bodies of csrc/lgssm_elbo.h (elbo_probe_body, elbo_body) one (b,t) at a time against float64 ----
# Kernel families by key: "tpp" k_elbo_probe_tpp / k_elbo_tpp<SDims<4,4,2>> (one thread per step, levels[2] == 1), "n4w" / "n16w" /
# "rt" k_elbo_probe<D> / k_elbo<D> (one wavefront per step, levels[2] == 0) for SDims<4,4,2> (KVAE_ELBO_TPP=0), SDims<16,16,2>
# (misaligned operands or KVAE_N16=0) and RDims.  Bars = 4 x ELBO_YARDSTICK; the yardstick of "<family>.<quantity>" is the
# largest per-slice ratio of the FLOAT32 run of the torch oracle (O.lgssm_elbo_terms) against its float64 run over the case lists
# of both tiers (elbo_yardstick() reruns it); ".lv" keys: the cases with a raised _safe_cholesky level, where the yardstick differs
# by more than 2 x from level 0 (a poisoned pivot amplifies rounding).  Kernel ratios against the same float64 runs: DESIGN section 2.
# Less than a factor 2 under the bar, on the host bodies and on gfx950 alike: tpp.gC.sum / n4w.gC.sum (1.37 x), n16w.in (1.39 x),
# tpp.gQ.lv (1.5 x), tpp.gB.lv (1.5 x), rt.gA.lv (1.6 x), tpp.gA.lv (1.9 x); n4w.ent.lv (1.9 x) on gfx950.
ELBO_YARDSTICK = {   # float32 torch oracle against its float64 run, largest ratio over the case lists of both tiers
    "n16w.em": 3.08e-07, "n16w.em.lv": 2.35e-06, "n16w.ent": 1.08e-07, "n16w.ent.lv": 1.85e-06, "n16w.gA": 2.90e-07,
    "n16w.gB": 2.47e-07, "n16w.gC": 1.81e-07, "n16w.gC.lv": 4.60e-07, "n16w.gC.sum": 1.69e-07, "n16w.gC.sum.lv": 7.40e-08,
    "n16w.gQ": 5.40e-07, "n16w.gU": 3.39e-07, "n16w.gY": 2.01e-07, "n16w.gY.lv": 4.81e-07, "n16w.g_Sigmas": 3.22e-07,
    "n16w.g_mus": 1.97e-07, "n16w.g_mus.lv": 4.31e-06, "n16w.in": 3.79e-08, "n16w.in.lv": 1.33e-07, "n16w.tr": 3.22e-07,
    "n4w.em": 9.39e-07, "n4w.ent": 2.26e-07, "n4w.ent.lv": 3.14e-06, "n4w.gA": 3.00e-07, "n4w.gA.lv": 9.24e-07, "n4w.gB": 2.71e-07,
    "n4w.gB.lv": 9.62e-07, "n4w.gC": 1.02e-06, "n4w.gC.sum": 9.06e-08, "n4w.gC.sum.lv": 2.03e-07, "n4w.gQ": 8.52e-07,
    "n4w.gQ.sum": 2.70e-07, "n4w.gU": 9.32e-07, "n4w.gY": 9.28e-07, "n4w.g_Sigmas": 1.25e-06, "n4w.g_mus": 8.13e-07,
    "n4w.g_mus.lv": 1.34e-05, "n4w.in": 2.46e-07, "n4w.tr": 3.77e-07, "n4w.tr.lv": 1.04e-06, "rt.em": 2.53e-07,
    "rt.em.lv": 7.90e-07, "rt.ent": 2.39e-07, "rt.ent.lv": 8.64e-07, "rt.gA": 3.08e-07, "rt.gA.lv": 7.59e-07, "rt.gB": 3.05e-07,
    "rt.gB.lv": 8.35e-07, "rt.gC": 1.84e-07, "rt.gC.lv": 7.05e-07, "rt.gC.sum": 2.34e-07, "rt.gQ": 6.49e-07, "rt.gQ.lv": 1.69e-06,
    "rt.gQ.sum": 2.51e-07, "rt.gU": 3.72e-07, "rt.gU.lv": 9.79e-07, "rt.gY": 1.54e-07, "rt.gY.lv": 7.02e-07,
    "rt.g_Sigmas": 4.04e-07, "rt.g_Sigmas.lv": 2.13e-06, "rt.g_mus": 2.86e-07, "rt.g_mus.lv": 2.19e-06, "rt.in": 9.95e-08,
    "rt.in.lv": 2.26e-07, "rt.tr": 6.40e-07, "rt.tr.lv": 1.58e-06, "tpp.em": 9.39e-07, "tpp.ent": 2.75e-07, "tpp.ent.lv": 7.47e-06,
    "tpp.gA": 3.58e-07, "tpp.gA.lv": 1.48e-06, "tpp.gB": 2.71e-07, "tpp.gB.lv": 1.19e-06, "tpp.gC": 1.02e-06,
    "tpp.gC.sum": 9.06e-08, "tpp.gC.sum.lv": 2.03e-07, "tpp.gQ": 6.53e-07, "tpp.gQ.lv": 2.31e-06, "tpp.gQ.sum": 2.74e-07,
    "tpp.gU": 4.77e-07, "tpp.gU.lv": 1.59e-06, "tpp.gY": 9.28e-07, "tpp.g_Sigmas": 8.11e-07, "tpp.g_Sigmas.lv": 2.71e-06,
    "tpp.g_mus": 8.13e-07, "tpp.g_mus.lv": 1.34e-05, "tpp.in": 2.46e-07, "tpp.tr": 5.48e-07, "tpp.tr.lv": 1.64e-06,
}
ELBO_STEP_TOL = {k: 4.0 * v for k, v in ELBO_YARDSTICK.items()}
ELBO_TERMS = ("tr", "em", "in", "ent")
ELBO_GRADS = ("g_mus", "g_Sigmas", "gY", "gU", "gA", "gB", "gC", "gQ")
ELBO_GUARD = -7.25e33   # what the guard records and every output element hold before the call
ELBO_SIG_BAD = {0: None, 2: -5e-5, 3: -4e-4, 5: -1.0}   # the first diagonal entry of the ONE poisoned Sigma_s, by level wanted
ELBO_Q_BAD = {0: None, 1: -3e-6, 5: -1.0}              # ... and entry min(2, n-1) of the poisoned Q


def _elbo_bar(name, raised, free):
    if free:
        return float("inf")
    return ELBO_STEP_TOL[name + ".lv"] if raised and name + ".lv" in ELBO_STEP_TOL else ELBO_STEP_TOL[name]


def _guarded(dev, B, T, rec):
    """([B,T,rec] view, the flat buffer it lives in): one record in front and one behind, everything filled with ELBO_GUARD."""
    flat = torch.full(((B * T + 2) * rec,), ELBO_GUARD, device=dev, dtype=torch.float32)
    return flat[rec:(B * T + 1) * rec].view(B, T, rec), flat


def elbo_raw(DEV, mus, Sig, eps, Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, S0, slots, grads=True, need_q=True, use_ws=True,
             sig_odd=False):
    """kvae_lgssm_elbo through the loaded library, the problem built as LgssmElbo builds it (lgssm_ops._Call / _GradSink), the
    outputs NOT summed.  terms, g_mus, g_Sigmas and ws_lz have one guard record in front and one behind; every output element
    holds ELBO_GUARD before the call: afterwards both guards must be untouched and every (b,t) overwritten (ws_lz: when the
    batch resolved Sigma_s at level 0 - a step whose own level is raised parks nothing).  use_ws=False: ws_lz = NULL, the
    "always recompute" path of the C ABI.  sig_odd: Sigma_s 4 bytes off a 16-byte boundary.
    Returns CPU tensors: terms [B,T,4], levels [3], ws [B,T,n] | None and, with grads, g_mus, g_Sigmas, gY, gU, gA, gB, gC,
    gQ | None per step."""
    import ctypes as C
    from kvae import _native as N
    from kvae.kalman.lgssm_ops import _Call, _GradSink
    d = lambda t: None if t is None else t.detach().float().to(DEV).contiguous()
    mus, eps, Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, S0 = (d(t) for t in (mus, eps, Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, S0))
    Sig = _device_leaf(Sig, DEV, odd=sig_odd)[0].detach()
    call = _Call(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, S0, slots)
    B, T, n, m, p = call.dims
    dev = call.Y.device
    (terms, f_terms), (ws, f_ws) = _guarded(dev, B, T, 4), (_guarded(dev, B, T, n) if use_ws else (None, None))
    levels = torch.full((3,), -1, device=dev, dtype=torch.int32)
    g_mus = g_Sig = f_gm = f_gS = sink = None
    filled = []
    if grads:
        (g_mus, f_gm), (g_Sig, f_gS) = _guarded(dev, B, T, n), _guarded(dev, B, T, n * n)
        sink = _GradSink(call, packed, A, Bm, Cm, Q, slots, need_q)
        filled = [sink.gY, sink.gU] + [b for b, _ in sink.out.values()] + ([sink.gpacked] if sink.gpacked is not None else [])
        for t in filled:
            t.fill_(ELBO_GUARD)
    call.lib.check(call.lib.dll.kvae_lgssm_elbo(C.byref(call.prob), N.ptr(mus), N.ptr(Sig), N.ptr(eps), N.ptr(terms), N.ptr(levels),
                                                N.ptr(ws), N.ptr(g_mus), N.ptr(g_Sig), C.byref(sink.g) if sink else None, call.stream),
                   "kvae_lgssm_elbo")
    lv = levels.cpu().tolist()
    for name, view, flat, rec in (("terms", terms, f_terms, 4), ("ws_lz", ws, f_ws, n), ("g_mus", g_mus, f_gm, n), ("g_Sigmas", g_Sig, f_gS, n * n)):
        if flat is None:
            continue
        flat = flat.cpu()
        assert bool((flat[:rec] == ELBO_GUARD).all()), (name, "the guard record in front was written")
        assert bool((flat[-rec:] == ELBO_GUARD).all()), (name, "the guard record behind was written")
        if name != "ws_lz" or lv[0] == 0:
            left = (view.cpu().reshape(B * T, -1) == ELBO_GUARD).any(-1).nonzero().flatten().tolist()
            assert not left, (name, "not overwritten at (b,t)", [divmod(q, T) for q in left[:4]])
    for t in filled:
        assert not bool((t == ELBO_GUARD).any()), "an element of a gradient buffer was not overwritten"
    c = lambda t: None if t is None else t.detach().cpu().clone()
    out = dict(terms=c(terms), levels=lv, ws=c(ws))
    if grads:
        nn, nm = n * n, n * m

        def stack(name, off, r, cc):
            if off is not None:
                return c(sink.gpacked[..., off:off + r * cc]).reshape(B, T, r, cc)
            return c(sink.out[name][0]) if name in sink.out else None
        out.update(g_mus=c(g_mus), g_Sigmas=c(g_Sig).reshape(B, T, n, n), gY=c(sink.gY), gU=c(sink.gU), gA=stack("gA", slots.A, n, n),
                   gB=stack("gB", slots.B, n, m), gC=stack("gC", slots.C, p, n), gQ=stack("gQ", slots.Q, n, n))
    return out


def _elbo_oracle(ops, dtype, grads=True):
    """O.lgssm_elbo_terms(per_step=True) in `dtype` on the CPU, every per-step operand expanded to a [B,T,r,c] leaf of its own (so a
    broadcast operand has a per-step gradient too); gradients of the total by autograd.  The same dict as elbo_raw returns."""
    from oracle import torch_oracle as O
    c = lambda t: t.detach().cpu().to(dtype)
    B, T = ops["Y"].shape[:2]
    lv = {k: c(ops[k]).clone().requires_grad_(grads) for k in ("mus", "Sig", "Y", "U", "A", "B", "C", "Q")}
    shared = {k: lv[k] for k in ("C", "Q") if lv[k].dim() == 2}   # autograd sums a broadcast operand's gradient in `dtype`
    for k in ("A", "B", "C", "Q"):
        if lv[k].dim() == 2:
            lv[k] = lv[k].expand(B, T, *lv[k].shape).clone()
            if grads:
                lv[k].retain_grad()
    mask = torch.ones(B, T, dtype=dtype) if ops["mask"] is None else c(ops["mask"])
    with torch.set_grad_enabled(grads):
        terms = torch.stack(O.lgssm_elbo_terms(lv["mus"], lv["Sig"], lv["Y"], lv["U"], lv["A"], lv["B"], lv["C"], lv["Q"], c(ops["R"]),
                                               c(ops["mu0"]), c(ops["S0"]), mask, c(ops["eps"]), per_step=True), -1)
    lvS = O.safe_cholesky(lv["Sig"].detach(), return_level=True)[1]
    lvQ = O.safe_cholesky(lv["Q"].detach()[:, 1:], return_level=True)[1] if T > 1 else 0
    out = dict(terms=terms.detach(), levels=[lvS, lvQ, None], ws=None)
    if grads:
        terms.sum().backward()
        g = lambda k: lv[k].grad if lv[k].grad is not None else torch.zeros_like(lv[k])
        out.update(g_mus=g("mus"), g_Sigmas=g("Sig"), gY=g("Y"), gU=g("U"), gA=g("A"), gB=g("B"), gC=g("C"), gQ=g("Q"))
        out.update({"g%s.sum" % k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in shared.items()})
    return out


def _elbo_compare(fam, raised, got, ref, layout, free, out):
    """Per (b,t): the four terms and every gradient stack `got` holds; the gradient of a broadcast operand as a whole tensor (the
    per-step buffer summed in float32, as lgssm_ops._reduce_to does; the float32 oracle: autograd's own sum); the four sums within 1e-4 of float64.  Keys of `out`: "<fam>.<quantity>" (+ ".lv" for a case with a raised level)."""
    sfx = ".lv" if raised else ""

    def steps(name, a, b):
        ratio, where = _per_step_ratio(a.detach().cpu(), b.detach())
        out[name + sfx] = max(out.get(name + sfx, 0.0), ratio)
        bar = _elbo_bar(name, raised, free)
        assert ratio < bar, (name, "ratio %.3g at (b,t) = %s, bar %.3g" % (ratio, where, bar), fam, layout)
    for i, k in enumerate(ELBO_TERMS):
        steps(f"{fam}.{k}", got["terms"][..., i:i + 1], ref["terms"][..., i:i + 1])
    for k in ELBO_GRADS:
        if got.get(k) is not None:
            steps(f"{fam}.{k}", got[k], ref[k])
    for k, lay in (("gC", "abq"), ("gQ", "abc")):
        if layout == lay and got.get(k) is not None:
            name = f"{fam}.{k}.sum"
            ratio = rel_err(got[name[len(fam) + 1:]] if name[len(fam) + 1:] in got else got[k].sum((0, 1)), ref[name[len(fam) + 1:]])   # (the product sums in float32)
            out[name + sfx] = max(out.get(name + sfx, 0.0), ratio)
            assert ratio < _elbo_bar(name, raised, free), (name, ratio, fam, layout)
    for i, k in enumerate(ELBO_TERMS):
        a, b = float(got["terms"][..., i].sum()), float(ref["terms"][..., i].sum())
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-3, ("sum of", k, a, b, fam, layout)


def _elbo_poison_q(pos, B, T, for_q):
    """The (b,t) of the ONE poisoned matrix: pos "first" (q = 0; Q: q = 1), an index q = b T + t, or "last"; a Q moves on to t = 1
    of its sequence, since Q_0 is never factorised."""
    q = {"first": 1 if for_q else 0, "last": B * T - 1}.get(pos, pos)
    q = min(int(q), B * T - 1)
    b, t = divmod(q, T)
    if for_q and t == 0 and T > 1:
        t = 1
    return b, t


def elbo_per_step(DEV, B, T, n, m, p, fam, layout="plain", mask_kind=None, prior="shared", levels=(0, 0), pos="first", q_grad=True,
                  family=None, sig_odd=False, seed=0, yardstick=False, free=False):
    """kvae_lgssm_elbo (elbo_raw: the un-summed terms and the sink's per-step gradients) against a FLOAT64 run of
    O.lgssm_elbo_terms(per_step=True) on exactly the float32 operand values, one (b,t) slice at a time (_per_step_ratio).
    fam: the key of the bars ("tpp", "n4w", "n16w", "rt"); family: what levels[2] must report (None: not 2 or 3).
    layout: "abc" one packed record A|B|C and ONE Q for the batch (q_grad: with its gradient); "abq" one packed record A|B|Q and a
    broadcast C; "plain" four [B,T,r,c] stacks.  Sigma_s, Q and Sigma0 dense SPD (asserted), R not diagonal; prior "shared" or
    "per_seq" (mu0_sb, Sigma0_sb != 0); mask_kind: a kind of _step_mask.  levels = (level of Sigma_s, level of Q) of _safe_cholesky,
    forced by ONE poisoned matrix at `pos` (_elbo_poison_q; layout "abc": the shared Q itself, which only (0,1) probes).  With T = 1
    no Q is ever factorised: its level must be 0 whatever Q holds.  The levels of the float64 run, of the C oracle and of the
    kernel must agree.
    Exact, on what the kernel wrote: emission term, gY, gC zero at hidden steps; transition term, gA, gB, gU, gQ zero at t = 0; init
    term zero at t > 0; g_Sigmas symmetric to the bit, and diagonal at level 5, where the clamped entry's gradient is exactly 0;
    ws_lz = NULL gives the bits of the parked-sample path and meets the same bars; with mus, eps, Sigma_s of ONE sequence redrawn
    (first, middle, last) every output of every other sequence keeps its bits.
    yardstick: the float32 run of the torch oracle in the kernel's place; free: no bars (measuring).  Returns {key: largest ratio}."""
    from kvae.kalman.lgssm_ops import Slots
    from oracle import c_oracle
    assert layout in ("abc", "abq", "plain") and prior in ("shared", "per_seq")
    g = torch.Generator().manual_seed(7919 * seed + 1000 * B + 10 * T + n + 3 * len(layout))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    eye, eyep = torch.eye(n, dtype=torch.float64), torch.eye(p, dtype=torch.float64)
    per_b = (B,) if prior == "per_seq" else ()

    def draw_q(Bn):   # mus, eps, Sigma_s of Bn sequences
        W = 0.1 * rn(Bn, T, n, n)
        return 0.5 * rn(Bn, T, n), rn(Bn, T, n), W @ W.mT + 0.3 * eye
    mus, eps, Sig = draw_q(B)
    Y, U = rn(B, T, p), 0.3 * rn(B, T, m)
    A, Bm = 0.9 * eye + 0.08 * rn(B, T, n, n), 0.1 * rn(B, T, n, m)
    C = 0.3 * (rn(p, n) if layout == "abq" else rn(B, T, p, n))
    Wq = rn(*(() if layout == "abc" else (B, T)), n, n)
    Q = 0.02 * eye + 0.0005 * (Wq @ Wq.mT)
    Wr = 0.1 * rn(p, p)
    R = 0.03 * eyep + Wr @ Wr.T
    mu0 = 0.1 * rn(*per_b, n)
    W0 = 0.2 * rn(*per_b, n, n)
    S0 = W0 @ W0.mT + 0.5 * eye
    mask = _step_mask(mask_kind, B, T, g)
    for M in (Sig, Q, S0, R):
        assert float(torch.linalg.eigvalsh(M.float().double()).min()) > 0.0
    lvS, lvQ = levels
    sb, st = _elbo_poison_q(pos, B, T, False)
    qb, qt = _elbo_poison_q(pos, B, T, True)
    bad_S = None if ELBO_SIG_BAD[lvS] is None else torch.diag(torch.tensor([ELBO_SIG_BAD[lvS]] + [0.2] * (n - 1), dtype=torch.float64))
    jq = min(2, n - 1)
    bad_Q = None if ELBO_Q_BAD[lvQ] is None else torch.diag(torch.tensor([0.02] * jq + [ELBO_Q_BAD[lvQ]] + [0.02] * (n - 1 - jq), dtype=torch.float64))
    if bad_S is not None:
        Sig[sb, st] = bad_S
    if bad_Q is not None:
        if layout == "abc":
            Q = bad_Q
        else:
            Q[qb, qt] = bad_Q
    want = [lvS, lvQ if T > 1 else 0]
    r32 = lambda t: None if t is None else t.float().double()   # the float32 values are the problem
    ops = {k: r32(v) for k, v in dict(mus=mus, Sig=Sig, eps=eps, Y=Y, U=U, mask=mask, A=A, B=Bm, C=C, Q=Q, R=R, mu0=mu0, S0=S0).items()}
    ref = _elbo_oracle(ops, torch.float64)
    assert ref["levels"][:2] == want, ("levels of the float64 run", ref["levels"], want)
    _, clv = c_oracle.elbo_terms(ops["mus"], ops["Sig"], ops["eps"], ops["Y"], ops["U"], ops["mask"], ops["A"], ops["B"], ops["C"], ops["Q"],
                                 ops["R"], ops["mu0"][0] if per_b else ops["mu0"], ops["S0"][0] if per_b else ops["S0"])
    assert list(clv) == want, ("levels of the C oracle", list(clv), want)
    raised = max(want) > 0
    out = {}
    if yardstick:
        got = _elbo_oracle(ops, torch.float32)
        assert got["levels"][:2] == want, ("levels of the float32 run", got["levels"], want)
        _elbo_compare(fam, raised, got, ref, layout, True, out)
        return out
    nn, nm = n * n, n * m
    fl = lambda t: t.reshape(B, T, -1)
    if layout == "plain":
        stacks, slots = (None, ops["A"], ops["B"], ops["C"], ops["Q"]), Slots()
    elif layout == "abc":
        stacks, slots = (torch.cat([fl(ops["A"]), fl(ops["B"]), fl(ops["C"])], -1), None, None, None, ops["Q"]), Slots(A=0, B=nn, C=nn + nm)
    else:
        stacks, slots = (torch.cat([fl(ops["A"]), fl(ops["B"]), fl(ops["Q"])], -1), None, None, ops["C"], None), Slots(A=0, B=nn, Q=nn + nm)
    need_q = layout != "abc" or q_grad

    def run(mus_, eps_, Sig_, **kw):
        r = elbo_raw(DEV, mus_, Sig_, eps_, ops["Y"], ops["U"], ops["mask"], *stacks, ops["R"], ops["mu0"], ops["S0"], slots, need_q=need_q,
                     sig_odd=sig_odd, **kw)
        assert r["levels"][:2] == want, ("levels of the kernel", r["levels"], want)
        if family is None:
            assert r["levels"][2] not in (2, 3), ("kernel family", r["levels"][2])
        else:
            assert r["levels"][2] == family, ("kernel family", r["levels"][2], family)
        return r
    got = run(ops["mus"], ops["eps"], ops["Sig"])
    _elbo_compare(fam, raised, got, ref, layout, free, out)
    # ---- exact, on what the kernel wrote ----
    where = lambda cond: [tuple(x) for x in cond.nonzero()[:4].tolist()]
    flat = lambda t: t.reshape(B, T, -1)
    tm = got["terms"]
    if mask is not None and bool((ops["mask"] == 0).any()):
        hidden = ops["mask"] == 0
        for k, v in (("em", tm[..., 1:2]), ("gY", got["gY"]), ("gC", got["gC"])):
            bad = (flat(v) != 0).any(-1) & hidden
            assert not bool(bad.any()), (k, "not exactly zero at hidden (b,t)", where(bad), fam, layout)
    for k, v in (("tr", tm[..., 0:1]), ("gA", got["gA"]), ("gB", got["gB"]), ("gU", got["gU"]), ("gQ", got["gQ"])):
        if v is not None:
            bad = (flat(v)[:, 0] != 0).any(-1)
            assert not bool(bad.any()), (k, "not exactly zero at t = 0 of sequences", where(bad), fam, layout)
    bad = tm[:, 1:, 2] != 0
    assert not bool(bad.any()), ("in", "not exactly zero at (b,t-1)", where(bad), fam, layout)
    gS = got["g_Sigmas"]
    bad = (gS != gS.mT).flatten(2).any(-1)
    assert not bool(bad.any()), ("g_Sigmas", "not symmetric to the bit at (b,t)", where(bad), fam, layout)
    offdiag = lambda M: (M - torch.diag_embed(torch.diagonal(M, dim1=-2, dim2=-1))).flatten(2).abs().amax(-1)
    if want[0] == 5:
        assert float(offdiag(gS).max()) == 0.0, ("g_Sigmas", "not diagonal at level 5", where(offdiag(gS) != 0), fam)
        assert float(gS[sb, st, 0, 0]) == 0.0, ("g_Sigmas", "the clamped entry has a gradient", (sb, st), float(gS[sb, st, 0, 0]), fam)
        assert float(gS[sb, st].diagonal()[1:].abs().min()) > 0.0 if n > 1 else True
    if want[1] == 5 and got["gQ"] is not None:
        gQ = got["gQ"]
        assert float(offdiag(gQ).max()) == 0.0, ("gQ", "not diagonal at level 5", where(offdiag(gQ) != 0), fam)
        clamped = gQ[:, 1:, jq, jq] if layout == "abc" else gQ[qb, qt, jq, jq]
        assert float(clamped.abs().max()) == 0.0, ("gQ", "the clamped entry has a gradient", (qb, qt), fam, layout)
    # ---- ws_lz = NULL: the "always recompute" path of the C ABI ----
    same = lambda a, b_: all((a[k] is None and b_[k] is None) or torch.equal(a[k], b_[k]) for k in ("terms",) + ELBO_GRADS)
    got_nows = run(ops["mus"], ops["eps"], ops["Sig"], use_ws=False)
    _elbo_compare(fam, raised, got_nows, ref, layout, free, {})
    out["ws_null_bits_equal"] = float(same(got, got_nows))
    if not free:
        assert out["ws_null_bits_equal"] == 1.0, ("ws_lz = NULL and the parked-sample path differ in bits", fam, layout, (B, T))
    # ---- sequence isolation: the t = 0 / t = T-1 neighbour fetch ----
    if B > 1:
        for b2 in sorted({0, B // 2, B - 1}):
            m2, e2, S2 = (t.clone() for t in (ops["mus"], ops["eps"], ops["Sig"]))
            dm, de, dS = draw_q(1)
            m2[b2], e2[b2], S2[b2] = r32(dm[0]), r32(de[0]), r32(dS[0])
            if bad_S is not None and sb == b2:
                S2[sb, st] = ops["Sig"][sb, st]
            other = run(m2, e2, S2)
            keep = torch.arange(B) != b2
            for k in ("terms", "ws") + ELBO_GRADS:
                if got[k] is None or (k == "ws" and want[0] != 0):
                    continue
                bad = (flat(got[k]) != flat(other[k])).any(-1) & keep[:, None]
                assert not bool(bad.any()), (k, "changed at (b,t) when sequence %d was redrawn" % b2, where(bad), fam, layout)
            changed = (flat(got["terms"])[b2] != flat(other["terms"])[b2]).any()
            assert bool(changed), "the redrawn sequence kept its bits: the isolation check checks nothing"
    return out


def _el(B, T, layout, mask_kind, prior, levels=(0, 0), pos="first", **kw):
    return dict(B=B, T=T, layout=layout, mask_kind=mask_kind, prior=prior, levels=levels, pos=pos, **kw)


ELBO_LEVELS = [(0, 0), (0, 1), (2, 0), (3, 0), (5, 0), (0, 5), (2, 5)]
_ELBO_LAYOUTS, _ELBO_MASKS, _ELBO_POS = ("abc", "abq", "plain"), (None, "ones", "t0_hidden", "last_hidden", "all_hidden", "random"), ("first", 63, 64, "last")


def _elbo_rot(k, B, T, **kw):
    """Entry k of the rotation over layouts, masks, priors, levels and positions (not their product)."""
    return _el(B, T, _ELBO_LAYOUTS[k % 3], _ELBO_MASKS[(k + k // 3) % 6], ("shared", "per_seq")[(k // 2) % 2], ELBO_LEVELS[k % 7],
               _ELBO_POS[(k + k // 7) % 4], **kw)


# thread-per-step (4,4,2): B T = 1, 2, 63, 64, 65 (T = 1: every step is a whole sequence), 63, 64, 65, 128, 129 with T > 1 (a block
# that ends mid-sequence, the ragged last block), 37 x 23 once.  The first eight shapes are also the wave-per-step (4,4,2) list.
ELBO_TPP_SHAPES = [(1, 1), (1, 2), (63, 1), (64, 1), (65, 1), (9, 7), (1, 64), (13, 5), (32, 4), (43, 3)]
ELBO_TPP_CASES = [_elbo_rot(3 * i + j, B, T) for i, (B, T) in enumerate(ELBO_TPP_SHAPES) for j in range(3)]
ELBO_TPP_CASES.append(_el(37, 23, "abq", "random", "per_seq", (2, 5), 64))
# the ONE poisoned matrix at q = 0 (Q: q = 1), 63, 64 and the last (b,t): the probe's level must arrive from every place of a block
ELBO_TPP_CASES += [_el(B, T, lay, mk, pr, lv, pos) for pos in _ELBO_POS for B, T, lay, mk, pr, lv in (
    (13, 5, "plain", "random", "shared", (2, 0)), (13, 5, "abq", None, "per_seq", (0, 1)),
    (43, 3, "abq", "t0_hidden", "shared", (5, 0)), (43, 3, "plain", "last_hidden", "per_seq", (0, 5)))]
# a shared poisoned Q, which only (b,t) = (0,1) probes; with T = 1 it is never probed and its level stays 0
ELBO_TPP_CASES += [_el(13, 5, "abc", "random", "shared", (0, 1)), _el(43, 3, "abc", None, "per_seq", (0, 5)),
                   _el(32, 4, "abc", "all_hidden", "shared", (2, 5), q_grad=False),
                   _el(63, 1, "abc", "ones", "shared", (0, 5)), _el(64, 1, "abc", "random", "per_seq", (0, 1)), _el(65, 1, "abq", None, "shared", (0, 5))]
ELBO_N4W_CASES = [c for c in ELBO_TPP_CASES if (c["B"], c["T"]) in ELBO_TPP_SHAPES[:8]]
# run-time dimensions on k_elbo_probe<RDims> / k_elbo<RDims>, B = 3, T = 1, 2, 7
ELBO_RT_DIMS = [(2, 1, 1), (5, 3, 2), (8, 8, 3), (12, 12, 2), (16, 8, 2), (16, 16, 16), (1, 1, 1)]
ELBO_RT_CASES = [dict(n=n, m=m, p=p, **_elbo_rot(3 * i + j + 1, 3, T)) for i, (n, m, p) in enumerate(ELBO_RT_DIMS) for j, T in enumerate((1, 2, 7))]
# wave-per-step (16,16,2): Sigma_s 4 bytes off a 16-byte boundary (the gate of kvae_lgssm_elbo), and the same under KVAE_N16=0
ELBO_N16W_CASES = [dict(sig_odd=True, **_elbo_rot(2 * i + 3 * j + 2, B, T)) for i, B in enumerate((1, 3)) for j, T in enumerate((1, 2, 5))]
ELBO_CASE_LISTS = {"tpp": ((4, 4, 2), ELBO_TPP_CASES), "n4w": ((4, 4, 2), ELBO_N4W_CASES), "n16w": ((16, 16, 2), ELBO_N16W_CASES),
                   "rt": (None, ELBO_RT_CASES)}


def elbo_case_id(c):
    dims = "%d-%d-%d_" % (c["n"], c["m"], c["p"]) if "n" in c else ""
    extra = "".join("_%s%s" % (k, "" if v is True else v) for k, v in c.items() if k in ("sig_odd", "q_grad", "seed"))
    return "%sB%d_T%d_%s_%s_%s_S%dQ%d_%s%s" % (dims, c["B"], c["T"], c["layout"], c["mask_kind"], c["prior"], *c["levels"], c["pos"], extra)


def run_elbo_case(DEV, fam, case, **kw):
    """One entry of ELBO_CASE_LISTS[fam] through elbo_per_step."""
    c = dict(case)
    dims = tuple(c.pop(k) for k in ("n", "m", "p")) if "n" in c else ELBO_CASE_LISTS[fam][0]
    return elbo_per_step(DEV, c.pop("B"), c.pop("T"), *dims, fam, **c, **kw)


def run_elbo_list(DEV, fam, family, **kw):
    """Every case of one list (what a child process started with KVAE_ELBO_TPP=0 or KVAE_N16=0 runs); prints and returns the
    largest ratio per key."""
    worst = {}
    for c in ELBO_CASE_LISTS[fam][1]:
        for k, v in run_elbo_case(DEV, fam, c, family=family, **kw).items():
            worst[k] = min(worst.get(k, 1.0), v) if k == "ws_null_bits_equal" else max(worst.get(k, 0.0), v)
    print("ELBO_WORST", fam, worst)
    return worst


def elbo_yardstick():
    """The measured ELBO_YARDSTICK: float32 torch against float64 torch over every case list; a ".lv" key where the raised-level
    cases differ by more than 2 x from level 0, else the larger of the two under the plain key."""
    raw = {}
    for fam in ELBO_CASE_LISTS:
        for k, v in run_elbo_list("cpu", fam, None, yardstick=True).items():
            raw[k] = max(raw.get(k, 0.0), v)
    out = {}
    for k, v in raw.items():
        if k.endswith(".lv"):
            base = raw.get(k[:-3])
            if base is None or v > 2.0 * base or v < 0.5 * base:
                out[k] = v
                if base is None:
                    out[k[:-3]] = v
            else:
                out[k[:-3]] = max(base, v)
        else:
            out.setdefault(k, v)
    return dict(sorted(out.items()))
