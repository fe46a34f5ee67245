"""Device-agnostic cases of kvae_lgssm_switching_em / lgssm_ops.switching_em_statistics / switching_em_mstep /
KalmanFilter.em_statistics / em_step / kvae.train.em.fit_dynamics_em: run against the host simulation
(tests/test_switching_em.py: the kernel bodies of csrc/lgssm_swf.h and csrc/lgssm_em.h on emulated wavefronts) and against the
gfx950 library (tests/test_gpu_switching_em.py).  The reference is lgssm_ops.switching_em_statistics_torch in FLOAT64 on the same
float32-rounded numbers; the checks of the equations themselves (Fisher's identity, the monotone likelihood) compare that
restatement with autograd of switching_log_marginal_torch and with its own likelihood, where GPB2 is exact."""
import ctypes as C
import math

import torch

from swf_cases import CASES, LONG_CASE, inputs, small_model
import swf_cases
import sws_cases

STATS = ("N", "S11", "S10", "S00", "counts", "Syz", "Szz", "Syy", "Nobs", "z0", "z0z0")   # the blocks of a row of ws, in order
SUMS = STATS + ("nseq",)
SMOOTH = sws_cases.SMOOTH
PARAMS = ("A", "B", "Q", "C", "R", "P", "mu0", "Sigma0")
# Yardsticks, by the project's standing rule (swf_cases.YARDSTICK): the largest distance of switching_em_statistics_torch in FLOAT32
# from its float64 run on the same inputs over CASES + [LONG_CASE] with seed 0, as the ratio |got - ref|_max / max(1, |ref|_max) per
# slice - "row_X": block X of one sequence's row; "sum_X": the output X summed over the sequences - measured on the CPU by
# yardsticks() (rerun: python tests/em_cases.py).  Bars = 4 x: the margin covers another summation order.
YARDSTICK = {
    "row_N": 7.16e-7, "row_S11": 7.30e-7, "row_S10": 9.03e-7, "row_S00": 5.65e-7, "row_counts": 5.30e-7, "row_Syz": 4.66e-7,
    "row_Szz": 7.34e-7, "row_Syy": 1.12e-7, "row_z0": 6.54e-7, "row_z0z0": 7.31e-7,
    "sum_N": 5.17e-7, "sum_S11": 4.93e-7, "sum_S10": 3.99e-7, "sum_S00": 3.69e-7, "sum_counts": 4.74e-7, "sum_Syz": 4.04e-7,
    "sum_Szz": 5.24e-7, "sum_Syy": 6.97e-8, "sum_z0": 4.28e-7, "sum_z0z0": 7.66e-7,
}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
EXACT = ("Nobs", "nseq")   # counts of steps and of sequences: small integers, exact in float32
# em_step (mstep_on_kernel below): the parameters after three EM iterations of the float32 restatement against the float64 ones, the
# same ratio per tensor, per case - measured on the CPU by mstep_yardsticks()
MSTEP_CASES = {"K1": ((3, 9, 1, 4, 2, True), ("A", "B", "Q", "C", "P")), "K3": ((8, 30, 3, 4, 2, True), ("A", "B", "Q", "C", "P"))}
MSTEP_ITERS = 3
MSTEP_YARDSTICK = {
    "K1": {"A": 3.12e-7, "B": 1.35e-7, "Q": 2.05e-7, "C": 2.36e-7, "P": 0.0},   # K = 1: P = [[1]] exactly
    "K3": {"A": 3.25e-7, "B": 2.15e-7, "Q": 5.61e-7, "C": 1.49e-7, "P": 6.30e-8},
}
# the model-level case (model_level below), measured the same way by model_mstep_yardsticks() with the host simulation injected
MODEL_MSTEP_YARDSTICK = {"A": 4.46e-7, "B": 4.53e-7, "Q": 2.56e-6, "C": 1.10e-8, "P": 4.80e-8}
SKIP_CASE = (2, 6, 8, 4, 1, False)   # 12 transitions over 8 regimes: the float64 N_k run from 0.158 to 5.46, all below the default
#                                      min_count = n + m + 1 = 6, five of them below 1
NOTHING_HELD = {"regimes": [], "rows": [], "B_held": [], "emission": False}


def ops():
    from kvae.kalman import lgssm_ops
    return lgssm_ops


_REF = {}


def reference(case, seed=0):
    """(args32, mask, the float64 restatement per sequence), computed once per case and shared among the tests; nobody writes to it."""
    key = (tuple(case), seed)
    if key not in _REF:
        args, mask = inputs(*case, seed=seed)
        _REF[key] = (args, mask, ops().switching_em_statistics_torch(*(a.double() for a in args), mask=mask, per_sequence=True))
    return _REF[key]


def ratio(got, ref):
    """|got - ref|_max / max(1, |ref|_max) of one slice."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def distances(rows, sums, ref):
    """The ratios of every block of the per-sequence rows (the largest over b) and of every summed output against the float64 run
    `ref` (per sequence)."""
    out = {}
    for k in STATS:
        if k not in EXACT:
            out["row_" + k] = max(ratio(rows[k][b], ref[k][b]) for b in range(ref[k].shape[0]))
            out["sum_" + k] = ratio(sums[k], ref[k].sum(0))
    return out


def run(DEV, args, mask=None, **kw):
    return ops().switching_em_statistics(*(a.to(DEV) for a in args), mask=None if mask is None else mask.to(DEV), **kw)


def run_rows(DEV, args, mask=None, **kw):
    """(the outputs, the per-sequence rows of ws as a dict of [B, ...] blocks) of one call on the kernel."""
    K, n, m = args[0].shape[0], args[0].shape[1], args[1].shape[2]
    ws = []
    got = run(DEV, args, mask, impl="hip", ws_out=ws, **kw)
    return got, ops().em_ws_blocks(ws[0], K, n, m), ws[0]


def check_stats(rows, sums, ref, tol=None, what=""):
    tol = TOL if tol is None else tol
    dist = distances(rows, sums, ref)
    for k, v in dist.items():
        print(what, k, v, "bar", tol[k])
    for k, v in dist.items():
        assert v < tol[k], (what, k, v, tol[k])
    for k in STATS:
        assert rows[k].shape == ref[k].shape and sums[k].shape == ref[k].shape[1:], k
        assert sums[k].dtype == torch.float32 and bool(torch.isfinite(sums[k]).all()) and bool(torch.isfinite(rows[k]).all()), k
    Bsz = ref["N"].shape[0]
    assert torch.equal(rows["Nobs"].cpu().double(), ref["Nobs"]) and float(sums["Nobs"]) == float(ref["Nobs"].sum())
    assert float(sums["nseq"]) == float(Bsz)
    for k in ("S11", "S00", "Szz", "z0z0"):
        assert torch.equal(rows[k], rows[k].mT) and torch.equal(sums[k], sums[k].mT), k   # mirrored from the upper triangle
    return dist


# ---- per sequence against float64; against the existing smoother ---------------------------------------------------------------
def per_sequence(DEV, case):
    """Every block of every sequence's row and every summed output against the float64 restatement under the bars; the smoother
    outputs and log_lik_seq are the bits of switching_smoother(impl="hip"); N and counts are the sums of regime_smooth and
    regime_pairs, Syz and Szz what mus_smooth / Sigmas_smooth give, within the bars."""
    args, mask, ref = reference(case)
    got, rows, _ = run_rows(DEV, args, mask)
    dist = check_stats(rows, got, ref, what=str(case))
    smo = sws_cases.run(DEV, args, mask, impl="hip")
    for k in SMOOTH + ("log_lik_seq",):
        assert torch.equal(got[k], smo[k]), k
    c = lambda t: t.detach().cpu().double()
    assert ratio(got["N"], c(smo["regime_smooth"]).sum((0, 1))) < TOL["sum_N"]
    assert ratio(got["counts"], c(smo["regime_pairs"]).sum((0, 1))) < TOL["sum_counts"]
    Y = args[8].double()
    ob = torch.ones(Y.shape[:2], dtype=torch.float64) if mask is None else (mask != 0).double()
    m_, V_ = c(smo["mus_smooth"]), c(smo["Sigmas_smooth"])
    Syz = torch.einsum("bt,btp,btn->pn", ob, Y, m_)
    Szz = torch.einsum("bt,btrc->rc", ob, V_ + m_.unsqueeze(-1) * m_.unsqueeze(-2))
    assert ratio(got["Syz"], Syz) < TOL["sum_Syz"] and ratio(got["Szz"], Szz) < TOL["sum_Szz"]
    return dist


def yardsticks():
    """The float32 torch restatement against the float64 one over CASES + [LONG_CASE]: the numbers YARDSTICK holds."""
    worst = {}
    for case in CASES + [LONG_CASE]:
        args, mask, ref = reference(case)
        f32 = ops().switching_em_statistics_torch(*args, mask=mask, per_sequence=True)
        for k, v in distances(f32, {k: f32[k].sum(0) for k in STATS}, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def identities_float64(case=(3, 12, 7, 4, 2, True)):
    """In float64: N = sum_bt regime_smooth and counts = sum_bt regime_pairs (4e-15 measured; asserted at 1e-13, a few hundred
    roundings of sums of order 10), and the statistics are the sums of their per-sequence rows."""
    args, mask, ref = reference(case)
    assert ratio(ref["N"].sum(0), ref["regime_smooth"].sum((0, 1))) < 1e-13
    assert ratio(ref["counts"].sum(0), ref["regime_pairs"].sum((0, 1))) < 1e-13
    tot = ops().switching_em_statistics_torch(*(a.double() for a in args), mask=mask)
    for k in STATS:
        assert ratio(tot[k], ref[k].sum(0)) < 1e-13, k
    assert float(tot["nseq"]) == case[0]


# ---- bits --------------------------------------------------------------------------------------------------------------------------
def bits(DEV, case=(4, 3, 3, 4, 2, True)):
    """Each output alone gives the bits of the full call and nothing else is returned; two calls give the same bits (the rows of ws
    included); the rows of a batch of 4 are the rows of its two halves; in float64 em_add of the halves is the whole to 1e-12."""
    O = ops()
    args, mask = inputs(*case, seed=3)
    full, _, ws = run_rows(DEV, args, mask)
    again, _, ws2 = run_rows(DEV, args, mask)
    assert torch.equal(ws, ws2)
    for k in SUMS + SMOOTH + ("log_lik_seq",):
        assert torch.equal(full[k], again[k]), k
    for k in SUMS + SMOOTH + ("log_lik_seq",):
        one = run(DEV, args, mask, want=(k,), impl="hip")
        assert [n for n, v in one.items() if v is not None] == [k], k
        assert torch.equal(one[k], full[k]), k
    half = lambda lo, hi: (args[:8] + (args[8][lo:hi], args[9][lo:hi]), mask[lo:hi])
    (a0, m0), (a1, m1) = half(0, 2), half(2, 4)
    g0, _, w0 = run_rows(DEV, a0, m0)
    g1, _, w1 = run_rows(DEV, a1, m1)
    assert torch.equal(torch.cat([w0, w1]), ws)                              # a sequence's row does not depend on B
    d = lambda a: tuple(t.double() for t in a)
    whole = O.switching_em_statistics_torch(*d(args), mask=mask)
    parts = O.em_add(O.switching_em_statistics_torch(*d(a0), mask=m0), O.switching_em_statistics_torch(*d(a1), mask=m1))
    for k in SUMS:
        assert ratio(parts[k], whole[k]) < 1e-12, k
    assert ratio(parts["log_lik_seq"], whole["log_lik_seq"]) < 1e-12    # batched float64 ops: not the same bits at another batch size
    added = O.em_add(g0, g1)                                                  # the kernel's halves, added in float64
    for k in STATS:
        if k not in EXACT:
            assert ratio(added[k], full[k]) < TOL["sum_" + k], k
    assert float(added["nseq"]) == 4.0 and float(added["Nobs"]) == float(full["Nobs"])


# ---- the equations: Fisher's identity, the monotone likelihood (float64 restatement only) --------------------------------------
def exact_case(name, R_scale=1.0):
    """(args64, mask) of the cases where GPB2 is exact: "K1" (3, 9), "K1_open" the same unmasked, "identity" P = I at (2, 6, 3),
    "shared" shared A / B / Q at (2, 7, 3); R = 0.05 R_scale I."""
    if name in ("K1", "K1_open"):
        args, mask = inputs(3, 9, 1, masked=name == "K1", seed=4)
    elif name == "identity":
        args, mask = inputs(2, 6, 3, masked=True, seed=4)
        args = args[:5] + (torch.eye(3),) + args[6:]
    elif name == "shared":
        args, mask = inputs(2, 7, 3, masked=True, seed=4, shared=True)
    else:
        raise KeyError(name)
    args = [a.double() for a in args]
    args[4] = args[4] * R_scale
    return tuple(args), mask


def expected_complete_loglik(stats, A, Bm, Q, Cm, R, P, mu0, Sigma0):
    """Q(theta; stats) up to constants in theta: the regimes' dynamics, the emission, the transitions and the initial state."""
    F = torch.cat([A, Bm], -1)
    quad = stats["S11"] - F @ stats["S10"].mT - stats["S10"] @ F.mT + F @ stats["S00"] @ F.mT
    val = -0.5 * (stats["N"] * torch.logdet(Q)).sum() - 0.5 * torch.einsum("kij,kji->", torch.linalg.inv(Q), quad)
    eq = stats["Syy"] - Cm @ stats["Syz"].mT - stats["Syz"] @ Cm.mT + Cm @ stats["Szz"] @ Cm.mT
    val = val - 0.5 * stats["Nobs"].sum() * torch.logdet(R) - 0.5 * torch.trace(torch.linalg.inv(R) @ eq)
    live = stats["counts"] > 0
    val = val + (stats["counts"] * torch.where(live, P, torch.ones_like(P)).log()).sum()
    ns = stats["nseq"].sum()
    q0 = stats["z0z0"] - torch.outer(stats["z0"], mu0) - torch.outer(mu0, stats["z0"]) + ns * torch.outer(mu0, mu0)
    return val - 0.5 * ns * torch.logdet(Sigma0) - 0.5 * torch.trace(torch.linalg.inv(Sigma0) @ q0)


def fisher_residuals(name, R_scale):
    """Fisher's identity at theta = theta_old: the gradient of Q(theta; stats(theta_old)) against autograd of log p(a | u)
    (switching_log_marginal_torch), for A, B, Q, C, mu0, Sigma0: {name: |g_Q - g_ll|_max / |g_ll|_max}.  Q and Sigma0 enter both
    sides through their symmetric part."""
    O = ops()
    args, mask = exact_case(name, R_scale)
    stats = O.switching_em_statistics_torch(*args, mask=mask)
    stats = {k: stats[k] for k in SUMS}
    names = ("A", "B", "Q", "C", "R", "P", "mu0", "Sigma0")
    diff = ("A", "B", "Q", "C", "mu0", "Sigma0")

    def leaves():
        th = {k: v.clone().requires_grad_(k in diff) for k, v in zip(names, args[:8])}
        sym = {k: (0.5 * (v + v.mT) if k in ("Q", "Sigma0") else v) for k, v in th.items()}
        return th, sym

    th, sym = leaves()
    expected_complete_loglik(stats, *(sym[k] for k in names)).backward()
    gq = {k: th[k].grad for k in diff}
    th, sym = leaves()
    O.switching_log_marginal_torch(*(sym[k] for k in names), args[8], args[9], mask=mask)["seq_ll"].sum().backward()
    return {k: float((gq[k] - th[k].grad).abs().max() / th[k].grad.abs().max()) for k in diff}


def fisher(name):
    """<= 1e-4 at R = 0.05 I and <= 1e-6 at R = 5 I: the residual is the 1e-6 jitter inside the density (it falls as 1 / R), not the
    recursion."""
    for scale, bar in ((1.0, 1e-4), (100.0, 1e-6)):
        res = fisher_residuals(name, scale)
        print(name, "R x", scale, res)
        for k, v in res.items():
            assert v <= bar, (name, scale, k, v)


def em_iterate(args, mask_batches, iters, update, dtype, stat_fn=None):
    """`iters` EM iterations through the restatement in `dtype` over one or several batches [(Y, U, mask), ...] with the starting
    parameters args[:8] - what KalmanFilter.em_step / fit_dynamics_em do, parameters kept in `dtype` between iterations.  Returns
    (the final parameters as a dict, the log-likelihood history, the skipped lists of every iteration)."""
    O = ops()
    th = {k: v.to(dtype) for k, v in zip(PARAMS, args[:8])}
    hist, skipped = [], []
    for _ in range(iters):
        tot = None
        for Y, U, mask in mask_batches:
            st = O.switching_em_statistics_torch(*(th[k] for k in PARAMS), Y.to(dtype), U.to(dtype), mask=mask, want=SUMS + ("log_lik_seq",))
            tot = st if tot is None else O.em_add(tot, st)
        new, sk = O.switching_em_mstep(tot, th, update)
        th = {k: v.to(dtype) for k, v in new.items()}
        hist.append(float(tot["log_lik_seq"].double().sum()))
        skipped.append(sk)
    return th, hist, skipped


def monotone(name, update, iters=5):
    """EM cannot lower the exact likelihood where inference is exact: every step of `iters` + 1 evaluations rises."""
    args, mask = exact_case(name)
    _, hist, _ = em_iterate(args, [(args[8], args[9], mask)], iters + 1, update, torch.float64)
    steps = [b - a for a, b in zip(hist, hist[1:])]
    print(name, "log-likelihood", hist, "smallest step", min(steps))
    assert len(steps) == iters and all(s > 0 for s in steps), hist
    return min(steps)


EVERYTHING = ("A", "B", "Q", "C", "R", "P", "mu0", "Sigma0")


def gpb2_monotone_report():
    """Not a theorem and not asserted: the smallest step on the general GPB2 cases."""
    out = {}
    for case in ((3, 12, 3), (4, 20, 2), (8, 30, 3)):
        args, mask = inputs(*case, masked=True, seed=4)
        _, hist, _ = em_iterate(args, [(args[8], args[9], mask)], 6, EVERYTHING, torch.float64)
        out[case] = min(b - a for a, b in zip(hist, hist[1:]))
    return out


# ---- em_step on the kernel ---------------------------------------------------------------------------------------------------------
def make_filter(args, DEV):
    """A KalmanFilter over switching dynamics that holds the parameters args[:8]."""
    from kvae.kalman.kalman_filter import KalmanFilter
    from kvae.kalman.switch_dyn_param import StickyRegimePrior, SwitchingDynamicsParameter
    A, Bm, Q, Cm, R, P, mu0, Sigma0 = args[:8]
    K = A.shape[0]
    prior = StickyRegimePrior(K)
    prior.transition_matrix = P.clone()
    torch.manual_seed(0)
    dyn = SwitchingDynamicsParameter(A, Bm, Cm.expand(K, *Cm.shape).clone(), Q, prior=prior)
    kf = KalmanFilter(1.0, 1.0, mu0, Sigma0, dyn)
    kf.R.copy_(R)
    return kf.to(DEV)


def filter_params(kf):
    dyn = kf.dyn_params
    c = lambda t: t.detach().cpu().clone()
    return dict(A=c(dyn.A), B=c(dyn.B), Q=c(dyn.Q), C=c(dyn.C[0]), R=c(kf.R), P=c(dyn.prior.transition_matrix), mu0=c(kf.mu0),
                Sigma0=c(kf.Sigma0))


def mstep_distances(got, ref, update):
    return {k: ratio(got[k], ref[k]) for k in update}


def mstep_yardsticks():
    out = {}
    for name, (case, update) in MSTEP_CASES.items():
        args, mask = inputs(*case, seed=4)
        batch = [(args[8], args[9], mask)]
        ref, _, _ = em_iterate(args, batch, MSTEP_ITERS, update, torch.float64)
        f32, _, _ = em_iterate(args, batch, MSTEP_ITERS, update, torch.float32)
        out[name] = mstep_distances(f32, ref, update)
    return out


def mstep_on_kernel(DEV, name):
    """Three em_step iterations on the kernel against the float64 M-step of the float64 statistics, per tensor; what is not named in
    `update` keeps its bits; at K = 1 (exact inference) log_lik rises at every iteration."""
    case, update = MSTEP_CASES[name]
    args, mask = inputs(*case, seed=4)
    ref, _, _ = em_iterate(args, [(args[8], args[9], mask)], MSTEP_ITERS, update, torch.float64)
    kf = make_filter(args, DEV)
    start = filter_params(kf)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    lls = []
    for _ in range(MSTEP_ITERS):
        out = kf.em_step(Y, U, mk, update=update)
        assert set(out) == {"log_lik", "stats", "skipped"} and out["skipped"] == NOTHING_HELD
        lls.append(float(out["log_lik"]))
    lls.append(float(kf.em_statistics(Y, U, mk, want=("log_lik_seq",))["log_lik_seq"].double().sum()))
    got = filter_params(kf)
    dist = mstep_distances(got, ref, update)
    for k, v in dist.items():
        print(name, k, v, "bar", 4.0 * MSTEP_YARDSTICK[name][k])
    for k, v in dist.items():
        assert v <= 4.0 * MSTEP_YARDSTICK[name][k], (name, k, v)
    for k in PARAMS:
        if k not in update:
            assert torch.equal(got[k], start[k]), k
        else:
            assert not torch.equal(got[k], start[k]) or (k == "P" and case[2] == 1), k
    assert bool(torch.equal(kf.dyn_params._prior_matrix(torch.device(DEV), torch.float32).cpu(), got["P"]))   # the cache was rebuilt
    if case[2] == 1:
        assert all(b > a for a, b in zip(lls, lls[1:])), lls
    return dist


def skipped_regimes(DEV):
    """SKIP_CASE: 12 transitions over 8 regimes.  With the default min_count = n + m + 1 every regime keeps its parameters; with
    min_count = 1 the regimes whose expected visits fall below it (the float64 route names them; none within 1e-3 of the threshold)
    keep the bits of their A_k, B_k, Q_k and are named in `skipped`, the others move; with min_count = 0 nobody is skipped."""
    args, mask = inputs(*SKIP_CASE)
    K = SKIP_CASE[2]
    N64 = ops().switching_em_statistics_torch(*(a.double() for a in args), mask=mask, want=("N",))["N"]
    print("N", N64.tolist())
    assert 0.15 < float(N64.min()) < 0.16 and float((N64 - 1.0).abs().min()) > 1e-3
    low = [k for k in range(K) if float(N64[k]) < 1.0]
    assert low and len(low) < K, low
    Y, U = args[8].to(DEV), args[9].to(DEV)
    kf = make_filter(args, DEV)
    start = filter_params(kf)
    out = kf.em_step(Y, U, update=("A", "B", "Q"))
    assert out["skipped"] == dict(NOTHING_HELD, regimes=list(range(K))), out["skipped"]
    assert all(torch.equal(v, start[k]) for k, v in filter_params(kf).items())
    out = kf.em_step(Y, U, update=("A", "B", "Q"), min_count=1.0)
    assert out["skipped"] == dict(NOTHING_HELD, regimes=low), (out["skipped"], low)
    got = filter_params(kf)
    for k in range(K):
        for name in ("A", "B", "Q"):
            assert torch.equal(got[name][k], start[name][k]) == (k in low), (name, k)
    for name in ("C", "R", "P", "mu0", "Sigma0"):
        assert torch.equal(got[name], start[name]), name
    kf = make_filter(args, DEV)
    assert kf.em_step(Y, U, update=("A", "B", "Q"), min_count=0.0)["skipped"]["regimes"] == []
    # a row of P without counts keeps its values: regime 2 is never left when nobody enters it
    O = ops()
    stats = {k: v.clone() for k, v in out["stats"].items() if v is not None}
    stats["counts"][2] = 0.0
    new, sk = O.switching_em_mstep(stats, start, ("P",))
    assert sk == dict(NOTHING_HELD, rows=[2]) and torch.equal(new["P"][2].cpu(), start["P"][2].double())
    assert float((new["P"].sum(1) - 1.0).abs().max()) < 1e-6 and float((new["P"][:2].sum(1) - 1.0).abs().max()) < 1e-12


# ---- without a control input; degenerate statistics ------------------------------------------------------------------------------
def no_controls_float64():
    """u = 0 makes the u-block of every S00_k exactly singular: the default update holds B_k (named under "B_held"), fits A_k given
    it, and - K = 1, where inference is exact - the likelihood still rises at every step; update=("B",) alone changes nothing."""
    O = ops()
    args, mask = exact_case("K1")
    args = args[:9] + (torch.zeros_like(args[9]),)
    th, hist, skipped = em_iterate(args, [(args[8], args[9], mask)], 6, EVERYTHING, torch.float64)
    assert all(sk == dict(NOTHING_HELD, B_held=[0]) for sk in skipped), skipped
    assert torch.equal(th["B"], args[1]) and not torch.equal(th["A"], args[0]) and not torch.equal(th["Q"], args[2])
    steps = [b - a for a, b in zip(hist, hist[1:])]
    print("u = 0: log-likelihood", hist)
    assert all(s_ > 0 for s_ in steps), hist
    args3, mask3 = inputs(3, 12, 3, masked=True, seed=4)
    args3 = tuple(a.double() for a in args3[:9]) + (torch.zeros_like(args3[9]).double(),)
    stats = O.switching_em_statistics_torch(*args3, mask=mask3)
    old = dict(zip(PARAMS, args3[:8]))
    new, sk = O.switching_em_mstep(stats, old)
    assert sk == dict(NOTHING_HELD, B_held=[0, 1, 2]) and torch.equal(new["B"], old["B"])
    assert all(bool(torch.isfinite(v).all()) for v in new.values())
    only_a, sk_a = O.switching_em_mstep(stats, old, ("A", "Q", "C", "P"))
    assert sk_a == NOTHING_HELD
    for k in ("A", "Q", "C", "P"):
        assert ratio(new[k], only_a[k]) < 1e-12, k                            # holding B is the A-only maximiser
    same, sk_b = O.switching_em_mstep(stats, old, ("B",))
    assert sk_b == dict(NOTHING_HELD, B_held=[0, 1, 2]) and all(torch.equal(same[k], old[k]) for k in PARAMS)


def degenerate_statistics():
    """No observed step: C and R keep their values and "emission" says so; a regime with a NaN in its statistics is skipped;
    statistics that lack log_lik_seq: em_step returns
    log_lik = None."""
    O = ops()
    args, _ = inputs(2, 4, 2, seed=4)
    args = tuple(a.double() for a in args)
    stats = O.switching_em_statistics_torch(*args, mask=torch.zeros(2, 4))
    assert float(stats["Nobs"]) == 0.0
    old = dict(zip(PARAMS, args[:8]))
    new, sk = O.switching_em_mstep(stats, old, ("C", "R"))
    assert sk == dict(NOTHING_HELD, emission=True) and torch.equal(new["C"], old["C"]) and torch.equal(new["R"], old["R"])
    full = O.switching_em_statistics_torch(*args)
    broken = {k: full[k].clone() for k in SUMS}
    broken["S00"][1, 0, 0] = float("nan")                                     # non-finite statistics of one regime: skipped, not raised
    new, sk = O.switching_em_mstep(broken, old, min_count=0.0)
    assert sk == dict(NOTHING_HELD, regimes=[1]) and all(torch.equal(new[k][1], old[k][1]) for k in ("A", "B", "Q"))
    assert all(bool(torch.isfinite(v).all()) for v in new.values()) and not torch.equal(new["A"][0], old["A"][0])
    kf = make_filter(args[:8], "cpu")
    out = kf.em_step(None, None, stats={k: full[k] for k in SUMS}, min_count=0.0)
    assert out["log_lik"] is None and out["skipped"] == NOTHING_HELD


def no_controls_model(DEV, K=3, B=3, T=12):
    """fit_dynamics_em without controls (u = None is zeros, as in forward()): runs, holds every B_k and says nothing else was
    skipped, moves A and Q, and its likelihood history is the float64 route's to 1e-4 relative."""
    model, x, mask, _, _ = swf_cases._model_case(DEV, K, B, T)
    before = filter_params(model.kalman_filter)
    u0 = torch.zeros(B, T, model.u_dim)
    _, hist64, sk64 = _model_route(model, [(x, u0, mask)], torch.float64)
    assert all(sk == dict(NOTHING_HELD, B_held=list(range(K))) for sk in sk64), sk64
    hist = model.fit_dynamics_em([(x, None, mask.to(DEV))], 2)
    again = model.kalman_filter.em_step(model.encode_sequence(x, sample=False)[0].detach(), u0.to(DEV))
    assert again["skipped"] == dict(NOTHING_HELD, B_held=list(range(K))), again["skipped"]
    assert len(hist) == 2 and all(math.isfinite(v) for v in hist)
    assert all(abs(a - b) <= 1e-4 * max(1.0, abs(b)) for a, b in zip(hist, hist64)), (hist, hist64)
    after = filter_params(model.kalman_filter)
    assert torch.equal(after["B"], before["B"]) and not torch.equal(after["A"], before["A"]) and not torch.equal(after["Q"], before["Q"])
    assert all(bool(torch.isfinite(v).all()) for v in after.values())


# ---- routing -------------------------------------------------------------------------------------------------------------------
def routing(DEV):
    """K = 9, n = 5 and float64 are outside the kernel: the Python layer takes switching_em_statistics_torch, impl="hip" raises; a
    carried state raises."""
    import pytest
    O = ops()
    ok = torch.zeros(1, device=DEV)
    S = O.switching_em_supported
    assert S(8, 4, 4, 2, ok) and S(1, 1, 1, 2, ok)
    assert not S(9, 4, 4, 2, ok) and not S(3, 5, 2, 2, ok) and not S(3, 4, 5, 2, ok) and not S(3, 4, 2, 3, ok)
    assert not S(3, 4, 2, 2, ok.double())
    for case, dt in (((2, 4, 9, 4, 2, False), torch.float32), ((2, 4, 3, 5, 2, True), torch.float32), ((2, 4, 3, 4, 2, True), torch.float64)):
        args, mask = inputs(*case, seed=8)
        args = tuple(a.to(dt) for a in args)
        got = run(DEV, args, mask)
        ref = O.switching_em_statistics_torch(*(a.double() for a in args), mask=mask)
        same = O.switching_em_statistics_torch(*args, mask=mask)
        for k in SUMS:
            assert got[k].dtype == dt
            assert ratio(got[k], ref[k]) < 1e-4, k
            if DEV == "cpu":
                assert torch.equal(got[k], same[k]), k                       # the restatement itself
        with pytest.raises(ValueError, match="impl='hip'"):
            run(DEV, args, mask, impl="hip")
    args, mask = inputs(2, 3, 2)
    with pytest.raises(ValueError):
        run(DEV, args, mask, want=("regimes",))
    with pytest.raises(ValueError):
        run(DEV, args, mask, impl="kernel")
    st = swf_cases.run(DEV, args, mask, impl="hip")["state"]
    with pytest.raises(ValueError, match="state"):
        run(DEV, args, mask, state=st)
    forced = run(DEV, args, mask, impl="torch")
    assert ratio(forced["S10"], run(DEV, args, mask)["S10"]) < 1e-4


def host_tensors_take_the_restatement():
    """Without a backend for host tensors (the GPU tier: nothing injected) the op on CPU tensors is the restatement, and impl="hip"
    raises."""
    import pytest
    O = ops()
    args, mask = inputs(2, 3, 2)
    a = O.switching_em_statistics(*args, mask=mask)
    b = O.switching_em_statistics_torch(*args, mask=mask)
    assert all(torch.equal(a[k], b[k]) for k in SUMS)
    with pytest.raises(ValueError, match="impl='hip'"):
        O.switching_em_statistics(*args, mask=mask, impl="hip")


# ---- the C ABI through raw pointers ------------------------------------------------------------------------------------------
def c_abi(lib, DEV, launches=None):
    """Every error code of include/kvae_lgssm.h, and under each not a byte of any output, of the history or of ws written; then which
    launches a call makes (launches: a function returning the counters [forward, backward, reduction, sequence sums], host
    simulation only)."""
    from kvae import _native as N
    B, T, K, n, m = 2, 3, 3, 4, 2
    args, mask = inputs(B, T, K, n, m, masked=True)
    names = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")
    ins = dict(zip(names, (a.to(DEV).contiguous() for a in args)), mask=mask.to(DEV))
    # buffers large enough for the shapes the failing calls claim (K = 9, n = m = 5) too
    big = lambda *s, dt=torch.float32: torch.full(s, 7, device=DEV, dtype=dt)
    fouts = dict(regime_filt=big(B, T, 9), regime_pred=big(B, T, 9), ll=big(B, T), seq_ll=big(B), a_pred=big(B, T, 3), S_out=big(B, T, 3, 3),
                 mus_filt=big(B, T, 5), Sigmas_filt=big(B, T, 5, 5), levels=big(B, T, dt=torch.int32), out_log_w=big(B, 9),
                 out_mu=big(B, 9, 5), out_Sigma=big(B, 9, 5, 5))
    hist = dict(hist_mu=big(B, T, 9, 5), hist_Sigma=big(B, T, 9, 5, 5), hist_W=big(B, T, 9, 9), hist_w=big(B, 9))
    souts = dict(regime_smooth=big(B, T, 9), regime_pairs=big(B, T, 9, 9), mus_smooth=big(B, T, 5), Sigmas_smooth=big(B, T, 5, 5))
    G = 9 * (1 + 25 + 50 + 100) + 81 + 10 + 25 + 4 + 1 + 5 + 25
    eouts = dict(ws=big(B, G), N=big(9), S11=big(9, 5, 5), S10=big(9, 5, 10), S00=big(9, 10, 10), counts=big(9, 9), Syz=big(2, 5), Szz=big(5, 5),
                 Syy=big(2, 2), Nobs=big(1), z0=big(5), z0z0=big(5, 5), nseq=big(1))
    st = dict(state_log_w=torch.zeros(B, 9, device=DEV), state_mu=torch.zeros(B, 9, 5, device=DEV),
              state_Sigma=torch.eye(5, device=DEV).repeat(B, 9, 1, 1))
    assert lib.dll.kvae_lgssm_switching_em_ws_floats(B, K, n, m) == B * (K * (1 + 16 + 24 + 36) + 9 + 8 + 16 + 4 + 1 + 4 + 16)
    assert lib.dll.kvae_lgssm_switching_em_ws_floats(0, K, n, m) == 0

    def call(drop=(), no_stats=False, **kw):
        pr, es = N.SwsProblem(), N.EmStats()
        f = pr.filt
        f.B, f.T, f.K, f.n, f.m, f.p = B, T, K, n, m, 2
        for k, v in list(ins.items()) + list(fouts.items()):
            if k not in drop:
                setattr(f, k, v.data_ptr())
        for k, v in list(hist.items()) + list(souts.items()):
            if k not in drop:
                setattr(pr, k, v.data_ptr())
        for k, v in eouts.items():
            if k not in drop:
                setattr(es, k, v.data_ptr())
        for k, v in kw.items():
            setattr(f, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        rc = lib.dll.kvae_lgssm_switching_em(C.byref(pr), None if no_stats else C.byref(es), None)
        if DEV != "cpu":
            torch.cuda.synchronize()
        return rc

    everything = list(fouts.values()) + list(hist.values()) + list(souts.values()) + list(eouts.values())
    untouched = lambda: all(bool((v == 7).all()) for v in everything)
    count = launches if launches is not None else (lambda: [0, 0, 0, 0])
    before = count()
    assert lib.dll.kvae_lgssm_switching_em(None, None, None) == 2
    for k in names + tuple(hist) + ("ws",):
        assert call(drop=(k,)) == 2, k                                      # KVAE_ERR_NULL
    assert call(no_stats=True) == 2 and call(drop=("ll",)) == 2             # no stats struct; seq_ll reads ll
    for kw in (dict(B=0), dict(T=0), dict(B=-1)):
        assert call(**kw) == 1, kw                                          # KVAE_ERR_DIMS
    for kw in (dict(K=9), dict(K=0), dict(n=5), dict(n=0), dict(m=5), dict(p=3), dict(p=1)):
        assert call(**kw) == 4, kw                                          # KVAE_ERR_ARG
    assert call(state_log_w=st["state_log_w"]) == 4 and call(state_mu=st["state_mu"], state_Sigma=st["state_Sigma"]) == 4
    assert call(drop=("mu0", "Sigma0"), **st) == 4                          # a carried state is not accepted
    assert untouched() and count() == before
    stats = tuple(k for k in eouts if k != "ws")
    assert call() == 0
    if launches is not None:
        assert [a - b for a, b in zip(count(), before)] == [1, 1, 1, 1]    # one forward, one backward, one reduction (and seq_ll)
        before = count()
        assert call(drop=stats + ("seq_ll",)) == 0
        assert [a - b for a, b in zip(count(), before)] == [1, 1, 0, 0]    # the smoother outputs alone: no reduction
        before = count()
        assert call(drop=stats + tuple(souts) + ("seq_ll",)) == 0
        assert [a - b for a, b in zip(count(), before)] == [1, 0, 0, 0]    # filter outputs alone
        before = count()
        assert call(drop=stats[1:] + tuple(souts) + tuple(fouts)) == 0
        assert [a - b for a, b in zip(count(), before)] == [1, 1, 1, 0]    # one statistic alone
    assert call(drop=("mask",)) == 0 and call(T=1) == 0
    assert not any(bool((v.reshape(-1)[:1] == 7).all()) for v in everything)


# ---- model level -----------------------------------------------------------------------------------------------------------------
MODEL_UPDATE = ("A", "B", "Q", "C", "P")


def _model_batches(DEV, K=3, B=3, T=12):
    model, x, mask, u, g = swf_cases._model_case(DEV, K, B, T)
    x2 = (torch.rand(B, T, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    u2 = (0.3 * torch.randn(B, T, model.u_dim, generator=g)).to(DEV)
    return model, [(x, u, mask.to(DEV)), (x2, u2, mask.to(DEV))], g


def _model_route(model, batches, dtype, iters=2):
    """fit_dynamics_em restated: the batches encoded by the model as it stands, then em_iterate in `dtype` on the host."""
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu()
    was = model.training
    model.eval()
    with torch.no_grad():
        enc = [(d(model.encode_sequence(x, sample=False)[0]), d(u), d(mask)) for x, u, mask in batches]
    model.train(was)
    args = (d(dyn.A), d(dyn.B), d(dyn.Q), d(dyn.C[0]), d(kf.R), dyn.prior.transition_matrix.clone(), d(kf.mu0), d(kf.Sigma0))
    return em_iterate(args, enc, iters, MODEL_UPDATE, dtype)


def model_mstep_yardsticks(DEV="cpu"):
    model, batches, _ = _model_batches(DEV)
    ref, _, _ = _model_route(model, batches, torch.float64)
    f32, _, _ = _model_route(model, batches, torch.float32)
    return mstep_distances(f32, ref, MODEL_UPDATE)


def model_level(DEV, K=3, B=3, T=12):
    """fit_dynamics_em over two batches for two iterations against the float64 route; the state_dict keeps its keys, the encoder,
    the decoder and the regime posterior network keep their bits, forward() under injected noise is bit-identical before and after a
    statistics call; training mode and tau are left as they were."""
    from kvae import noise
    model, batches, g = _model_batches(DEV, K, B, T)
    model.train()
    dyn = model.kalman_filter.dyn_params
    dyn.tau = 0.37
    x, u, mask = batches[0]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    nz = dict(eps_a=torch.randn(B * T, model.a_dim, generator=g).to(DEV), eps_z=torch.randn(B, T, model.z_dim, generator=g).to(DEV),
              gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV))
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_before = model(x, u=u)
        a = model.encode_sequence(x, sample=False)[0]
    st = model.kalman_filter.em_statistics(a, u, mask)
    assert all(st[k] is not None for k in SUMS + SMOOTH + ("log_lik_seq",))
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    with torch.no_grad():
        with noise.inject(**nz):
            fwd_after = model(x, u=u)
    for k in ("state_probs", "mus_smooth", "Sigmas_smooth", "a_samples", "x_logits"):
        assert torch.equal(fwd_before[k], fwd_after[k]), k
    ref, hist64, _ = _model_route(model, batches, torch.float64)
    hist = model.fit_dynamics_em(batches, 2, update=MODEL_UPDATE)
    assert len(hist) == 2 and all(isinstance(v, float) and math.isfinite(v) for v in hist)
    assert all(abs(a - b) <= 1e-4 * max(1.0, abs(b)) for a, b in zip(hist, hist64)), (hist, hist64)
    assert model.training and dyn.tau == 0.37
    after = model.state_dict()
    assert list(after) == list(before)
    moved = ("kalman_filter.dyn_params.A", "kalman_filter.dyn_params.B", "kalman_filter.dyn_params.Q", "kalman_filter.dyn_params.C")
    for k, v in after.items():
        assert torch.equal(v, before[k]) == (k not in moved), k              # encoder, decoder, posterior network, R, mu0, Sigma0
    got = filter_params(model.kalman_filter)
    dist = mstep_distances(got, ref, MODEL_UPDATE)
    for k, v in dist.items():
        print("model", k, v, "bar", 4.0 * MODEL_MSTEP_YARDSTICK[k])
    for k, v in dist.items():
        assert v <= 4.0 * MODEL_MSTEP_YARDSTICK[k], (k, v)
    return dist


def model_errors(DEV):
    import pytest
    lstm = small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    Y, U = torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 3, 4, device=DEV)
    with pytest.raises(ValueError, match="fit_dynamics_em"):
        lstm.fit_dynamics_em([x], 1)
    with pytest.raises(ValueError, match="em_step"):
        lstm.kalman_filter.em_step(Y, U)
    with pytest.raises(ValueError, match="em_statistics"):
        lstm.kalman_filter.em_statistics(Y, U)
    model = small_model("switching").to(DEV)
    for bad in ((x, None, torch.ones(2, 4)), (x, torch.zeros(2, 4, 4))):
        with pytest.raises(ValueError):
            model.fit_dynamics_em([bad], 1)
    with pytest.raises(ValueError):
        model.fit_dynamics_em([], 1)
    with pytest.raises(ValueError):
        model.kalman_filter.em_step(Y, U, update=("A", "alpha"))


if __name__ == "__main__":
    print("YARDSTICK", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print("MSTEP_YARDSTICK", {n: {k: float(f"{v:.3g}") for k, v in d.items()} for n, d in mstep_yardsticks().items()})
    print("GPB2 monotone (smallest step)", gpb2_monotone_report())
