"""Device-agnostic cases of kvae_regime_decode / lgssm_ops.regime_decode / KVAE.decode_regimes: run against the host simulation
(tests/test_regime_decode.py: the lane-grid body on emulated wavefronts, the LDS body as the simulation runs it) and against the
gfx950 library (tests/test_gpu_regime_decode.py).  The reference is lgssm_ops.regime_decode_torch in FLOAT64 on the same numbers;
the brute-force case is independent of it (all K^T paths enumerated)."""
import itertools
import math

import torch

from golden_util import rel_err
from parity_cases import _per_step_ratio

# (B, T, K) of the per-step parity, both tiers
SHAPES = [
    (3, 37, 7),    # the grid body with ragged K
    (2, 9, 3),
    (5, 1, 8),     # T = 1: no transition logits are read, path = argmax of init, kl has only kl_0
    (2, 2, 8),     # full grid; the prefetch has no next step
    (2, 33, 9),    # the LDS body at its smallest ...
    (3, 21, 16),   # ... and largest K
    (4, 5, 1),     # K = 1
    (65, 6, 4),    # more workgroups than one wavefront's worth of sequences
]
# beyond the list above: more steps than the 64 backpointer words one pass of the backtrace reads back, for both bodies.  They are
# held to the bars measured on SHAPES (they would only widen them).
LONG_SHAPES = [(2, 70, 5), (2, 67, 12)]
# Yardsticks, by the rule of parity_cases.RNN_YARDSTICK: the largest per-slice ratio (parity_cases._per_step_ratio: per (b,t) for
# marginals and kl, per b for path_logq) of regime_decode_torch in FLOAT32 against its float64 run, over SHAPES with seed 0 - the
# case list of both tiers (rerun: python tests/regime_decode_cases.py).  Bars = 4 x: the margin covers another summation order.
# Largest ratios the kernel reaches against the same float64 run (LONG_SHAPES included), host simulation | gfx950:
#   marginals 3.7e-7 | 3.5e-7    kl 2.0e-6 | 2.7e-6    path_logq 2.7e-7 | 2.1e-7      
YARDSTICK = {"marginals": 3.22e-7, "kl": 3.05e-6, "path_logq": 1.25e-7}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}
GAP = 1e-4   # a float64 decision gap (best minus runner-up) above which float32 must take the same decision


def prior(K, p_stay=0.8):
    from kvae.kalman.switch_dyn_param import StickyRegimePrior
    return StickyRegimePrior(K, p_stay).transition_matrix


def inputs(B, T, K, seed=0):
    """logits [B,T,K,K], init [B,K] drawn in float64 and rounded through float32 (the float64 reference starts from the same
    numbers), and the sticky prior P (p_stay = 0.8)."""
    g = torch.Generator().manual_seed(10000 * seed + 1000 * B + 10 * T + K)
    logits = torch.randn(B, T, K, K, generator=g, dtype=torch.float64)
    init = torch.randn(B, K, generator=g, dtype=torch.float64)
    return logits.float(), init.float(), prior(K)


def decision_gaps(logits, init):
    """Smallest float64 decision gap of each sequence [B]: best minus runner-up over i in every backpointer (t, j) and over j in
    the final argmax (inf where K = 1)."""
    B, T, K, _ = logits.shape
    gap = torch.full((B,), math.inf, dtype=torch.float64)
    if K == 1:
        return gap
    d = torch.log_softmax(init, -1)
    for t in range(1, T):
        cand = d.unsqueeze(-1) + torch.log_softmax(logits[:, t], -1)   # [B, i, j]
        top = cand.topk(2, dim=1).values
        gap = torch.minimum(gap, (top[:, 0] - top[:, 1]).amin(-1))
        d = top[:, 0]
    top = d.topk(2, dim=-1).values
    return torch.minimum(gap, top[:, 0] - top[:, 1])


def path_log_q(path, logits, init):
    """log q(s_{0:T-1}) of a given path [B,T], in the dtype of the logits."""
    B, T = path.shape
    lq = torch.log_softmax(init, -1).gather(1, path[:, :1]).squeeze(1)
    for t in range(1, T):
        row = torch.log_softmax(logits[:, t], -1)[torch.arange(B), path[:, t - 1]]
        lq = lq + row.gather(1, path[:, t:t + 1]).squeeze(1)
    return lq


_REF = {}


def reference(B, T, K, seed=0, p_stay=0.8):
    """(logits32, init32, P, float64 restatement, decision gaps), computed once per case and shared."""
    key = (B, T, K, seed, p_stay)
    if key not in _REF:
        from kvae.kalman import lgssm_ops
        logits, init, _ = inputs(B, T, K, seed)
        P = prior(K, p_stay)
        ref = lgssm_ops.regime_decode_torch(logits.double(), init.double(), P.double())
        _REF[key] = (logits, init, P, ref, decision_gaps(logits.double(), init.double()))
    return _REF[key]


def check_outputs(got, logits, init, ref, gaps, out=None):
    """All four outputs of one call against the float64 run: marginals and kl per (b,t), path_logq per b, under TOL; the path of
    EVERY sequence within the path_logq bar of the optimum, and equal to the float64 path wherever every decision gap exceeds
    GAP - which must be every sequence."""
    out = {} if out is None else out
    c = lambda t: t.detach().cpu()
    for name, g, r in (("marginals", got["marginals"], ref["marginals"]), ("kl", got["kl"].unsqueeze(-1), ref["kl"].unsqueeze(-1)),
                       ("path_logq", got["path_logq"][:, None, None], ref["path_logq"][:, None, None])):
        ratio, where = _per_step_ratio(c(g), r)
        out[name] = max(out.get(name, 0.0), ratio)
        print(name, tuple(logits.shape), ratio, where)
        assert ratio < TOL[name], (name, ratio, where, TOL[name])
    path = c(got["path"])
    assert path.dtype == torch.int64 and path.shape == ref["path"].shape
    K = logits.shape[2]
    assert int(path.min()) >= 0 and int(path.max()) < K
    opt = ref["path_logq"]
    mine = path_log_q(path, logits.double(), init.double())
    short = ((opt - mine).abs() / opt.abs().clamp_min(1.0))
    print("path", tuple(logits.shape), "short of the optimum", float(short.max()), "smallest gap", float(gaps.min()))
    assert bool((short < TOL["path_logq"]).all()), short
    decided = gaps > GAP
    assert float((~decided).double().mean()) == 0.0, gaps   # no sequence is left out of the comparison
    assert torch.equal(path[decided], ref["path"][decided])
    return out


def per_step(DEV, B, T, K, seed=0):
    from kvae.kalman import lgssm_ops
    logits, init, P, ref, gaps = reference(B, T, K, seed)
    got = lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV))
    return check_outputs(got, logits, init, ref, gaps)


def yardsticks():
    """The float32 torch restatement against the float64 one over SHAPES: the numbers YARDSTICK holds."""
    from kvae.kalman import lgssm_ops
    worst = {"marginals": 0.0, "kl": 0.0, "path_logq": 0.0}
    for B, T, K in SHAPES:
        logits, init, P, ref, _ = reference(B, T, K)
        f32 = lgssm_ops.regime_decode_torch(logits, init, P)
        for name, g, r in (("marginals", f32["marginals"], ref["marginals"]), ("kl", f32["kl"].unsqueeze(-1), ref["kl"].unsqueeze(-1)),
                           ("path_logq", f32["path_logq"][:, None, None], ref["path_logq"][:, None, None])):
            worst[name] = max(worst[name], _per_step_ratio(g, r)[0])
    return worst


# ---- brute force: every path enumerated, independent of the restatement ------------------------------------------------------
def brute_force(DEV, K, T, B=2, seed=0):
    """All K^T paths in float64: marginals by summation, the best path and its probability, KL(q || p) = sum_t kl_t."""
    from kvae.kalman import lgssm_ops
    logits, init, P = inputs(B, T, K, seed)
    got = lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV))
    l64, i64 = logits.double(), init.double()
    lq0 = i64 - torch.logsumexp(i64, -1, keepdim=True)
    lqt = l64 - torch.logsumexp(l64, -1, keepdim=True)
    lp = torch.log(torch.maximum(P.double(), torch.tensor(1e-8, dtype=torch.float64)))
    for b in range(B):
        marg = torch.zeros(T, K, dtype=torch.float64)
        kl, scored = 0.0, []
        for s in itertools.product(range(K), repeat=T):
            lq = float(lq0[b, s[0]]) + sum(float(lqt[b, t, s[t - 1], s[t]]) for t in range(1, T))
            lpr = math.log(1.0 / K) + sum(float(lp[s[t - 1], s[t]]) for t in range(1, T))
            q = math.exp(lq)
            for t in range(T):
                marg[t, s[t]] += q
            kl += q * (lq - lpr)
            scored.append((lq, s))
        scored.sort(key=lambda v: (-v[0], v[1]))
        (best, best_path), (second, _) = scored[0], scored[1]
        assert best - second > GAP, (best, second)   # the enumeration alone decides that float32 must find this path
        ratio, where = _per_step_ratio(got["marginals"][b:b + 1].cpu(), marg[None])
        assert ratio < TOL["marginals"], (ratio, where)
        assert got["path"][b].tolist() == list(best_path), (got["path"][b].tolist(), best_path)
        assert abs(float(got["path_logq"][b]) - best) < TOL["path_logq"] * max(1.0, abs(best))
        kl_sum = float(got["kl"][b].double().sum())
        # T terms, each within TOL["kl"] of a scale no larger than the largest term
        assert abs(kl_sum - kl) < TOL["kl"] * T * max(float(got["kl"][b].abs().max()), abs(kl)), (kl_sum, kl)
        print("brute", (K, T, b), "marginals", ratio, "kl", kl_sum, kl, "gap", best - second)


# ---- the sampled chain the reference pins: frequencies and the mean of log q - log p --------------------------------------------
def vs_sampled_chain(DEV, T, K, seed, S=8192):
    """One sequence replicated to S rows through SwitchingDynamicsParameter.regime_chain (hard samples, tau = 0.5, float64): the
    one-hot frequencies within 5 standard errors of the marginals at every (t,k), the mean of sum_t (log_q - log_p) within 5 of
    sum_t kl_t."""
    from kvae.kalman import lgssm_ops
    from kvae.kalman.switch_dyn_param import StickyRegimePrior, SwitchingDynamicsParameter
    logits, init, P = inputs(1, T, K, seed)
    got = lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV), want=("marginals", "kl"))
    dyn = SwitchingDynamicsParameter(torch.eye(2).repeat(K, 1, 1), torch.zeros(K, 2, 1), torch.zeros(K, 1, 2),
                                     prior=StickyRegimePrior(K, 0.8), hidden_lstm=4)
    dyn.tau = 0.5
    g = torch.Generator().manual_seed(77 + seed)
    gumbel = -torch.empty(S, T, K, dtype=torch.float64).exponential_(generator=g).log()
    with torch.no_grad():
        y, lq, lp = dyn.regime_chain(logits.double().expand(S, -1, -1, -1), init.double().expand(S, -1), gumbel, hard=True)
    m = got["marginals"][0].double().cpu()
    se = (m * (1 - m) / S).sqrt()
    dev_m = float(((y.mean(0) - m).abs() / se).max())
    draws = (lq - lp).sum(-1)
    dev_kl = float((draws.mean() - got["kl"][0].double().sum().cpu()).abs() / (draws.std() / math.sqrt(S)))
    print("sampled chain", (T, K), "marginals", dev_m, "s.e.; kl", dev_kl, "s.e.")
    assert dev_m <= 5 and dev_kl <= 5, (dev_m, dev_kl)


# ---- ties and clamps ---------------------------------------------------------------------------------------------------------------
def ties(DEV, K, B=2, T=6):
    """All-zero logits and init: every decision is a tie, so the path is all zeros (the lowest index wins everywhere); the
    marginals are 1/K - exactly where K is a power of two (1/K and its products are exact), within the bar otherwise; kl is that
    of uniform transitions."""
    from kvae.kalman import lgssm_ops
    logits, init, P = torch.zeros(B, T, K, K), torch.zeros(B, K), prior(K)
    got = lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV))
    ref = lgssm_ops.regime_decode_torch(logits.double(), init.double(), P.double())
    assert torch.equal(got["path"].cpu(), torch.zeros(B, T, dtype=torch.int64))
    assert torch.equal(ref["path"], torch.zeros(B, T, dtype=torch.int64))
    if K & (K - 1) == 0:
        assert torch.equal(got["marginals"].cpu(), torch.full((B, T, K), 1.0 / K))
    assert _per_step_ratio(got["marginals"].cpu(), ref["marginals"])[0] < TOL["marginals"]
    assert _per_step_ratio(got["kl"].unsqueeze(-1).cpu(), ref["kl"].unsqueeze(-1))[0] < TOL["kl"]
    assert _per_step_ratio(got["path_logq"][:, None, None].cpu(), ref["path_logq"][:, None, None])[0] < TOL["path_logq"]
    uniform = sum(math.log(1.0 / K) - math.log(max(float(P[0, j]), 1e-8)) for j in range(K)) / K
    assert abs(float(got["kl"][0, 1]) - uniform) < TOL["kl"] * abs(uniform) and abs(float(got["kl"][0, 0])) < 1e-6


def clamp(DEV, B, T, K):
    """StickyRegimePrior(K, 1.0): the off-diagonal entries of P are 0, so kl carries log(1e-8) terms - as the restatement's."""
    from kvae.kalman import lgssm_ops
    logits, init, P, ref, gaps = reference(B, T, K, seed=3, p_stay=1.0)
    assert float(P[0, 1]) == 0.0
    got = lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV))
    check_outputs(got, logits, init, ref, gaps)
    assert float(ref["kl"][:, 1:].min()) > 1.0   # the clamp term dominates: -log(1e-8) = 18.4 times the off-diagonal mass


def partial_outputs(DEV, B, T, K):
    """Each subset of `want` (NULL output pointers in the call) returns the same bits as the full call, None for the rest."""
    from kvae.kalman import lgssm_ops
    logits, init, P = (t.to(DEV) for t in inputs(B, T, K, seed=4))
    full = lgssm_ops.regime_decode(logits, init, P)
    names = ("marginals", "path", "kl")
    for r in (1, 2):
        for want in itertools.combinations(names, r):
            part = lgssm_ops.regime_decode(logits, init, P, want=want)
            for k in ("marginals", "path", "path_logq", "kl"):
                owner = "path" if k == "path_logq" else k
                if owner in want:
                    assert torch.equal(part[k], full[k]), (want, k)
                else:
                    assert part[k] is None, (want, k)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def c_abi(lib, DEV):
    """The error codes of include/kvae_lgssm.h through raw pointers, the workspace size, the refusal of K = 17."""
    import ctypes as C
    dll = lib.dll
    B, T, K = 2, 3, 4
    f = lambda *s: torch.zeros(*s, device=DEV)
    logits, init, P, marg, plq, kl = f(B, T, 17, 17), f(B, 17), f(17, 17), f(B, T, 17), f(B), f(B, T)
    path = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    ws = torch.zeros(B * T, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(logits=logits, init=init, P=P, marg=marg, path=path, plq=plq, kl=kl, ws=ws, B=B, T=T, K=K):
        return dll.kvae_regime_decode(p(logits), p(init), p(P), p(marg), p(path), p(plq), p(kl), p(ws), B, T, K, None)

    assert call() == 0
    for kw in (dict(logits=None), dict(init=None), dict(P=None)):
        assert call(**kw) == 2, kw                                        # KVAE_ERR_NULL
    for kw in (dict(B=0), dict(T=0), dict(K=17), dict(B=-1)):
        assert call(**kw) == 1, kw                                        # KVAE_ERR_DIMS
    for kw in (dict(K=0), dict(K=-3)):
        assert call(**kw) == 4, kw                                        # KVAE_ERR_ARG
    assert call(ws=None) == 2 and call(ws=None, path=None) == 2           # path or path_logq without a workspace
    assert call(ws=None, path=None, plq=None) == 0                        # neither: no workspace needed
    assert call(marg=None, kl=None) == 0 and call(marg=None, path=None, plq=None, kl=None, ws=None) == 0
    wsb = dll.kvae_regime_decode_ws_bytes
    assert wsb(5, 7, 8) == 5 * 7 * 4 and wsb(5, 7, 16) == 5 * 7 * 8 and wsb(5, 7, 9) == 5 * 7 * 8 and wsb(1, 1, 1) == 4
    assert wsb(5, 7, 17) == 0 and wsb(0, 7, 8) == 0 and wsb(5, 0, 8) == 0 and wsb(5, 7, 0) == 0
    assert wsb(1 << 33, 2, 16) == (1 << 33) * 16                          # 64-bit arithmetic
    if DEV != "cpu":
        torch.cuda.synchronize()


def k17_takes_torch(DEV):
    """K = 17 is outside the kernel: the Python layer takes regime_decode_torch (float32 there), forcing the kernel raises."""
    import pytest
    from kvae.kalman import lgssm_ops
    logits, init, P = inputs(2, 5, 17, seed=5)
    assert not lgssm_ops.regime_decode_supported(17, logits) and lgssm_ops.regime_decode_supported(16, logits)
    assert not lgssm_ops.regime_decode_supported(4, logits.double())
    got = lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV))
    ref = lgssm_ops.regime_decode_torch(logits.double(), init.double(), P.double())
    assert rel_err(got["marginals"].cpu(), ref["marginals"]) < 1e-5 and rel_err(got["kl"].cpu(), ref["kl"]) < 1e-5
    assert torch.equal(got["path"].cpu(), ref["path"]) or float(decision_gaps(logits.double(), init.double()).min()) <= GAP
    with pytest.raises(RuntimeError):
        lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV), impl="kernel")
    with pytest.raises(ValueError):
        lgssm_ops.regime_decode(logits.to(DEV), init.to(DEV), P.to(DEV), want=("paths",))


# ---- model level -----------------------------------------------------------------------------------------------------------------
def small_model(kind="switching", K=3):
    from post_cases import small_model as make
    return make(kind, K)


def _oracle_smoother(model, a, u, mask, path):
    """The float64 torch oracle's filter and smoother (oracle/torch_oracle.py) fed A[path_t], B[path_t], Q[path_t]."""
    from oracle import torch_oracle as O
    kf, dyn = model.kalman_filter, model.kalman_filter.dyn_params
    d = lambda t: t.detach().cpu().double()
    A, Bm, Q, Cm = d(dyn.A)[path], d(dyn.B)[path], d(dyn.Q)[path], d(dyn.C)[0]
    Bsz, T = path.shape
    a, u, mask = d(a), d(u), d(mask)
    mu, Sig = d(kf.mu0).expand(Bsz, -1).unsqueeze(-1), d(kf.Sigma0).expand(Bsz, -1, -1)
    mfs, Sfs, mps, Sps = [], [], [], []
    for t in range(T):
        mu, Sig, mu_p, Sig_p = O.filter_step(mu, Sig, a[:, t], u[:, t], A[:, t], Bm[:, t], Cm.expand(Bsz, -1, -1), Q[:, t], d(kf.R),
                                             mask[:, t])
        mfs.append(mu), Sfs.append(Sig), mps.append(mu_p), Sps.append(Sig_p)
    mus, Sigs = [mfs[-1]], [Sfs[-1]]
    for t in range(T - 2, -1, -1):
        m_s, S_s = O.smooth_step(Sfs[t], Sps[t + 1], Sigs[0], mfs[t], mps[t + 1], mus[0], A[:, t + 1])
        mus.insert(0, m_s), Sigs.insert(0, S_s)
    return torch.stack(mus, 1)


def model_level(DEV, K, B=3, T=12):
    from kvae import noise
    from kvae.kalman import lgssm_ops
    model = small_model("switching", K).to(DEV)
    model.train()
    dyn = model.kalman_filter.dyn_params
    dyn.tau = 0.37
    before = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(11 + K)
    x = (torch.rand(B, T, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    mask = torch.ones(B, T)
    mask[:, 4:7] = 0
    u = (0.3 * torch.randn(B, T, model.u_dim, generator=g)).to(DEV)
    out = model.decode_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    again = model.decode_regimes(x, u=u, mask=mask.to(DEV), decode=True)
    keys = ("regime_probs", "regimes", "regimes_logq", "regime_kl", "mus_smooth", "Sigmas_smooth", "mus_filt", "a_imputed",
            "x_imputed", "a_vae")
    for k in keys:
        assert torch.equal(out[k], again[k]), k                          # deterministic: bit-identical
    assert model.training and dyn.tau == 0.37                             # left as they were
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert out["regime_probs"].shape == (B, T, K) and out["regimes"].shape == (B, T) and out["regimes"].dtype == torch.int64
    assert out["regimes_logq"].shape == (B,) and out["regime_kl"].shape == (B, T)
    assert out["mus_smooth"].shape == (B, T, model.z_dim, 1) and out["a_imputed"].shape == (B, T, model.a_dim)
    assert out["x_imputed"].shape == x.shape and len(out["ABC"]) == 3
    assert float((out["regime_probs"].sum(-1) - 1).abs().max()) < TOL["marginals"]
    assert int(out["regimes"].min()) >= 0 and int(out["regimes"].max()) < K
    # the decode against the float64 restatement over the model's own logits
    model.eval()
    with torch.no_grad():
        a_mu = model.encode_sequence(x, sample=False)[0]
        assert torch.equal(a_mu, out["a_vae"])
        logits, init = dyn.markov_regime_posterior(a_mu)
    model.train()
    l32, i32 = logits.detach().cpu(), init.detach().cpu()
    ref = lgssm_ops.regime_decode_torch(l32.double(), i32.double(), dyn.prior.transition_matrix.double())
    got = {"marginals": out["regime_probs"], "path": out["regimes"], "path_logq": out["regimes_logq"], "kl": out["regime_kl"]}
    gaps = decision_gaps(l32.double(), i32.double())
    c = lambda t: t.detach().cpu()
    for name, gg, r in (("marginals", got["marginals"], ref["marginals"]), ("kl", got["kl"].unsqueeze(-1), ref["kl"].unsqueeze(-1)),
                        ("path_logq", got["path_logq"][:, None, None], ref["path_logq"][:, None, None])):
        assert _per_step_ratio(c(gg), r)[0] < TOL[name], name
    short = (ref["path_logq"] - path_log_q(c(got["path"]), l32.double(), i32.double())).abs() / ref["path_logq"].abs().clamp_min(1.0)
    assert bool((short < TOL["path_logq"]).all())
    decided = gaps > GAP
    assert torch.equal(c(got["path"])[decided], ref["path"][decided])
    # the smoother under the pinned path: the float64 oracle fed A[path_t], B[path_t], Q[path_t]; 1e-4 is the project's bar on
    # smoothed means against its oracles at n = 4 (tests/test_gpu_parity.py, parity_cases.values_vs_fp64_oracle)
    want = _oracle_smoother(model, out["a_vae"], u, mask, c(out["regimes"]))
    err = rel_err(c(out["mus_smooth"]), want)
    print("decode_regimes", DEV, K, "mus_smooth vs the float64 oracle", err, "smallest gap", float(gaps.min()))
    assert err < 1e-4, err
    A_seq = out["ABC"][0]
    assert torch.equal(A_seq, dyn.A.detach()[out["regimes"]])             # a one-hot mix picks the regime's matrix
    # smooth=False stops after the decode; sample_a=True draws a as forward does
    lean = model.decode_regimes(x, smooth=False)
    assert "mus_smooth" not in lean and torch.equal(lean["regimes"], model.decode_regimes(x)["regimes"])
    eps = torch.randn(B * T, model.a_dim, generator=g).to(DEV)
    with noise.inject(eps_a=eps):
        drawn = model.decode_regimes(x, sample_a=True, smooth=False)
        model.eval()
        with torch.no_grad():
            assert torch.equal(drawn["a_vae"], model.encode_sequence(x)[0])
        model.train()
    assert not torch.equal(drawn["a_vae"], out["a_vae"])


def forward_unchanged_by_pinned(DEV, K=3, B=2, T=8):
    """forward() after a pinned(...) block matches a forward() with the same injected noise taken before it; inside the block
    the given sequence is what compute_batch uses, with the log q / log p of that sequence."""
    from kvae import noise
    model = small_model("switching", K).to(DEV).eval()
    dyn = model.kalman_filter.dyn_params
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(B, T, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    nz = dict(eps_a=torch.randn(B * T, 2, generator=g).to(DEV), gumbel=(-torch.empty(B, T, K).exponential_(generator=g).log()).to(DEV))
    with torch.no_grad():
        with noise.inject(**nz):
            first = model(x)
            lq_first, lp_first = (t.clone() for t in dyn.elbo_terms())
        y = first["state_probs"]
        assert bool(((y == 0) | (y == 1)).all())                         # eval mode: a hard one-hot draw
        with noise.inject(**nz):
            with dyn.pinned(y):
                inside = model(x)
                lq_in, lp_in = (t.clone() for t in dyn.elbo_terms())
            second = model(x)
    for k in ("state_probs", "mus_smooth", "Sigmas_smooth", "a_samples", "x_logits"):
        assert torch.equal(first[k], second[k]), k
    # pinned to the draw itself: the same regimes, the same smoother, and the chain's log q / log p of that sequence
    assert torch.equal(inside["state_probs"], y) and rel_err(inside["mus_smooth"].cpu(), first["mus_smooth"].cpu()) < 1e-6
    assert float((lq_in - lq_first).abs().max()) < 1e-5 and float((lp_in - lp_first).abs().max()) < 1e-5
    assert dyn._pinned is None


def model_errors(DEV):
    import pytest
    lstm = small_model("lstm").to(DEV)
    x = torch.zeros(2, 3, 1, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="switching"):
        lstm.decode_regimes(x)
    model = small_model("switching").to(DEV)
    for bad in (dict(mask=torch.ones(2, 4)), dict(mask=torch.ones(3, 3)), dict(u=torch.zeros(2, 4, 4)), dict(u=torch.zeros(2, 3, 3)),
                dict(u=torch.zeros(2, 3)), dict(decode=True, smooth=False)):
        with pytest.raises(ValueError):
            model.decode_regimes(x, **bad)
    one = small_model("switching", K=1).to(DEV)                           # K = 1: ones, zeros and zeros, without a launch
    out = one.decode_regimes(x)
    assert torch.equal(out["regime_probs"], torch.ones(2, 3, 1, device=DEV)) and not bool(out["regimes"].any())
    assert not bool(out["regimes_logq"].any()) and not bool(out["regime_kl"].any()) and out["mus_smooth"].shape == (2, 3, 4, 1)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "kalman-vae_amd"))
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    print({k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print({s: float(reference(*s)[4].min()) for s in SHAPES + LONG_SHAPES})
