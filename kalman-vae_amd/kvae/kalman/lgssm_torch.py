"""The LGSSM read-outs of lgssm_ops restated in plain torch ops: what the dispatchers there fall back to for dtypes, devices and
shapes the HIP kernels are not built for, and (in float64) the references the kernels are tested against.  Nothing here touches
the native library: the module imports without it.  lgssm_ops re-exports every name, which is where callers take them from.
"""
import torch

_DECODE_OUTPUTS = ("marginals", "path", "kl")
_PRED_OUTPUTS = ("ll", "nis", "a_pred", "S", "levels", "seq_ll")
_LOG_2PI = 1.8378770664093453
_SWF_OUTPUTS = ("regime_filt", "regime_pred", "log_lik", "log_lik_seq", "a_pred", "S", "mus_filt", "Sigmas_filt", "levels", "state")
_SWS_SMOOTH = ("regime_smooth", "regime_pairs", "mus_smooth", "Sigmas_smooth")
_SWS_OUTPUTS = _SWF_OUTPUTS + _SWS_SMOOTH
_SWH_FORE = ("regime_fore", "a_fore", "S_fore", "mus_fore", "Sigmas_fore", "log_lik_fore", "levels_fore")
_SWH_OUTPUTS = _SWF_OUTPUTS + _SWH_FORE
_SWV_OUTPUTS = ("path", "path_log_joint", "scores", "backptr", "mus_filt", "Sigmas_filt", "levels", "state")


def _want(op, outputs, want):
    """`want` (one name or several) of the read-out `op` as a tuple, checked against the `outputs` it can compute."""
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [w for w in want if w not in outputs]
    if bad or not want:
        raise ValueError(f"{op}: want must name some of {outputs}, got {want}")
    return want


def _jitter_ladder(max_tries=5, jitter_init=1e-6):
    """The jitters 1e-6 * 10^level of the _safe_cholesky ladder as Python doubles, by the reference's repeated `*= 10.0`
    (10 ** level gives other doubles)."""
    jitter = jitter_init
    for _ in range(max_tries):
        yield jitter
        jitter *= 10.0


def safe_cholesky(Sigma, max_tries=5, jitter_init=1e-6):
    """The reference's _safe_cholesky ladder (kalman_filter.py:282-303 there) over a batch [..., n, n]: symmetrise, add
    jitter 1e-6 * 10^level until the WHOLE batch factorises (levels 0..4), else the clamped-diagonal fallback."""
    Sigma = 0.5 * (Sigma + Sigma.mT)
    eye = torch.eye(Sigma.shape[-1], device=Sigma.device, dtype=Sigma.dtype)
    for jitter in _jitter_ladder(max_tries, jitter_init):
        L, info = torch.linalg.cholesky_ex(Sigma + jitter * eye)
        if not bool((info != 0).any()):
            return L
    return torch.diag_embed(torch.sqrt(torch.diagonal(Sigma, dim1=-2, dim2=-1).clamp(min=1e-6)))


def safe_cholesky_items(Sigma, max_tries=5, jitter_init=1e-6):
    """The _safe_cholesky ladder applied PER ITEM of a batch [..., n, n]: (L, levels) with levels[...] the first level 0..4
    (jitter 1e-6 * 10^level) at which that item factorises, 5 = its clamped-diagonal fallback.  No host sync."""
    Sigma = 0.5 * (Sigma + Sigma.mT)
    eye = torch.eye(Sigma.shape[-1], device=Sigma.device, dtype=Sigma.dtype)
    L = torch.diag_embed(torch.sqrt(torch.diagonal(Sigma, dim1=-2, dim2=-1).clamp(min=1e-6)))
    levels = torch.full(Sigma.shape[:-2], max_tries, device=Sigma.device, dtype=torch.int32)
    for lv, jitter in enumerate(_jitter_ladder(max_tries, jitter_init)):
        Lv, info = torch.linalg.cholesky_ex(Sigma + jitter * eye)
        take = (levels == max_tries) & (info == 0) & torch.isfinite(Lv).all(-1).all(-1)
        L = torch.where(take[..., None, None], Lv, L)
        levels = torch.where(take, torch.full_like(levels, lv), levels)
    return L, levels


def _bt(t, Bsz, T):
    """[B,T,r,c] view of a per-step operand given as [r,c] or [B,T,r,c]."""
    return t.expand(Bsz, T, *t.shape[-2:]) if t.dim() == 2 else t


def _innovation(mus_pred, Sigmas_pred, Cm, R, Y, mask):
    """What predictive_torch and log_marginal_torch share, in the dtype of Sigmas_pred: the forecast a_pred = C mu_pred [B,T,p], its
    covariance S = C Sigma_pred C^T + R (symmetrised), the residual Y - a_pred and the observed steps [B,T] (bool, None = all)."""
    mp = mus_pred.squeeze(-1) if mus_pred.dim() == 4 else mus_pred
    dt = Sigmas_pred.dtype
    Bsz, T, n = mp.shape
    mp, Cm, R, Y = mp.to(dt), _bt(Cm.to(dt), Bsz, T), R.to(dt), Y.to(dt)
    a_pred = (Cm @ mp.unsqueeze(-1)).squeeze(-1)
    S = Cm @ Sigmas_pred @ Cm.mT + R
    S = 0.5 * (S + S.mT)
    observed = None if mask is None else mask.to(device=S.device).reshape(Bsz, T) != 0
    return a_pred, S, Y - a_pred, observed


def _gauss_ll(L, res):
    """(ll, nis) of the residuals res [..., p] under N(0, L L^T): nis = |L^-1 res|^2, ll = -(nis + log det + p log 2 pi) / 2."""
    w = torch.linalg.solve_triangular(L, res.unsqueeze(-1), upper=False).squeeze(-1)
    nis = (w * w).sum(-1)
    logdet = 2.0 * torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)
    return -0.5 * (nis + logdet + L.shape[-1] * _LOG_2PI), nis


def _observed_only(v, observed):
    """v with zeros where `observed` (bool, broadcast against v; None = everything observed) is False."""
    return v if observed is None else torch.where(observed, v, torch.zeros_like(v))


def regime_decode_torch(logits, init_logits, P, want=_DECODE_OUTPUTS):
    """The equations of kvae_regime_decode in torch ops, in the dtype of the logits: K > 16 and non-fp32 tensors, and (in float64)
    the reference the kernel is tested against.  Ties take the lowest index, in every backpointer and in the final argmax
    (an argmax over (value == max), whose first hit torch returns).  T - 1 iterations of about ten small launches."""
    want = _want("regime_decode", _DECODE_OUTPUTS, want)
    Bsz, T, K, _ = logits.shape
    dt = logits.dtype
    init_logits, P = init_logits.to(dt), P.to(device=logits.device, dtype=dt)
    first = lambda v: (v == v.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)   # lowest index among the maxima
    ls0 = torch.log_softmax(init_logits, -1)
    m, d = torch.softmax(init_logits, -1), ls0
    log_p = torch.log(P.clamp_min(1e-8))
    ms, kls, bps = [m], [(m * (ls0 - torch.full_like(ls0, 1.0 / K).log())).sum(-1)], []
    for t in range(1, T):
        lq = torch.log_softmax(logits[:, t], -1)              # [B, i, j]
        Q = torch.softmax(logits[:, t], -1)
        if "marginals" in want or "kl" in want:
            kls.append((m * (Q * (lq - log_p)).sum(-1)).sum(-1))
            m = torch.einsum("bi,bij->bj", m, Q)
            ms.append(m)
        if "path" in want:
            cand = (d.unsqueeze(-1) + lq).transpose(1, 2)      # [B, j, i]
            bps.append(first(cand))
            d = cand.max(-1).values
    out = {"marginals": None, "path": None, "path_logq": None, "kl": None}
    if "marginals" in want:
        out["marginals"] = torch.stack(ms, 1)
    if "kl" in want:
        out["kl"] = torch.stack(kls, 1)
    if "path" in want:
        out["path_logq"] = d.max(-1).values
        s = first(d)
        path = [s]
        for bp in reversed(bps):
            s = bp.gather(1, s.unsqueeze(1)).squeeze(1)
            path.append(s)
        out["path"] = torch.stack(path[::-1], 1)
    return out


def rollout_torch(kind, A, Bm, Cm, mu, L0, U, LQ, LR, S, H, lstm=None, h0=None, c0=None, y0=None, P=None, s0=None,
                  eps0=None, eps_z=None, eps_a=None, gumbel=None):
    """The same recursion as csrc/lgssm_gen.h in torch ops, in the dtype of mu (fp32 on the product path): the shapes the
    kernel is not built for (alpha-network hidden != 50 or a_dim != 2) - about fifteen launches per step."""
    K = A.shape[0]
    Bsz = mu.shape[0]
    rep = lambda t: t.repeat_interleave(S, 0)
    flat = lambda t: None if t is None else t.reshape(Bsz * S, *t.shape[2:]).to(mu.dtype)
    eps0, eps_z, eps_a, gumbel = flat(eps0), flat(eps_z), flat(eps_a), flat(gumbel)
    z = rep(mu)
    if eps0 is not None:
        z = z + (rep(L0) @ eps0.unsqueeze(-1)).squeeze(-1)
    R = z.shape[0]
    if kind == "switching":
        s = rep(s0)
    elif K == 1:
        w = z.new_ones(R, 1)
    else:
        w_ih, w_hh, b_ih, b_hh, head_w, head_b = lstm
        h, c, y = rep(h0), rep(c0), rep(y0)
    a_out, z_out, w_out = [], [], []
    for t in range(H):
        if kind == "switching":
            pi = s @ P
            if gumbel is not None:
                s = torch.nn.functional.one_hot((pi.log() + gumbel[:, t]).argmax(-1), K).to(pi.dtype)
            else:
                s = pi
            w = s
        elif K > 1:
            gi, gf, gg, go = (y @ w_ih.T + h @ w_hh.T + b_ih + b_hh).chunk(4, -1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            w = torch.softmax(h @ head_w.T + head_b, -1)
        zn = torch.einsum("rk,kij,rj->ri", w, A, z)
        if U is not None:
            zn = zn + torch.einsum("rk,kij,rj->ri", w, Bm, rep(U[:, t]))
        if eps_z is not None:
            LQt = torch.einsum("rk,kij->rij", w, LQ) if kind == "switching" else LQ
            zn = zn + (LQt @ eps_z[:, t].unsqueeze(-1)).squeeze(-1)
        z = zn
        a = Cm[0] @ z.unsqueeze(-1) if kind == "switching" else torch.einsum("rk,kij,rj->ri", w, Cm, z).unsqueeze(-1)
        a = a.squeeze(-1)
        if eps_a is not None:
            a = a + (LR @ eps_a[:, t].unsqueeze(-1)).squeeze(-1)
        y = a
        a_out.append(a), z_out.append(z), w_out.append(w)
    un = lambda lst: torch.stack(lst, 1).reshape(Bsz, S, H, -1)
    return un(a_out), un(z_out), un(w_out)


def posterior_paths_torch(mus_filt, Sigmas_filt, mus_pred, Sigmas_pred, A, Cm, Q, S, LR=None, eps=None, eta=None):
    """The recursion of csrc/lgssm_post.h in torch ops, batched over B and S, in the dtype of mus_filt: for dtypes, devices and
    shapes the kernels are not built for - several launches per time step.  Same arguments and returns as posterior_paths."""
    mf = mus_filt.squeeze(-1) if mus_filt.dim() == 4 else mus_filt
    mp = mus_pred.squeeze(-1) if mus_pred.dim() == 4 else mus_pred
    dt = mf.dtype
    Bsz, T, n = mf.shape
    Sf, Sp = Sigmas_filt.to(dt), Sigmas_pred.to(dt)
    A, Cm, Q = (_bt(t.to(dt), Bsz, T) for t in (A, Cm, Q))
    eye = torch.eye(n, device=mf.device, dtype=dt)
    J = torch.zeros(Bsz, T, n, n, device=mf.device, dtype=dt)
    P = Sf.clone()
    if T > 1:
        An, Qn = A[:, 1:], Q[:, 1:]
        Jt = torch.linalg.solve(Sp[:, 1:].mT, (Sf[:, :-1] @ An.mT).mT).mT
        G = eye - Jt @ An
        J[:, :-1] = Jt
        P[:, :-1] = G @ Sf[:, :-1] @ G.mT + Jt @ Qn @ Jt.mT
    L, levels = safe_cholesky_items(P)
    c = mf.clone()
    if T > 1:
        c[:, :-1] = mf[:, :-1] - (J[:, :-1] @ mp[:, 1:].unsqueeze(-1)).squeeze(-1)
    z = torch.zeros(Bsz, S, n, device=mf.device, dtype=dt)
    zs = [None] * T
    for t in range(T - 1, -1, -1):
        z = c[:, t, None] + z @ J[:, t].mT
        if eps is not None:
            z = z + eps[:, :, t].to(dt) @ L[:, t].mT
        zs[t] = z
    z = torch.stack(zs, 2)
    a = (Cm[:, None] @ z.unsqueeze(-1)).squeeze(-1)
    if eta is not None:
        a = a + eta.to(dt) @ LR.to(dt).mT
    return z, a, levels


def predictive_torch(mus_pred, Sigmas_pred, Cm, R, Y, mask=None, want=_PRED_OUTPUTS):
    """The equations of kvae_lgssm_predictive in torch ops, batched over (b, t), in the dtype of Sigmas_pred: other a_dim than 2,
    non-fp32 and host tensors, and (in float64) the reference the kernel is tested against.  The factor of S_t is found by the
    per-item ladder (safe_cholesky_items).  Same arguments and returns as predictive (without packed / slots)."""
    want = _want("predictive", _PRED_OUTPUTS, want)
    a_pred, S, res, observed = _innovation(mus_pred, Sigmas_pred, Cm, R, Y, mask)
    L, levels = safe_cholesky_items(S)
    ll, nis = (_observed_only(v, observed) for v in _gauss_ll(L, res))
    full = {"ll": ll, "nis": nis, "a_pred": a_pred, "S": S, "levels": levels, "seq_ll": ll.sum(1)}
    return {k: (v if k in want else None) for k, v in full.items()}


def log_marginal_torch(mus_pred, Sigmas_pred, Cm, R, Y, mask=None):
    """log_marginal in torch ops, differentiable, in the dtype of Sigmas_pred: other a_dim than 2, non-fp32 and host tensors, and
    (in float64) the reference the adjoint kernel is tested against.  The values are predictive_torch's.  Nothing is
    differentiated through safe_cholesky_items (its torch.where over failed cholesky_ex attempts turns into NaN * 0 in the
    backward): the levels are found without a tape, then S + jitter[level] I - for level-5 items the clamped diagonal matrix - is
    factorised once."""
    a_pred, S, res, observed = _innovation(mus_pred, Sigmas_pred, Cm, R, Y, mask)
    with torch.no_grad():
        _, levels = safe_cholesky_items(S)
    jitter = torch.tensor([*_jitter_ladder(), 0.0], device=S.device, dtype=torch.float64)[levels.long()]
    eye = torch.eye(S.shape[-1], device=S.device, dtype=S.dtype)
    St = S + (jitter[..., None, None] * eye.double()).to(S.dtype)
    clamped = torch.diag_embed(torch.diagonal(S, dim1=-2, dim2=-1).clamp(min=1e-6))
    St = torch.where((levels == 5)[..., None, None], clamped, St)
    ll = _observed_only(_gauss_ll(torch.linalg.cholesky(St), res)[0], observed)
    return {"ll": ll, "seq_ll": ll.sum(1), "levels": levels}


def _swf_state(state, Bsz, K, n):
    if state is None:
        return None
    lw, mu, Sig = state["log_w"], state["mu"], state["Sigma"]
    if lw.shape != (Bsz, K) or mu.shape != (Bsz, K, n) or Sig.shape != (Bsz, K, n, n):
        raise ValueError(f"switching_filter: state must hold log_w [{Bsz},{K}], mu [{Bsz},{K},{n}], Sigma [{Bsz},{K},{n},{n}], got "
                         f"{tuple(lw.shape)}, {tuple(mu.shape)}, {tuple(Sig.shape)}")
    return lw, mu, Sig


def _swf_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, history=False):
    """The sweep of switching_filter_torch: (every output of _SWF_OUTPUTS, the history, the cast (A, Bm, Q, Cm, U)).  history: the
    collapsed per-regime beliefs mu [B,T,K,n], Sigma [B,T,K,n,n] and the pair weights W [B,T,K,K] (indexed (i, j)) of every step,
    which switching_smoother_torch runs backwards over; None unless asked for."""
    dt, dev = A.dtype, Y.device
    K, n = A.shape[0], A.shape[1]
    Bsz, T, p = Y.shape
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = (t.detach().to(device=dev, dtype=dt) for t in (A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U))
    mask = None if mask is None else mask.detach().to(device=dev, dtype=dt).reshape(Bsz, T)
    st = _swf_state(state, Bsz, K, n)
    if st is None:
        lw = torch.full((Bsz, K), 1.0 / K, device=dev, dtype=dt).log()
        mu, Sig = mu0.expand(Bsz, K, n), Sigma0.expand(Bsz, K, n, n)
    else:
        lw, mu, Sig = (t.detach().to(device=dev, dtype=dt) for t in st)
    uniform = torch.full((K, K), 1.0 / K, device=dev, dtype=dt)
    outs = {k: [] for k in ("regime_filt", "regime_pred", "log_lik", "a_pred", "S", "mus_filt", "Sigmas_filt", "levels")}
    hist = {k: [] for k in ("mu", "Sigma", "W", "lw")} if history else None
    for t in range(T):
        Pt = uniform if (t == 0 and st is None) else P
        mk = torch.ones(Bsz, device=dev, dtype=dt) if mask is None else mask[:, t]
        s = _swf_step(A, Bm, Q, Cm, R, Pt, lw, mu, Sig, Y[:, t], U[:, t], mk)
        lw, mu, Sig = s["lw"], s["mu"], s["Sigma"]
        if history:
            hist["mu"].append(mu), hist["Sigma"].append(Sig), hist["W"].append(s["W"]), hist["lw"].append(lw)
        for k in outs:
            outs[k].append(s[k])
    full = {k: torch.stack(v, 1) for k, v in outs.items()}
    full["log_lik_seq"] = full["log_lik"].sum(1)
    full["state"] = {"log_w": lw, "mu": mu, "Sigma": Sig}
    return full, ({k: torch.stack(v, 1) for k, v in hist.items()} if history else None), (A, Bm, Q, Cm, U)


def _sw_pairs(A, Bm, Q, Cm, R, mu, Sig, y, u, mk):
    """The K^2 Kalman steps of one step of the switching read-outs over a batch [N, ...], indexed [N, i, j, ...] (regime i's belief
    (mu [N,K,n], Sig [N,K,n,n]) under regime j's dynamics): the filtered pair (muf, Sf), the pair forecast (ap, S), the pair density
    of y whatever the mask says (lraw), the same with zeros on hidden steps (lij), and the ladder level of S (lv)."""
    eye = torch.eye(A.shape[1], device=A.device, dtype=A.dtype)
    observed = mk != 0
    mp = torch.einsum("jrc,bic->bijr", A, mu) + torch.einsum("jrc,bc->bjr", Bm, u).unsqueeze(1)
    Sp = torch.einsum("jre,biec,jdc->bijrd", A, Sig, A) + Q
    ap = mp @ Cm.mT
    res = y[:, None, None, :] - ap
    S = Cm @ Sp @ Cm.mT + R
    S = 0.5 * (S + S.mT)
    L, lv = safe_cholesky_items(S)
    lraw = _gauss_ll(L, res)[0]
    lij = _observed_only(lraw, observed[:, None, None])
    Kg = torch.linalg.solve(S, Cm @ Sp).mT * mk[:, None, None, None, None]      # S^-1 (Sigma_pred C^T)^T, transposed
    muf = mp + (Kg @ res.unsqueeze(-1)).squeeze(-1)
    IKC = eye - Kg @ Cm
    Sf = IKC @ Sp @ IKC.mT + Kg @ R @ Kg.mT
    Sf = 0.5 * (Sf + Sf.mT)
    return muf, Sf, ap, S, lraw, lij, lv


def _swf_step(A, Bm, Q, Cm, R, Pt, lw, mu, Sig, y, u, mk, score=False):
    """One step of the sweep over a batch [N, ...] (the sequences of the filter; the (sequence, origin) items of the forecast): from
    the carried (lw [N,K], mu [N,K,n], Sig [N,K,n,n]) under the transition matrix Pt, the frame y [N,p], the input u [N,m] and the
    mask mk [N].  Returns the step's outputs under the names of _SWF_OUTPUTS, the collapsed beliefs it hands on (lw, mu, Sigma) and
    the pair weights W [N,i,j].  score: also "scored" [N] = logsumexp_ij(lw_i + log Pt[i,j] + l_ij) with the pair densities of y
    whatever mk says - the density of a frame that the step itself does not condition on."""
    dev, dt = A.device, A.dtype
    K = A.shape[0]
    N = lw.shape[0]
    eyeK = torch.eye(K, device=dev, dtype=dt)
    ninf = torch.full((), -float("inf"), device=dev, dtype=dt)
    observed = mk != 0
    muf, Sf, ap, S, lraw, lij, lv = _sw_pairs(A, Bm, Q, Cm, R, mu, Sig, y, u, mk)

    def weights(logc):   # (the column softmax W_{i|j}, logsumexp_ij, log w'(j)); a dead column is one-hot at i = j
        cmx = logc.amax(1)                                                       # [N, j]
        dead = cmx == ninf
        ex = torch.where(dead.unsqueeze(1), eyeK.expand(N, K, K), (logc - torch.where(dead, torch.zeros_like(cmx), cmx).unsqueeze(1)).exp())
        se = ex.sum(1)
        mx = cmx.amax(-1, keepdim=True)
        tot = mx.squeeze(-1) + (se * (cmx - mx).exp()).sum(-1).log()
        return ex / se.unsqueeze(1), tot, (cmx + se.log()) - tot.unsqueeze(-1)

    # ---- weights ----
    logp = lw.unsqueeze(-1) + Pt.log()                                           # [N, i, j]
    pw = lw.exp().unsqueeze(-1) * Pt
    W, tot, lw = weights(logp + lij)
    rf = lw.exp()
    # ---- collapse over i ----
    mu = (W.unsqueeze(-1) * muf).sum(1)                                          # [N, j, n]
    d = muf - mu.unsqueeze(1)
    Sig = (W[..., None, None] * (Sf + d.unsqueeze(-1) * d.unsqueeze(-2))).sum(1)
    Sig = 0.5 * (Sig + Sig.mT)
    # ---- outputs of the step ----
    a = (pw.unsqueeze(-1) * ap).sum((1, 2))
    e = ap - a[:, None, None, :]
    m_, V_ = _moment_match(rf, mu, Sig)
    out = dict(lw=lw, mu=mu, Sigma=Sig, W=W, regime_pred=pw.sum(1), regime_filt=rf, log_lik=torch.where(observed, tot, torch.zeros_like(tot)),
               levels=torch.where(pw > 0, lv, torch.zeros_like(lv)).amax((1, 2)), a_pred=a,
               S=(pw[..., None, None] * (S + e.unsqueeze(-1) * e.unsqueeze(-2))).sum((1, 2)), mus_filt=m_, Sigmas_filt=V_)
    if score:
        out["scored"] = weights(logp + lraw)[1]
    return out


@torch.no_grad()
def switching_filter_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, state=None, want=_SWF_OUTPUTS):
    """The equations of kvae_lgssm_switching_filter (include/kvae_lgssm.h) in torch ops, vectorised over (B, i, j), in the dtype of
    A: shapes outside the kernel's, non-fp32 and host tensors, and (in float64) the reference the kernel is tested against.
    T steps of about thirty small launches.  Same arguments and returns as switching_filter."""
    want = _want("switching_filter", _SWF_OUTPUTS, want)
    full, _, _ = _swf_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state)
    return {k: (full[k] if k in want else None) for k in _SWF_OUTPUTS}


def _swv_state(state, Bsz, K, n):
    if state is None:
        return None
    J, mu, Sig = state["score"], state["mu"], state["Sigma"]
    if J.shape != (Bsz, K) or mu.shape != (Bsz, K, n) or Sig.shape != (Bsz, K, n, n):
        raise ValueError(f"switching_viterbi: state must hold score [{Bsz},{K}], mu [{Bsz},{K},{n}], Sigma [{Bsz},{K},{n},{n}], got "
                         f"{tuple(J.shape)}, {tuple(mu.shape)}, {tuple(Sig.shape)}")
    return J, mu, Sig


def _first_max(v, dim):
    """The lowest index along `dim` among the maxima of v (an argmax over (value == max), whose first hit torch returns)."""
    return (v == v.amax(dim, keepdim=True)).to(torch.int8).argmax(dim)


def _swv_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, margins=False):
    """The sweep and backtrace of switching_viterbi_torch: every output of _SWV_OUTPUTS, and - margins, for the tests - "margin" [B], the smallest decision
    margin of the sequence: best minus runner-up of c_ij over i at every (t, j) with a finite maximum (the first step of a stream
    without carried state is left out: its K candidates are one and the same number) and of the final maximum over j; +inf where
    there is no runner-up."""
    dt, dev = A.dtype, Y.device
    K, n = A.shape[0], A.shape[1]
    Bsz, T, p = Y.shape
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = (t.detach().to(device=dev, dtype=dt) for t in (A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U))
    mask = None if mask is None else mask.detach().to(device=dev, dtype=dt).reshape(Bsz, T)
    st = _swv_state(state, Bsz, K, n)
    if st is None:
        J = torch.zeros(Bsz, K, device=dev, dtype=dt)
        mu, Sig = mu0.expand(Bsz, K, n), Sigma0.expand(Bsz, K, n, n)
    else:
        J, mu, Sig = (t.detach().to(device=dev, dtype=dt) for t in st)
    ninf = torch.full((), -float("inf"), device=dev, dtype=dt)
    log_uniform, logP = torch.full((K, K), 1.0 / K, device=dev, dtype=dt).log(), P.log()
    own = torch.arange(K, device=dev).expand(Bsz, K)
    margin = torch.full((Bsz,), float("inf"), device=dev, dtype=dt)

    def gap(v, dim):   # best minus runner-up along dim; +inf without a finite best or without a runner-up
        if v.shape[dim] < 2:
            return torch.full_like(v.amax(dim), float("inf"))
        top = v.topk(2, dim=dim).values
        best, second = top.select(dim, 0), top.select(dim, 1)
        return torch.where(best == ninf, torch.full_like(best, float("inf")), best - second)

    outs = {k: [] for k in ("scores", "backptr", "levels", "mu", "Sigma")}
    for t in range(T):
        first = t == 0 and st is None
        mk = torch.ones(Bsz, device=dev, dtype=dt) if mask is None else mask[:, t]
        muf, Sf, _, _, _, lij, lv = _sw_pairs(A, Bm, Q, Cm, R, mu, Sig, Y[:, t], U[:, t], mk)
        prior = J.unsqueeze(-1) + (log_uniform if first else logP)                # [B, i, j]
        c = prior + lij
        J = c.amax(1)                                                            # [B, j]
        bp = torch.where(J == ninf, own, _first_max(c, 1))                       # a column without a finite entry keeps i = j
        if margins and not first:
            margin = torch.minimum(margin, gap(c, 1).amin(-1))
        mu = muf.gather(1, bp[:, None, :, None].expand(Bsz, 1, K, n)).squeeze(1)  # the selected pair's belief: a copy
        Sig = Sf.gather(1, bp[:, None, :, None, None].expand(Bsz, 1, K, n, n)).squeeze(1)
        outs["scores"].append(J), outs["backptr"].append(bp.to(torch.int32)), outs["mu"].append(mu), outs["Sigma"].append(Sig)
        outs["levels"].append(torch.where(prior > ninf, lv, torch.zeros_like(lv)).amax((1, 2)))
    full = {k: torch.stack(outs[k], 1) for k in ("scores", "backptr", "levels")}
    full["state"] = {"score": J, "mu": mu, "Sigma": Sig}
    full["path_log_joint"] = J.amax(-1)
    if margins:
        full["margin"] = torch.minimum(margin, gap(J, 1))
    s = _first_max(J, 1)
    path = [s]
    for t in range(T - 1, 0, -1):
        s = outs["backptr"][t].long().gather(1, s.unsqueeze(1)).squeeze(1)
        path.append(s)
    path = torch.stack(path[::-1], 1)                                            # [B, T]
    full["path"] = path.to(torch.int32)
    full["mus_filt"] = torch.stack(outs["mu"], 1).gather(2, path[:, :, None, None].expand(Bsz, T, 1, n)).squeeze(2)
    full["Sigmas_filt"] = torch.stack(outs["Sigma"], 1).gather(2, path[:, :, None, None, None].expand(Bsz, T, 1, n, n)).squeeze(2)
    return full


@torch.no_grad()
def switching_viterbi_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, state=None, want=_SWV_OUTPUTS):
    """The equations of kvae_lgssm_switching_viterbi (include/kvae_lgssm.h) in torch ops, vectorised over (B, i, j), in the dtype of
    A: the pair steps of switching_filter_torch (_sw_pairs), a maximum and a gather in place of the collapse, then the backtrace.
    The fallback of switching_viterbi and (in float64) the reference its kernel is tested against.  Same arguments and returns as
    switching_viterbi."""
    want = _want("switching_viterbi", _SWV_OUTPUTS, want)
    full = _swv_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state)
    return {k: (full[k] if k in want else None) for k in _SWV_OUTPUTS}


def _moment_match(w, mu, Sig):
    """(mean [B,n], covariance [B,n,n]) of the mixture of the K Gaussians (mu [B,K,n], Sig [B,K,n,n]) under the weights w [B,K]."""
    m_ = (w.unsqueeze(-1) * mu).sum(1)
    dd = mu - m_.unsqueeze(1)
    return m_, (w[..., None, None] * (Sig + dd.unsqueeze(-1) * dd.unsqueeze(-2))).sum(1)


def _swh_args(op, Bm, Y, U_all, horizon, origins):
    """(H, t0, U_all [B,T+H,m]) of a forecast call, checked: horizon >= 1, origins "all" (t0 = 0) or "last" (t0 = T - 1), U_all
    [B,T+H,m] or None = zeros in the dtype of Y."""
    H = int(horizon)
    Bsz, T, m = Y.shape[0], Y.shape[1], Bm.shape[2]
    if H < 1:
        raise ValueError(f"{op}: horizon must be >= 1, got {horizon}")
    if origins not in ("all", "last"):
        raise ValueError(f"{op}: origins must be 'all' or 'last', got {origins!r}")
    if U_all is None:
        U_all = torch.zeros(Bsz, T + H, m, device=Y.device, dtype=Y.dtype)
    if tuple(U_all.shape) != (Bsz, T + H, m):
        raise ValueError(f"{op}: U_all must be [B, T+H, m] = [{Bsz}, {T + H}, {m}], got {list(U_all.shape)}")
    return H, (0 if origins == "all" else T - 1), U_all


@torch.no_grad()
def switching_forecast_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U_all, horizon, mask=None, origins="all", state=None, want=_SWH_OUTPUTS):
    """The equations of kvae_lgssm_switching_forecast (include/kvae_lgssm.h) in torch ops, in the dtype of A: the sweep of
    switching_filter_torch with its history kept, then H horizon steps - each the sweep's own step (_swf_step) with the mask at 0 -
    vectorised over the B * T_o (sequence, origin) items.  The fallback of switching_forecast and (in float64) the reference its
    kernel is tested against.  Same arguments and returns as switching_forecast."""
    want = _want("switching_forecast", _SWH_OUTPUTS, want)
    H, t0, U_all = _swh_args("switching_forecast", Bm, Y, U_all, horizon, origins)
    Bsz, T, p = Y.shape
    full, hist, (A, Bm, Q, Cm, _) = _swf_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U_all[:, :T], mask, state, history=True)
    dt, dev = A.dtype, Y.device
    K, n, To = A.shape[0], A.shape[1], T - t0
    R, P, Y, U_all = (t.detach().to(device=dev, dtype=dt) for t in (R, P, Y, U_all))
    mask = None if mask is None else mask.detach().to(device=dev, dtype=dt).reshape(Bsz, T)
    items = lambda t: t[:, t0:].reshape(Bsz * To, *t.shape[2:])                 # [B, T, ...] -> [B T_o, ...]
    lw, mu, Sig = items(hist["lw"]), items(hist["mu"]), items(hist["Sigma"])
    hidden = torch.zeros(Bsz * To, device=dev, dtype=dt)
    origin = torch.arange(t0, T, device=dev)
    outs = {k: [] for k in _SWH_FORE}
    for h in range(1, H + 1):
        step = origin + h                                                        # [T_o]
        target = step < T
        at = step.clamp(max=T - 1)
        y = torch.where(target[None, :, None], Y[:, at], torch.zeros((), device=dev, dtype=dt)).reshape(Bsz * To, p)
        observed = (target[None, :] if mask is None else target[None, :] & (mask[:, at] != 0)).expand(Bsz, To).reshape(Bsz * To)
        s = _swf_step(A, Bm, Q, Cm, R, P, lw, mu, Sig, y, U_all[:, step].reshape(Bsz * To, -1), hidden, score=True)
        lw, mu, Sig = s["lw"], s["mu"], s["Sigma"]
        outs["regime_fore"].append(s["regime_pred"]), outs["a_fore"].append(s["a_pred"]), outs["S_fore"].append(s["S"])
        outs["mus_fore"].append(s["mus_filt"]), outs["Sigmas_fore"].append(s["Sigmas_filt"]), outs["levels_fore"].append(s["levels"])
        outs["log_lik_fore"].append(torch.where(observed, s["scored"], torch.zeros_like(s["scored"])))
    for k, v in outs.items():
        v = torch.stack(v, 1)                                                    # [B T_o, H, ...]
        full[k] = v.reshape(Bsz, To, *v.shape[1:])
    return {k: (full[k] if k in want else None) for k in _SWH_OUTPUTS}


@torch.no_grad()
def switching_smoother_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, state=None, want=_SWS_OUTPUTS):
    """The equations of kvae_lgssm_switching_smoother (include/kvae_lgssm.h) in torch ops, in the dtype of A: the sweep of
    switching_filter_torch with its history kept, then the backward pass vectorised over (B, j, k) = (regime at t, regime at
    t + 1).  The fallback of switching_smoother and (in float64) the reference its kernel is tested against.  Every Q_k must be
    positive definite.  Same arguments and returns as switching_smoother."""
    want = _want("switching_smoother", _SWS_OUTPUTS, want)
    full, hist, (A, Bm, Q, Cm, U) = _swf_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, history=True)
    full.update(_sws_backward(A, Bm, Q, U, hist, full["regime_filt"][:, -1]))
    return {k: (full[k] if k in want else None) for k in _SWS_OUTPUTS}


def _sws_pair_step(A, Bm, Q, u, mu, Sig, ms, Ss, W, M):
    """One transition of the backward pass, over every pair (j = source regime, k = destination regime): [B, j, k, ...].  (mu, Sig)
    [B, j, ...]: the source beliefs; u [B, m]: the input of the destination step; (ms, Ss, M) [B, k, ...]: the destination's smoothed
    beliefs and weights; W [B, j, k]: the filter's pair weights of the destination step.  Returns (J, the smoothed pair mean and
    covariance, the pair marginal)."""
    # ---- the filter's predict of pair (j, k) ----
    mp = torch.einsum("jrc,bic->bijr", A, mu) + torch.einsum("jrc,bc->bjr", Bm, u).unsqueeze(1)
    Sp = torch.einsum("jre,biec,jdc->bijrd", A, Sig, A) + Q
    J = torch.linalg.solve(Sp.mT, (Sig.unsqueeze(2) @ A.mT).mT).mT                   # Sigma A_k^T Sigma_p^-1
    mj = mu.unsqueeze(2) + (J @ (ms.unsqueeze(1) - mp).unsqueeze(-1)).squeeze(-1)
    Sj = Sig.unsqueeze(2) + J @ (Ss.unsqueeze(1) - Sp) @ J.mT
    Sj = 0.5 * (Sj + Sj.mT)
    return J, mj, Sj, W * M.unsqueeze(1)


def _sws_backward(A, Bm, Q, U, hist, w_last, em=None):
    """The backward pass of switching_smoother_torch over the history of _swf_forward and the final weights w_last [B,K]: the
    four outputs of _SWS_SMOOTH.  em: None, or dict(mu0, Sigma0, Y, mask) - then the pass also crosses the transition into t = 0
    and the second return value holds the expected sufficient statistics PER SEQUENCE (switching_em_statistics_torch)."""
    K, T = A.shape[0], U.shape[1]
    eyeK = torch.eye(K, device=A.device, dtype=A.dtype)
    M, ms, Ss = w_last, hist["mu"][:, -1], hist["Sigma"][:, -1]
    outs = {"regime_smooth": [M], "regime_pairs": [], "mus_smooth": [], "Sigmas_smooth": []}
    m_, S_ = _moment_match(M, ms, Ss)
    outs["mus_smooth"].append(m_), outs["Sigmas_smooth"].append(S_)
    acc = None if em is None else _EmSums(em, A.shape[1], U.shape[2], K, w_last)
    for t in range(T - 1, -1, -1):
        if acc is not None:
            acc.emission(t, m_, S_)
        if t == 0:
            break
        mu, Sig = hist["mu"][:, t - 1], hist["Sigma"][:, t - 1]                      # regime j at t - 1: [B, j, ...]
        J, mj, Sj, pair = _sws_pair_step(A, Bm, Q, U[:, t], mu, Sig, ms, Ss, hist["W"][:, t], M)
        if acc is not None:
            acc.transition(pair, ms, Ss, J, mj, Sj, U[:, t], first=False)
        # ---- weights: M_{t-1}, V_{k|j} ----
        M = pair.sum(2)
        dead = ~(M > 0)
        V = torch.where(dead.unsqueeze(2), eyeK.expand_as(pair), pair / torch.where(dead, torch.ones_like(M), M).unsqueeze(2))
        # ---- collapse over k ----
        ms = (V.unsqueeze(-1) * mj).sum(2)
        d = mj - ms.unsqueeze(2)
        Ss = (V[..., None, None] * (Sj + d.unsqueeze(-1) * d.unsqueeze(-2))).sum(2)
        Ss = 0.5 * (Ss + Ss.mT)
        m_, S_ = _moment_match(M, ms, Ss)
        outs["regime_smooth"].append(M), outs["regime_pairs"].append(pair), outs["mus_smooth"].append(m_), outs["Sigmas_smooth"].append(S_)
    smooth = {k: (torch.stack(v[::-1], 1) if v else w_last.new_zeros(w_last.shape[0], 0, K, K)) for k, v in outs.items()}
    if acc is None:
        return smooth
    # ---- the transition into t = 0: every source regime starts at (mu0, Sigma0); W of the uniform-matrix step ----
    Bsz, n = w_last.shape[0], A.shape[1]
    mu, Sig = em["mu0"].expand(Bsz, K, n), em["Sigma0"].expand(Bsz, K, n, n)
    J, mj, Sj, pair = _sws_pair_step(A, Bm, Q, U[:, 0], mu, Sig, ms, Ss, hist["W"][:, 0], M)
    acc.transition(pair, ms, Ss, J, mj, Sj, U[:, 0], first=True)
    return smooth, acc.s


_EM_STATS = ("N", "S11", "S10", "S00", "counts", "Syz", "Szz", "Syy", "Nobs", "z0", "z0z0", "nseq")
_EM_OUTPUTS = _EM_STATS + ("log_lik_seq",) + _SWS_SMOOTH


class _EmSums:
    """The expected sufficient statistics of include/kvae_lgssm.h kvae_lgssm_switching_em, per sequence ([B, ...]), accumulated by
    _sws_backward step by step."""

    def __init__(self, em, n, m, K, ref):
        Bsz, x = ref.shape[0], n + m
        z = lambda *s: ref.new_zeros(Bsz, *s)
        self.Y, self.mask, self.n = em["Y"], em["mask"], n
        self.s = dict(N=z(K), S11=z(K, n, n), S10=z(K, n, x), S00=z(K, x, x), counts=z(K, K), Syz=z(self.Y.shape[-1], n), Szz=z(n, n),
                      Syy=z(self.Y.shape[-1], self.Y.shape[-1]), Nobs=z(1), z0=z(n), z0z0=z(n, n), nseq=z(1) + 1.0)

    def emission(self, t, m_, V_):
        y = self.Y[:, t]
        ob = torch.ones_like(y[:, 0]) if self.mask is None else (self.mask[:, t] != 0).to(y.dtype)
        y = torch.where(ob[:, None] != 0, y, torch.zeros_like(y))   # selected, as the kernel does: a hidden y adds exactly 0
        s = self.s
        s["Syz"] += y.unsqueeze(-1) * m_.unsqueeze(-2)
        s["Szz"] += ob[:, None, None] * (V_ + m_.unsqueeze(-1) * m_.unsqueeze(-2))
        s["Syy"] += y.unsqueeze(-1) * y.unsqueeze(-2)
        s["Nobs"] += ob[:, None]

    def transition(self, xi, ms, Ss, J, mj, Sj, u, first):
        """xi [B,j,k]; (ms, Ss) [B,k,...] the destination; J, (mj, Sj) [B,j,k,...] the gain and the smoothed source; u [B,m]."""
        s, n = self.s, self.n
        w = xi[..., None, None]
        out = lambda a, b: a.unsqueeze(-1) * b.unsqueeze(-2)
        msx, ux = ms.unsqueeze(1).expand_as(mj), u[:, None, None, :].expand(*mj.shape[:3], u.shape[-1])
        s["N"] += xi.sum(1)
        s["S11"] += xi.sum(1)[..., None, None] * (Ss + out(ms, ms))
        s["S10"][..., :n] += (w * (Ss.unsqueeze(1) @ J.mT + out(msx, mj))).sum(1)
        s["S10"][..., n:] += (w * out(msx, ux)).sum(1)
        zz = w * (Sj + out(mj, mj))
        zu = (w * out(mj, ux)).sum(1)
        s["S00"][..., :n, :n] += zz.sum(1)
        s["S00"][..., :n, n:] += zu
        s["S00"][..., n:, :n] += zu.mT
        s["S00"][..., n:, n:] += (w * out(ux, ux)).sum(1)
        if first:
            s["z0"] += (xi.unsqueeze(-1) * mj).sum((1, 2))
            s["z0z0"] += zz.sum((1, 2))
        else:
            s["counts"] += xi


@torch.no_grad()
def switching_em_statistics_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, want=_EM_OUTPUTS, per_sequence=False):
    """The equations of kvae_lgssm_switching_em (include/kvae_lgssm.h) in torch ops, in the dtype of A: the
    sweep of switching_filter_torch with its history kept, then the smoother's backward pass carried one transition further, into
    t = 0, with the expected sufficient statistics of the switching model accumulated on the way.  The fallback of
    switching_em_statistics and (in float64) the reference its kernel is tested against.  Returns the statistics summed over the
    sequences (per_sequence: with their leading [B]), "log_lik_seq" [B] and the four smoother outputs; entries not asked for are None."""
    want = _want("switching_em_statistics", _EM_OUTPUTS, want)
    full, hist, (A, Bm, Q, Cm, U) = _swf_forward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, None, history=True)
    dt, dev = A.dtype, A.device
    em = dict(mu0=mu0.detach().to(dev, dt), Sigma0=Sigma0.detach().to(dev, dt), Y=Y.detach().to(dev, dt),
              mask=None if mask is None else mask.detach().to(dev, dt).reshape(Y.shape[0], Y.shape[1]))
    smooth, stats = _sws_backward(A, Bm, Q, U, hist, full["regime_filt"][:, -1], em)
    if not per_sequence:
        stats = {k: v.sum(0) for k, v in stats.items()}
    stats.update(smooth, log_lik_seq=full["log_lik_seq"])
    return {k: (stats[k] if k in want else None) for k in _EM_OUTPUTS}


_EM_PARAMS = ("A", "B", "Q", "C", "R", "P", "mu0", "Sigma0")


@torch.no_grad()
def switching_em_mstep(stats, old, update=("A", "B", "Q", "C", "P"), min_count=None):
    """The closed-form M-step of EM for the switching model, in float64 on the statistics' device.  stats: the sums of
    switching_em_statistics (added over batches with em_add); old: dict of the current A [K,n,n], B [K,n,m], Q, C [p,n], R, P [K,K],
    mu0, Sigma0; update: which of them to re-estimate.  Returns (params, skipped): the float64 parameters - the old value where a name
    is not in `update` - and {"regimes": [k, ...], "rows": [j, ...], "B_held": [k, ...], "emission": bool}.
      [A_k B_k] = S10_k S00_k^-1                 Q_k = sym((S11_k - [A_k B_k] S10_k^T) / N_k)
      C = Syz Szz^-1                             R = sym((Syy - C Syz^T) / Nobs)
      P[j, :] = counts[j, :] / sum_k counts[j, k]
      mu0 = z0 / nseq                            Sigma0 = z0z0 / nseq - mu0 mu0^T
    (with only one of A / B, or Q without both, or R without C, named in `update`: the maximiser given the ones held, and the
    general quadratic form for the covariance).  Regime k keeps its old A_k, B_k, Q_k where N_k < min_count (default n + m + 1) or
    the new Q_k fails cholesky_ex (or S00_k cannot be inverted at all); a row of P keeps its old values where its counts sum to 0.
    Without a control input - u = None is zeros, as in forward() - the u-block of S00_k is singular (smallest eigenvalue <= 1e-10 of
    S00_k's largest): B_k is held, A_k is the maximiser given it, Q_k takes the general form, and k is listed under "B_held", not
    under "regimes".  The 1e-10 is a choice, not a measurement: far above float64 rounding of an exactly zero block (the case
    of u = None), far below any u that carries information; a u between the two is fitted jointly and may give a poorly determined B_k.
    A regime whose statistics are not finite is skipped like one below min_count.  C and R keep their old values ("emission": True) where no step is observed, Szz cannot be inverted or the new
    R is not positive definite.  Everything held is listed in `skipped`, which takes a host synchronisation: the M-step cannot be
    captured into a graph."""
    update = _want("switching_em_mstep", _EM_PARAMS, update)
    dev = stats["N"].device
    s = {k: v.detach().to(dev, torch.float64) for k, v in stats.items() if v is not None and k in _EM_STATS}
    o = {k: old[k].detach().to(dev, torch.float64) for k in _EM_PARAMS}
    new = dict(o)
    skipped = {"regimes": [], "rows": [], "B_held": [], "emission": False}
    sym = lambda M: 0.5 * (M + M.mT)
    if any(k in update for k in ("A", "B", "Q")):
        K, n, m = o["A"].shape[0], o["A"].shape[1], o["B"].shape[2]
        min_count = n + m + 1 if min_count is None else min_count
        S11, S10, S00, Nk = s["S11"], s["S10"], s["S00"], s["N"]
        finite = torch.isfinite(S00).all(-1).all(-1) & torch.isfinite(S10).all(-1).all(-1) & torch.isfinite(S11).all(-1).all(-1) & torch.isfinite(Nk)
        low = ~(Nk >= min_count) | ~finite   # a regime with non-finite statistics is skipped like one never visited
        eye = torch.eye(n + m, device=dev, dtype=torch.float64)
        safe00 = torch.where(low[:, None, None], eye.expand_as(S00), S00)
        S10, S11 = torch.where(low[:, None, None], torch.zeros_like(S10), S10), torch.where(low[:, None, None], torch.zeros_like(S11), S11)
        # without a control input (u = 0, or the same u at every step up to rounding) the u-block of S00_k is singular and B_k
        # cannot be told from the data: it is held, and A_k is the maximiser given it
        flat = torch.linalg.eigvalsh(sym(safe00[:, n:, n:]))[:, 0] <= 1e-10 * torch.linalg.eigvalsh(sym(safe00))[:, -1].clamp_min(1e-300)
        Fo = torch.cat([o["A"], o["B"]], -1)

        def solved(S, X):   # X S^-1 per regime, and where it could not be had
            sol, info = torch.linalg.solve_ex(S, X, left=False)
            return sol, (info != 0) | ~torch.isfinite(sol).all(-1).all(-1)

        uu_safe = torch.where(flat[:, None, None], eye[:m, :m].expand(K, m, m), safe00[:, n:, n:])
        Fa, bad_a = solved(safe00[:, :n, :n], S10[..., :n] - o["B"] @ safe00[:, n:, :n])
        Fa = torch.cat([Fa, o["B"]], -1)
        if "A" in update and "B" in update:
            Fj, bad_j = solved(torch.where(flat[:, None, None], eye.expand_as(S00), safe00), S10)
            F, unsolved = torch.where(flat[:, None, None], Fa, Fj), torch.where(flat, bad_a, bad_j)
        elif "A" in update:
            F, unsolved = Fa, bad_a
        elif "B" in update:
            Fb, bad_b = solved(uu_safe, S10[..., n:] - o["A"] @ safe00[:, :n, n:])
            F, unsolved = torch.where(flat[:, None, None], Fo, torch.cat([o["A"], Fb], -1)), bad_b & ~flat
        else:
            F, unsolved = Fo, torch.zeros_like(low)
        F = torch.where(unsolved[:, None, None], Fo, F)
        joint = ~flat if ("A" in update and "B" in update) else torch.zeros_like(flat)   # where F is the joint maximiser
        Nsafe = torch.where(low, torch.ones_like(Nk), Nk)[:, None, None]
        Qn = torch.where(joint[:, None, None], sym((S11 - F @ S10.mT) / Nsafe),
                         sym((S11 - F @ S10.mT - S10 @ F.mT + F @ S00 @ F.mT) / Nsafe))
        info = torch.linalg.cholesky_ex(Qn).info
        bad = low | unsolved | (info != 0) | ~torch.isfinite(Qn).all(-1).all(-1)
        keep = bad[:, None, None]
        if "A" in update:
            new["A"] = torch.where(keep, o["A"], F[..., :n])
        if "B" in update:
            new["B"] = torch.where(keep, o["B"], F[..., n:])
        if "Q" in update:
            new["Q"] = torch.where(keep, o["Q"], Qn)
        skipped["regimes"] = [int(k) for k in torch.nonzero(bad).flatten().tolist()]
        if "B" in update:
            skipped["B_held"] = [int(k) for k in torch.nonzero(flat & ~bad).flatten().tolist()]
    if "C" in update or "R" in update:
        Cn, Syz, nobs = o["C"], s["Syz"], s["Nobs"].sum()
        lost = ~(nobs > 0)
        if "C" in update:   # C = Syz Szz^-1; held, with R, where Szz cannot be inverted (too few observed steps)
            Cs, info = torch.linalg.solve_ex(s["Szz"], Syz, left=False)
            lost = lost | (info != 0) | ~torch.isfinite(Cs).all()
            Cn = torch.where(lost, o["C"], Cs)
            new["C"] = Cn
        if "R" in update:
            quad = s["Syy"] - Cn @ Syz.mT if "C" in update else s["Syy"] - Cn @ Syz.mT - Syz @ Cn.mT + Cn @ s["Szz"] @ Cn.mT
            Rn = sym(quad / torch.where(lost, torch.ones_like(nobs), nobs))
            lost = lost | (torch.linalg.cholesky_ex(Rn).info != 0) | ~torch.isfinite(Rn).all()
            new["R"] = torch.where(lost, o["R"], Rn)
            if "C" in update:
                new["C"] = torch.where(lost, o["C"], Cn)
        skipped["emission"] = bool(lost)
    if "P" in update:
        rows = s["counts"].sum(1)
        empty = ~(rows > 0)
        new["P"] = torch.where(empty[:, None], o["P"], s["counts"] / torch.where(empty, torch.ones_like(rows), rows)[:, None])
        skipped["rows"] = [int(j) for j in torch.nonzero(empty).flatten().tolist()]
    if "mu0" in update or "Sigma0" in update:
        mean = s["z0"] / s["nseq"]
        if "Sigma0" in update:
            ref = mean if "mu0" in update else o["mu0"]   # around the mean kept: E (z - mu0)(z - mu0)^T
            new["Sigma0"] = sym(s["z0z0"] / s["nseq"] - torch.outer(mean, ref) - torch.outer(ref, mean) + torch.outer(ref, ref))
        if "mu0" in update:
            new["mu0"] = mean
    return new, skipped


def switching_log_marginal_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None):
    """switching_log_marginal in torch ops, DIFFERENTIABLE, in the dtype of A: dict(ll [B,T], seq_ll [B], levels [B,T]) - the log_lik,
    log_lik_seq and levels of switching_filter_torch without a carried state - with a tape through A, Bm, Q, Cm, P, mu0, Sigma0, Y
    and U (R is a buffer of the model).  The fallback of switching_log_marginal and (in float64) the reference its adjoint kernel is
    tested against.  It is the gradient of the GPB2 VALUE: where the filter is exact (P = I, shared A / B / Q, t <= 1) the exact
    gradient of log p(a | u), elsewhere the gradient of the approximation.
    The sweep of _swf_forward without the detaches, restated where autograd would otherwise give NaN: the ladder levels are found
    without a tape and S + jitter[level] I is factorised once (as log_marginal_torch); every -inf (a zero of P, a dead column) is
    kept out of the taped arithmetic by selects, so that its gradient is 0.  Q and Sigma0 enter through their symmetric part (the
    same numbers for symmetric matrices): their gradients are the gradients over symmetric matrices, hence symmetric."""
    dt, dev = A.dtype, Y.device
    K, n = A.shape[0], A.shape[1]
    Bsz, T, p = Y.shape
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U = (t.to(device=dev, dtype=dt) for t in (A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U))
    R = R.detach()
    Q, Sigma0 = 0.5 * (Q + Q.mT), 0.5 * (Sigma0 + Sigma0.mT)
    mask = None if mask is None else mask.detach().to(device=dev, dtype=dt).reshape(Bsz, T)
    lw = torch.full((Bsz, K), 1.0 / K, device=dev, dtype=dt).log()
    mu, Sig = mu0.expand(Bsz, K, n), Sigma0.expand(Bsz, K, n, n)
    eye, eyeP, eyeK = torch.eye(n, device=dev, dtype=dt), torch.eye(p, device=dev, dtype=dt), torch.eye(K, device=dev, dtype=dt)
    uniform = torch.full((K, K), 1.0 / K, device=dev, dtype=dt)
    jitters = torch.tensor([*_jitter_ladder(), 0.0], device=dev, dtype=torch.float64)
    zero = torch.zeros((), device=dev, dtype=dt)
    lls, levels = [], []
    for t in range(T):
        Pt = uniform if t == 0 else P
        mk = torch.ones(Bsz, device=dev, dtype=dt) if mask is None else mask[:, t]
        observed = mk != 0
        # ---- the K^2 filter steps: [B, i, j, ...] ----
        mp = torch.einsum("jrc,bic->bijr", A, mu) + torch.einsum("jrc,bc->bjr", Bm, U[:, t]).unsqueeze(1)
        Sp = torch.einsum("jre,biec,jdc->bijrd", A, Sig, A) + Q
        ap = mp @ Cm.mT
        res = Y[:, t, None, None, :] - ap
        S = Cm @ Sp @ Cm.mT + R
        S = 0.5 * (S + S.mT)
        with torch.no_grad():
            _, lv = safe_cholesky_items(S)
        St = S + (jitters[lv.long()][..., None, None] * eyeP.double()).to(dt)
        clamped = torch.diag_embed(torch.diagonal(S, dim1=-2, dim2=-1).clamp(min=1e-6))
        St = torch.where((lv == 5)[..., None, None], clamped, St)
        lij = _observed_only(_gauss_ll(torch.linalg.cholesky(St), res)[0], observed[:, None, None])
        Kg = torch.linalg.solve(S, Cm @ Sp).mT * mk[:, None, None, None, None]
        muf = mp + (Kg @ res.unsqueeze(-1)).squeeze(-1)
        IKC = eye - Kg @ Cm
        Sf = IKC @ Sp @ IKC.mT + Kg @ R @ Kg.mT
        Sf = 0.5 * (Sf + Sf.mT)
        # ---- weights: an impossible pair (P[i,j] = 0, or regime i dead) is masked out, never added as -inf ----
        possible = (Pt > 0) & torch.isfinite(lw.detach()).unsqueeze(-1)               # [B, i, j]
        logc = torch.where(possible, torch.where(possible, lw.unsqueeze(-1), zero) + torch.where(Pt > 0, Pt, torch.ones_like(Pt)).log() + lij, zero)
        with torch.no_grad():
            pw = lw.exp().unsqueeze(-1) * Pt
            cmx = torch.where(possible, logc, torch.full_like(logc, -float("inf"))).amax(1)   # [B, j]
            dead = ~possible.any(1)
            shift = torch.where(dead, torch.zeros_like(cmx), cmx)
        ex = torch.where(possible, (logc - shift.unsqueeze(1)).exp(), zero)
        ex = torch.where(dead.unsqueeze(1), eyeK.expand(Bsz, K, K), ex)
        se = ex.sum(1)
        W = ex / se.unsqueeze(1)
        with torch.no_grad():
            mx = torch.where(dead, torch.full_like(cmx, -float("inf")), cmx).amax(-1, keepdim=True)
        col = torch.where(dead, zero, se * (shift - mx).exp())                       # a dead column adds nothing
        tot = mx.squeeze(-1) + col.sum(-1).log()
        lw = torch.where(dead, torch.full_like(cmx, -float("inf")), (shift + torch.where(dead, torch.ones_like(se), se).log()) - tot.unsqueeze(-1))
        # ---- collapse over i ----
        mu = (W.unsqueeze(-1) * muf).sum(1)
        d = muf - mu.unsqueeze(1)
        Sig = (W[..., None, None] * (Sf + d.unsqueeze(-1) * d.unsqueeze(-2))).sum(1)
        Sig = 0.5 * (Sig + Sig.mT)
        lls.append(torch.where(observed, tot, torch.zeros_like(tot)))
        levels.append(torch.where(pw > 0, lv, torch.zeros_like(lv)).amax((1, 2)))
    ll = torch.stack(lls, 1)
    return {"ll": ll, "seq_ll": ll.sum(1), "levels": torch.stack(levels, 1)}



_SPF_OUTPUTS = ("log_lik", "log_lik_seq", "regime_filt", "mus_filt", "Sigmas_filt", "ess", "resampled", "regimes", "ancestors", "levels",
                "paths", "path_log_w", "state")
_SPF_FORCE = ("regimes", "resampled", "ancestors")
SPF_PARTICLES = (64, 128, 256)


def _spf_state(state, Bsz, G, N, n):
    if state is None:
        return None
    lw, reg, mu, Sig = state["log_w"], state["regime"], state["mu"], state["Sigma"]
    if lw.shape != (Bsz, G, N) or reg.shape != (Bsz, G, N) or mu.shape != (Bsz, G, N, n) or Sig.shape != (Bsz, G, N, n, n):
        raise ValueError(f"switching_pf: state must hold log_w [{Bsz},{G},{N}], regime [{Bsz},{G},{N}], mu [{Bsz},{G},{N},{n}], Sigma "
                         f"[{Bsz},{G},{N},{n},{n}], got {tuple(lw.shape)}, {tuple(reg.shape)}, {tuple(mu.shape)}, {tuple(Sig.shape)}")
    return lw, reg, mu, Sig


def _spf_draws(pf_regime, pf_resample, Bsz, T):
    if pf_regime.dim() != 4 or pf_regime.shape[0] != Bsz or pf_regime.shape[2] != T:
        raise ValueError(f"switching_pf: pf_regime must be [B,G,T,N] = [{Bsz},G,{T},N], got {tuple(pf_regime.shape)}")
    G, N = pf_regime.shape[1], pf_regime.shape[3]
    if pf_resample.shape != (Bsz, G, T):
        raise ValueError(f"switching_pf: pf_resample must be [{Bsz},{G},{T}], got {tuple(pf_resample.shape)}")
    return G, N


def lineages(regimes, ancestors):
    """paths [B,G,N,T] of the final slots: slot n's lineage walked back over ancestors [B,G,T,N] / regimes [B,G,T,N] -
    i = n; for t = T-1 .. 0: i = ancestors_t[i], paths[n, t] = regimes_t[i]."""
    Bsz, G, T, N = regimes.shape
    i = torch.arange(N, device=regimes.device).expand(Bsz, G, N)
    cols = [None] * T
    for t in range(T - 1, -1, -1):
        i = ancestors[:, :, t].long().gather(-1, i)
        cols[t] = regimes[:, :, t].gather(-1, i)
    return torch.stack(cols, -1)


@torch.no_grad()
def switching_pf_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, pf_regime, pf_resample, mask=None, ess_threshold=0.5, state=None,
                       want=_SPF_OUTPUTS, force=None, margins=False):
    """The equations of kvae_lgssm_switching_pf (include/kvae_lgssm.h) in torch ops, vectorised over (B, G, particle, regime), in
    the dtype of A: shapes outside the kernel's, non-fp32 and host tensors, and (in float64) the reference the kernel is tested
    against.  The per-regime Kalman steps use the helpers of switching_filter_torch.  T steps of about forty small launches.
    Same arguments and returns as switching_pf.  force: a dict with any of "regimes" [B,G,T,N], "resampled" [B,G,T], "ancestors"
    [B,G,T,N] - recorded decisions replayed in place of this run's own (a free-running comparison of two precisions is meaningless
    once one boundary decision differs).  margins: also return "margin_regime" [B,G,T,N] (the distance of theta sum_j e_j from the
    nearest boundary of the cumulative e, over sum_j e_j), "margin_ancestor" [B,G,T,N] (of the position from the nearest cumulative
    weight) and "margin_ess" [B,G,T] (|ess - ess_threshold N|): how close this run's decisions were to going the other way."""
    want = _want("switching_pf", _SPF_OUTPUTS, want)
    force = {} if force is None else dict(force)
    if any(k not in _SPF_FORCE for k in force):
        raise ValueError(f"switching_pf_torch: force may hold {_SPF_FORCE}, got {tuple(force)}")
    if not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError(f"switching_pf: ess_threshold must be in [0, 1], got {ess_threshold}")
    dt, dev = A.dtype, Y.device
    K, n = A.shape[0], A.shape[1]
    Bsz, T, p = Y.shape
    G, N = _spf_draws(pf_regime, pf_resample, Bsz, T)
    A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, pf_regime, pf_resample = (
        t.detach().to(device=dev, dtype=dt) for t in (A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, pf_regime, pf_resample))
    mask = None if mask is None else mask.detach().to(device=dev, dtype=dt).reshape(Bsz, T)
    st = _spf_state(state, Bsz, G, N, n)
    nlogN = -torch.tensor(float(N), device=dev, dtype=dt).log()
    if st is None:
        lw = nlogN.expand(Bsz, G, N)
        reg = torch.zeros(Bsz, G, N, device=dev, dtype=torch.long)
        mu, Sig = mu0.expand(Bsz, G, N, n), Sigma0.expand(Bsz, G, N, n, n)
    else:
        lw, mu, Sig = (t.detach().to(device=dev, dtype=dt) for t in (st[0], st[2], st[3]))
        reg = st[1].detach().to(dev).long()
    eye = torch.eye(n, device=dev, dtype=dt)
    logP = P.log()
    luni = torch.full((), 1.0 / K, device=dev, dtype=dt).log()
    slots = torch.arange(N, device=dev)
    inf = float("inf")
    outs = {k: [] for k in ("log_lik", "regime_filt", "mus_filt", "Sigmas_filt", "ess", "resampled", "regimes", "ancestors", "levels",
                            "margin_regime", "margin_ancestor", "margin_ess")}
    for t in range(T):
        mk = torch.ones(Bsz, device=dev, dtype=dt) if mask is None else mask[:, t]
        observed = mk != 0
        # ---- every particle under every regime: [B, G, i, j, ...] ----
        mp = torch.einsum("jrc,bgic->bgijr", A, mu) + torch.einsum("jrc,bc->bjr", Bm, U[:, t])[:, None, None]
        Sp = torch.einsum("jre,bgiec,jdc->bgijrd", A, Sig, A) + Q
        res = Y[:, t, None, None, None, :] - mp @ Cm.mT
        S = Cm @ Sp @ Cm.mT + R
        S = 0.5 * (S + S.mT)
        L, lv = safe_cholesky_items(S)
        lij = _observed_only(_gauss_ll(L, res)[0], observed[:, None, None, None])
        lp = luni.expand(Bsz, G, N, K) if (t == 0 and st is None) else logP[reg]
        logc = lp + lij
        mx = logc.amax(-1, keepdim=True)
        e = (logc - mx).exp()
        se = e[..., 0]
        for j in range(1, K):
            se = se + e[..., j]
        inc = mx.squeeze(-1) + se.log()
        # ---- the weights ----
        a = lw + inc
        top = a.amax(-1, keepdim=True)
        ex = (a - top).exp()
        tot = ex.sum(-1, keepdim=True)
        ll = (top + tot.log()).squeeze(-1)
        lwn = (a - top) - tot.log()
        Wn = ex / tot
        rf = (Wn.unsqueeze(-1) * (e / se.unsqueeze(-1))).sum(2)
        ess = 1.0 / (Wn * Wn).sum(-1)
        # ---- the draw ----
        thr = pf_regime[:, :, t] * se
        cs = torch.zeros_like(se)
        s = torch.full_like(reg, -1)
        last = torch.zeros_like(reg)
        gap = torch.full_like(se, inf)
        for j in range(K):
            cs = cs + e[..., j]
            s = torch.where((s < 0) & (cs > thr), torch.full_like(s, j), s)
            last = torch.where(e[..., j] > 0, torch.full_like(last, j), last)
            if j < K - 1:
                gap = torch.minimum(gap, (cs - thr).abs())
        s = torch.where(s < 0, last, s)
        if "regimes" in force:
            s = force["regimes"][:, :, t].to(dev).long()
        # ---- the measurement update under the drawn regime ----
        pick = lambda v: v.gather(3, s.reshape(Bsz, G, N, 1, *([1] * (v.dim() - 4))).expand(Bsz, G, N, 1, *v.shape[4:])).squeeze(3)
        mps, Sps, Ss, rs_ = pick(mp), pick(Sp), pick(S), pick(res)
        Kg = torch.linalg.solve(Ss, Cm @ Sps).mT * mk[:, None, None, None, None]
        muf = mps + (Kg @ rs_.unsqueeze(-1)).squeeze(-1)
        IKC = eye - Kg @ Cm
        Sf = IKC @ Sps @ IKC.mT + Kg @ R @ Kg.mT
        Sf = 0.5 * (Sf + Sf.mT)
        m_ = (Wn.unsqueeze(-1) * muf).sum(2)
        dd = muf - m_.unsqueeze(2)
        V = (Wn[..., None, None] * (Sf + dd.unsqueeze(-1) * dd.unsqueeze(-2))).sum(2)
        # ---- systematic resampling ----
        if ess_threshold >= 1.0:
            rs = torch.ones(Bsz, G, device=dev, dtype=torch.bool)
        elif ess_threshold <= 0.0:
            rs = torch.zeros(Bsz, G, device=dev, dtype=torch.bool)
        else:
            rs = ess < ess_threshold * N
        if "resampled" in force:
            rs = force["resampled"][:, :, t].to(dev) != 0
        cum = Wn.cumsum(-1)
        pos = (pf_resample[:, :, t, None] + slots.to(dt)) / N
        anc = torch.searchsorted(cum, pos.contiguous(), right=True).clamp(max=N - 1)
        above = torch.where(anc < N - 1, (cum.gather(-1, anc) - pos).abs(), torch.full_like(pos, inf))   # the last slot takes the rest
        below = torch.where(anc > 0, (pos - cum.gather(-1, (anc - 1).clamp(min=0))).abs(), torch.full_like(pos, inf))
        if "ancestors" in force:
            anc = force["ancestors"][:, :, t].to(dev).long()
        anc = torch.where(rs.unsqueeze(-1), anc, slots.expand(Bsz, G, N))
        mu = muf.gather(2, anc[..., None].expand(Bsz, G, N, n))
        Sig = Sf.gather(2, anc[..., None, None].expand(Bsz, G, N, n, n))
        reg = s.gather(2, anc)
        lw = torch.where(rs.unsqueeze(-1), nlogN.expand(Bsz, G, N), lwn)
        # ---- outputs of the step ----
        outs["log_lik"].append(torch.where(observed.unsqueeze(-1), ll, torch.zeros_like(ll)))
        outs["regime_filt"].append(rf), outs["mus_filt"].append(m_), outs["Sigmas_filt"].append(V), outs["ess"].append(ess)
        outs["resampled"].append(rs), outs["regimes"].append(s.to(torch.int32)), outs["ancestors"].append(anc.to(torch.int32))
        outs["levels"].append(torch.where(lp > -inf, lv, torch.zeros_like(lv)).amax((2, 3)))
        outs["margin_regime"].append(gap / se), outs["margin_ancestor"].append(torch.minimum(above, below))
        outs["margin_ess"].append((ess - ess_threshold * N).abs())
    full = {k: torch.stack(v, 2) for k, v in outs.items()}
    full["log_lik_seq"] = full["log_lik"].sum(2)
    full["paths"] = lineages(full["regimes"], full["ancestors"])
    full["path_log_w"] = lw
    full["state"] = {"log_w": lw, "regime": reg.to(torch.int32), "mu": mu, "Sigma": Sig}
    out = {k: (full[k] if k in want else None) for k in _SPF_OUTPUTS}
    if margins:
        out.update({k: full[k] for k in ("margin_regime", "margin_ancestor", "margin_ess")})
    return out
