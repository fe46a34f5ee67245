"""One-step-ahead prediction diagnostics: the shipped counterpart of the reference's kalman_prediction_test
(kvae/train/testing.py:100-177 there), which its epoch loop calls every five epochs to report the one-step-ahead MSE of the
latents against a persistence baseline.  The reference predicts from SMOOTHED means, which have seen the future; this one
predicts from the FILTER (KVAE.score: a_pred_t = C_t mu_{t|t-1} has seen a_{0:t-1} only), and adds the exact predictive
log-likelihood and the mean normalised innovation squared (2 = a_dim for a calibrated model).
"""
import torch


def _frames(model, batch_or_x):
    """x [B,T,...] on the model's device, from x itself or a batch: a dict with "images", or a tuple whose first entry is x."""
    if isinstance(batch_or_x, dict):
        x = batch_or_x["images"]
    elif isinstance(batch_or_x, (tuple, list)):
        x = batch_or_x[0]
    else:
        x = batch_or_x
    return x.to(next(model.parameters()).device)


@torch.no_grad()
def prediction_scores(model, batch_or_x, mask=None, u=None):
    """Scores of the filter's one-step-ahead predictions on x [B,T,...] (or a batch: a dict with "images", or a tuple whose
    first entry is x); mask [B,T] (1 = observed) and u [B,T,m] optional.  Predictions come from the filter, not from smoothed
    means.  Python floats:
      mse_kf            mean squared error of a_pred_t against the encoding a_vae_t over observed steps t >= 1
      mse_naive         the same for the persistence prediction a_vae_{t-1}
      log_lik_per_step  sum of log p(a_t | a_{0:t-1}, u) over observed steps / their number
      nis_mean          mean normalised innovation squared over observed steps"""
    sc = model.score(_frames(model, batch_or_x), u=u, mask=mask)
    a, a_pred = sc["a_vae"], sc["a_pred"].to(sc["a_vae"].dtype)
    Bsz, T = a.shape[:2]
    mk = torch.ones(Bsz, T, device=a.device, dtype=a.dtype) if mask is None else mask.to(device=a.device, dtype=a.dtype)
    w = mk[:, 1:]
    count = (w.sum() * a.shape[-1]).clamp(min=1.0)
    mse_kf = (((a_pred[:, 1:] - a[:, 1:]) ** 2).sum(-1) * w).sum() / count
    mse_naive = (((a[:, :-1] - a[:, 1:]) ** 2).sum(-1) * w).sum() / count
    n_obs = mk.sum().clamp(min=1.0)
    return {"mse_kf": float(mse_kf), "mse_naive": float(mse_naive), "log_lik_per_step": float(sc["log_lik"].sum() / n_obs),
            "nis_mean": float(sc["nis"].sum() / n_obs)}


@torch.no_grad()
def regime_filter_scores(model, batch_or_x, mask=None, u=None):
    """The generative switching model against its amortised regime posterior on x [B,T,...] (or a batch, as prediction_scores
    takes it): KVAE.filter_regimes - causal, the regimes summed out - next to KVAE.score and KVAE.decode_regimes, which go
    through the bidirectional posterior network.  Switching dynamics only.  Python floats:
      log_lik_per_step       sum of the regime-marginal log p(a_t | a_{0:t-1}, u) over observed steps / their number
      log_lik_per_step_map   the same for score(): the density conditional on the posterior's most likely regime path
      regime_agreement       share of steps whose causal argmax regime equals decode_regimes' path
      regime_kl              mean over steps of KL(q(s_t) || p(s_t | a_{0:t})), q(s_t) the posterior network's marginals"""
    x = _frames(model, batch_or_x)
    fr = model.filter_regimes(x, u=u, mask=mask)
    sc =model.score(x, u=u, mask=mask, regimes="map")
    dec = model.decode_regimes(x, u=u, mask=mask, smooth=False)
    n_obs = fr["n_obs"].sum().clamp(min=1.0)
    q, pf = dec["regime_probs"].double(), fr["regime_filt"].double()
    tiny = torch.finfo(torch.float32).tiny
    kl = (q * (q.clamp_min(tiny).log() - pf.clamp_min(tiny).log())).sum(-1)
    return {"log_lik_per_step": float(fr["log_lik_seq"].sum() / n_obs),
            "log_lik_per_step_map": float(sc["log_lik_seq"].sum() / n_obs),
            "regime_agreement": float((fr["regimes"] == dec["regimes"]).double().mean()),
            "regime_kl": float(kl.mean())}


def particle_filter_scores(model, batch_or_x, mask=None, u=None, num_particles=256, replicates=4, ess_threshold=0.5):
    """The size of the GPB2 approximation on x [B,T,...] (or a batch, as prediction_scores takes it): KVAE.particle_filter_regimes
    - unbiased in the likelihood, consistent in the regimes - next to KVAE.filter_regimes.  Switching dynamics only.  Python floats:
      log_lik_per_step_pf    sum over sequences of log_lik_seq_mean (the logmeanexp over the replicates) / observed steps
      log_lik_per_step_gpb2  the same for filter_regimes' log_lik_seq
      gpb2_gap_per_step      their difference, particle filter minus GPB2
      pf_std                 the spread of log_lik_seq over the replicates (standard deviation, mean over sequences; 0 for one)
      regime_tv              mean over (b, t) of the total variation between regime_filt_mean and filter_regimes' regime_filt
      ess_mean               mean effective sample size over replicates and steps"""
    x = _frames(model, batch_or_x)
    pf = model.particle_filter_regimes(x, u=u, mask=mask, num_particles=num_particles, replicates=replicates, ess_threshold=ess_threshold)
    fr = model.filter_regimes(x, u=u, mask=mask)
    n_obs = fr["n_obs"].sum().clamp(min=1.0)
    seq = pf["log_lik_seq"].double()
    ll_pf, ll_gpb2 = float(pf["log_lik_seq_mean"].double().sum() / n_obs), float(fr["log_lik_seq"].double().sum() / n_obs)
    tv = 0.5 * (pf["regime_filt_mean"].double() - fr["regime_filt"].double()).abs().sum(-1)
    return {"log_lik_per_step_pf": ll_pf, "log_lik_per_step_gpb2": ll_gpb2, "gpb2_gap_per_step": ll_pf - ll_gpb2,
            "pf_std": float(seq.std(1, unbiased=True).mean()) if seq.shape[1] > 1 else 0.0,
            "regime_tv": float(tv.mean()), "ess_mean": float(pf["ess"].double().mean())}


@torch.no_grad()
def forecast_scores(model, batch_or_x, horizon, mask=None, u=None):
    """Forecast skill against horizon on x [B,T,...] (or a batch, as prediction_scores takes it): KVAE.forecast_regimes from every
    origin, scored against the encoded frames it forecasts - the counterpart of prediction_scores for h > 1.  Switching dynamics
    only.  u [B,T+horizon,m] or None.  Python lists of length `horizon`, entry h-1 over the valid (b, t) - the target t+h lies
    inside the sequence and is observed:
      mse        mean squared error of a_fore against the encoded target, per component of a
      mse_naive  the same for persistence (a_t as the forecast of a_{t+h}), over those of the targets whose origin is observed
      log_lik    mean of log p(a_{t+h} | a_{0:t}, u)
      nis_mean   mean of r^T S_fore^-1 r, r = a_{t+h} - a_fore: p (= 2) when the forecast is calibrated
      count      the number of valid (b, t)
    A horizon without a valid target gives count 0 and nan elsewhere."""
    x = _frames(model, batch_or_x)
    dev = x.device
    H = int(horizon)
    fc = model.forecast_regimes(x, H, u=u, mask=mask)
    a = fc["a_vae"].double()
    Bsz, T, p = a.shape
    target = (torch.arange(T, device=dev)[:, None] + torch.arange(1, H + 1, device=dev)[None, :]).clamp(max=T - 1)   # [T,H]
    valid = fc["valid"]
    r = a[:, target] - fc["a_fore"].double()                                                   # [B,T,H,p]
    nis = (r.unsqueeze(-2) @ torch.linalg.solve(fc["S_fore"].double(), r.unsqueeze(-1))).reshape(Bsz, T, H)
    origin = valid if mask is None else valid & (mask.to(dev)[:, :, None] != 0)
    naive = a[:, target] - a[:, :, None, :]
    mean = lambda v, w: (torch.where(w, v, torch.zeros_like(v)).sum((0, 1)) / w.sum((0, 1))).tolist()
    return {"mse": mean((r * r).mean(-1), valid), "mse_naive": mean((naive * naive).mean(-1), origin),
            "log_lik": mean(fc["log_lik_fore"].double(), valid), "nis_mean": mean(nis, valid), "count": valid.sum((0, 1)).tolist()}


@torch.no_grad()
def viterbi_scores(model, batch_or_x, mask=None, u=None):
    """Four segmentations of x [B,T,...] (or a batch, as prediction_scores takes it) under ONE yardstick, the exact joint
    log p(a, s = path | u) of the generative switching model (KalmanFilter.path_log_joint): the path of KVAE.viterbi_regimes, the
    path of KVAE.decode_regimes (the amortised posterior network's) and the per-step argmax of filter_regimes' regime_filt and of
    smooth_regimes' regime_smooth (which need not be paths the prior allows: their joint may be -inf).  Switching dynamics only.
    Python floats:
      log_joint_<name>  mean over sequences of the exact joint of that segmentation, <name> in viterbi, decode, filter, smooth
      agreement_<name>  share of steps on which it equals the Viterbi path (1 for viterbi itself)
      log_lik           mean over sequences of filter_regimes' log_lik_seq = log p(a | u) with the regimes summed out: the upper
                        reference of every joint (up to the GPB2 error)"""
    x = _frames(model, batch_or_x)
    vit = model.viterbi_regimes(x, u=u, mask=mask, smooth=False)
    sm = model.smooth_regimes(x, u=u, mask=mask)
    paths = {"viterbi": vit["regimes"], "decode": model.decode_regimes(x, u=u, mask=mask, smooth=False)["regimes"],
             "filter": model._argmax_lowest(sm["regime_filt"]), "smooth": sm["regimes"]}
    kf, a = model.kalman_filter, vit["a_vae"]
    uu = torch.zeros(a.shape[0], a.shape[1], model.u_dim, device=a.device, dtype=a.dtype) if u is None else u.to(device=a.device, dtype=a.dtype)
    out = {"log_lik": float(sm["log_lik_seq"].double().mean())}
    for name, path in paths.items():   # (a pinned path takes no draw: the training flag plays no part)
        out["log_joint_" + name] = float(kf.path_log_joint(a, uu, path, mask).double().mean())
        out["agreement_" + name] = float((path == paths["viterbi"]).double().mean())
    return out
