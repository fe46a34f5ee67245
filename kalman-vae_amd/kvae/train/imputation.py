"""Frame-mask builders of the reference's imputation tooling (kvae/train/imputation.py:4-36 there): the input
pattern of BASELINE configs[3] ("observe, hide a block, observe again") and of masked training.  Same function
names, arguments and results; everything else in that module (imputation plots, MSE reports) is evaluation tooling
outside the hot path and is not shipped.  `config_block_mask` wires KVAEConfig.t_init_mask / t_steps_mask in.
`sample_imputation_scores` (no counterpart there) scores the sampled completions of KVAE.sample_imputations,
`regime_smoother_scores` the switching smoother of KVAE.smooth_regimes on the hidden frames.
"""
import torch


def mask_impute_planning(batch_size, T, t_init_mask=4, t_steps_mask=12, device=None):
    """[B,T] mask, 1 = observed: frames [t_init_mask, t_init_mask + t_steps_mask) hidden, clipped at T."""
    t = torch.arange(T, device=device)
    hidden = (t >= t_init_mask) & (t < min(t_init_mask + t_steps_mask, T))
    return (~hidden).to(torch.float32).expand(batch_size, T).contiguous()


def mask_impute_random(batch_size, T, t_init_mask=4, drop_prob=0.5, device=None):
    """First t_init_mask frames observed; every later frame dropped independently with probability drop_prob."""
    mask = torch.ones(batch_size, T, device=device)
    if T > t_init_mask:
        keep = torch.full((batch_size, T - t_init_mask), 1.0 - drop_prob, device=device)
        mask[:, t_init_mask:] = torch.bernoulli(keep)
    return mask


def make_training_mask(batch_size, T, t_init_mask=4, drop_prob=0.0, device=None, strategy="random", t_steps_mask=12):
    if strategy.lower() == "block":
        return mask_impute_planning(batch_size, T, t_init_mask=t_init_mask, t_steps_mask=t_steps_mask, device=device)
    if drop_prob <= 0:
        return torch.ones(batch_size, T, device=device)
    return mask_impute_random(batch_size, T, t_init_mask=t_init_mask, drop_prob=drop_prob, device=device)


def config_block_mask(config, batch_size, T, device=None):
    """The block mask the reference's epoch loop evaluates imputation with (train.py:318-322 there):
    KVAEConfig.t_init_mask observed frames, then KVAEConfig.t_steps_mask hidden ones."""
    return mask_impute_planning(batch_size, T, t_init_mask=config.t_init_mask, t_steps_mask=config.t_steps_mask,
                                device=device)


def sample_imputation_scores(x, x_samples, mask):
    """Scores of S sampled completions x_samples [B,S,T,...] of x [B,T,...] on the HIDDEN frames (mask [B,T], 1 = observed):
    the three numbers to report next to the reference's impute_epoch MSE (of the decoded smoothed mean).
      mse_mean   MSE of the ensemble mean frame
      mse_best   best-of-S MSE: per sequence the sample closest to x over its hidden frames, averaged over sequences
      std        mean per-pixel standard deviation over the S samples (0 for S = 1)
    0-d tensors; 0 where nothing is hidden.  Pure torch, no host sync."""
    hid = (1.0 - mask.to(device=x.device, dtype=x.dtype))                 # [B,T]
    pix = x[0, 0].numel()
    w = hid.reshape(*hid.shape, *([1] * (x.dim() - 2)))                   # [B,T,1,..]
    count = (hid.sum() * pix).clamp(min=1.0)
    err_mean = ((x_samples.mean(1) - x) ** 2 * w).sum() / count
    per = ((x_samples - x.unsqueeze(1)) ** 2 * w.unsqueeze(1)).flatten(2).sum(-1)          # [B,S] squared error on hidden frames
    per_count = (hid.sum(1) * pix).clamp(min=1.0)                                          # [B]
    has = (hid.sum(1) > 0).to(x.dtype)
    best = ((per.min(1).values / per_count) * has).sum() / has.sum().clamp(min=1.0)
    std = x_samples.std(1, unbiased=False) if x_samples.shape[1] > 1 else torch.zeros_like(x)
    return {"mse_mean": err_mean, "mse_best": best, "std": (std * w).sum() / count}


@torch.no_grad()
def regime_smoother_scores(model, x, mask, u=None):
    """The generative switching model's own smoother (KVAE.smooth_regimes) next to the read-outs that go through the regime
    posterior network, on the HIDDEN frames of x [B,T,...] (mask [B,T], 1 = observed).  Switching dynamics only.  Python floats:
      mse_smooth         MSE of x_smooth: the decoded smoothed latent, which has seen the frames after the gap
      mse_impute         MSE of impute()'s x_imputed (the reference's imputation, one drawn regime sequence)
      mse_pred           MSE of filter_regimes' one-step-ahead forecast x_pred, which has not
      regime_agreement   share of steps whose smoothed argmax regime equals decode_regimes' most likely path
    0 for the errors where nothing is hidden.  The model's training mode is left as it was."""
    dev = next(model.parameters()).device
    x, mask = x.to(dev), mask.to(dev)
    was_training = model.training
    try:
        sm = model.smooth_regimes(x, u=u, mask=mask, decode=True)
        fr = model.filter_regimes(x, u=u, mask=mask, decode=True)
        dec = model.decode_regimes(x, u=u, mask=mask, smooth=False)
        imp = model.impute(x, mask, u=u)
    finally:
        model.train(was_training)
    hid = 1.0 - mask.to(x.dtype)
    w = hid.reshape(*hid.shape, *([1] * (x.dim() - 2)))
    count = (hid.sum() * x[0, 0].numel()).clamp(min=1.0)
    mse = lambda y: float((((y.to(x.dtype) - x) ** 2) * w).sum() / count)
    return {"mse_smooth": mse(sm["x_smooth"]), "mse_impute": mse(imp["x_imputed"]), "mse_pred": mse(fr["x_pred"]),
            "regime_agreement": float((sm["regimes"] == dec["regimes"]).double().mean())}
