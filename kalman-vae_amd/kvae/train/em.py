"""Closed-form EM for the dynamics of a KVAE with switching dynamics (Murphy 1998, with GPB2 inference).

The generative switching model - (A_k, B_k, Q_k), the shared (C, R), the transition matrix P and (mu0, Sigma0) - is fitted to the
ENCODED sequences: the encoder, the decoder and the regime posterior network are read, never written.  One iteration is an E-step
per batch (KalmanFilter.em_statistics: one call of kvae_lgssm_switching_em on the GPU path, capturable into a hipGraph) whose
statistics are added over the batches (lgssm_ops.em_add), then ONE M-step (KalmanFilter.em_step with the added statistics), which
reads its skipped lists back to the host and is therefore not capturable.  No learning rate, no tau schedule."""
import torch

from kvae.kalman import lgssm_ops


@torch.no_grad()
def fit_dynamics_em(model, batches, iters, update=("A", "B", "Q", "C", "P"), sample_a=False, min_count=None):
    """Fit the switching dynamics of `model` (a KVAE with dynamics = "switching") by `iters` EM iterations over `batches`: a
    sequence (not a one-shot iterator) of x, (x, u), (x, u, mask) or dicts with those keys; u = None is zeros - B_k is then held,
    the data cannot tell it - and mask [B,T] has 1 = observed.  Every batch is encoded in eval mode: once, before the first
    iteration, with sample_a=False (a = the mean of q(a | x); the encoder is never written, so the encodings do not change), or
    anew in every iteration with sample_a=True (a ~ q(a | x): each iteration then fits other draws, and the returned values are
    not comparable from one iteration to the next).  update: which of "A", "B", "Q", "C", "R", "P", "mu0", "Sigma0" to
    re-estimate; min_count: KalmanFilter.em_step's.  Returns the history of sum_b log p(a_b | u_b) under GPB2, one float per
    iteration, each measured BEFORE that iteration's M-step."""
    kf = model.kalman_filter
    if not kf.dyn_params.is_switching_dynamics:
        raise ValueError('fit_dynamics_em needs a model with dynamics = "switching" (config.dynamics_model); this one has '
                         f'"{model.config.dynamics_model}"')
    batches = [_unpack(b) for b in batches]
    if not batches:
        raise ValueError("fit_dynamics_em: no batches")

    def encoded(x, u, mask):
        with model._readout("fit_dynamics_em", x, u, mask, sample=bool(sample_a)) as (a_vae, _, _, u_, mask_):
            return a_vae, u_, mask_

    fixed = None if sample_a else [encoded(*b) for b in batches]
    history = []
    for _ in range(int(iters)):
        total = None
        for i, batch in enumerate(batches):
            a_vae, u_, mask_ = encoded(*batch) if fixed is None else fixed[i]
            stats = kf.em_statistics(a_vae, u_, mask_, want=lgssm_ops._EM_STATS + ("log_lik_seq",))
            total = stats if total is None else lgssm_ops.em_add(total, stats)
        history.append(float(kf.em_step(None, None, update=update, stats=total, min_count=min_count)["log_lik"]))
    return history


def _unpack(batch):
    if isinstance(batch, dict):
        return batch["x"], batch.get("u"), batch.get("mask")
    if torch.is_tensor(batch):
        return batch, None, None
    batch = tuple(batch)
    return batch[0], (batch[1] if len(batch) > 1 else None), (batch[2] if len(batch) > 2 else None)
