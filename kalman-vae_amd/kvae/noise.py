"""Noise injection for parity testing.

The reference draws its randomness from torch's global generator in three places:
  * KVAE.reparameterize          eps_a  ~ N(0,1)  [B*T, a_dim]      (model.py:81-84)
  * KalmanFilter.elbo rsample    eps_z  ~ N(0,1)  [B,T,n]           (kalman_filter.py:351)
  * gumbel_softmax               gumbel ~ Gumbel  [B,T,K]           (switch_dyn_param.py:52,69)
Results on a GPU can only be compared with the CPU oracle if both consume the same draws, so the
drop-in classes look here first: inside `with inject(eps_a=..., eps_z=..., gumbel=...)` the given
tensors are used instead of fresh device-side draws.  Every draw site asks normal() / gumbel() below.

KVAE.generate (no counterpart in the reference) draws four more, all before its one rollout launch:
  * gen_z0      ~ N(0,1)  [B,S,n]     start state z_{T0-1} = mu + L_Sigma gen_z0
  * gen_z       ~ N(0,1)  [B,S,H,n]   process noise of each step
  * gen_a       ~ N(0,1)  [B,S,H,p]   emission noise of each step
  * gen_gumbel  ~ Gumbel  [B,S,H,K]   regime draws of the switching dynamics

KalmanFilter.sample_posterior / KVAE.sample_imputations (no counterpart either) draw two, before their two launches:
  * post_z      ~ N(0,1)  [B,S,T,n]   the draw of each step of each posterior path (z_t = ... + chol(P_t) post_z_t)
  * post_a      ~ N(0,1)  [B,S,T,p]   emission noise of each step (only with emission_noise=True)

KVAE.log_likelihood (no counterpart either) draws one, before the filter runs:
  * ll_a        ~ N(0,1)  [B,S,T,p]   the proposal draws a_s = a_mu + sqrt(a_var) ll_a_s (its regime draws take `gumbel`,
                                      one row per (b, s): [B*S,T,K])

KalmanFilter.particle_filter_regimes / KVAE.particle_filter_regimes (no counterpart either) draw two, before their launches:
  * pf_regime   ~ U[0,1)  [B,G,T,N]   the regime draw of every particle of every replicate at every step
  * pf_resample ~ U[0,1)  [B,G,T]     the offset of the systematic resampling of every replicate at every step
"""
import contextlib

import torch

_slots = {"eps_a": None, "eps_z": None, "gumbel": None, "gen_z0": None, "gen_z": None, "gen_a": None, "gen_gumbel": None,
          "post_z": None, "post_a": None, "ll_a": None, "pf_regime": None, "pf_resample": None}


def take(name):
    v = _slots.get(name)
    _slots[name] = None if v is None else v  # values stay for the whole context (re-usable)
    return v


def normal(slot, shape, device, dtype):
    """The tensor injected into `slot`, moved, cast and reshaped to `shape`; without one a fresh N(0,1) draw of that shape."""
    v = take(slot)
    return torch.randn(shape, device=device, dtype=dtype) if v is None else v.to(device=device, dtype=dtype).reshape(shape)


def gumbel(slot, shape, device, dtype):
    """As normal(), the fresh draw being standard Gumbel: -log(Exp(1))."""
    v = take(slot)
    if v is None:
        return -torch.empty(shape, device=device, dtype=dtype).exponential_().log()
    return v.to(device=device, dtype=dtype).reshape(shape)


def uniform(slot, shape, device, dtype):
    """As normal(), the fresh draw being uniform on [0, 1)."""
    v = take(slot)
    return torch.rand(shape, device=device, dtype=dtype) if v is None else v.to(device=device, dtype=dtype).reshape(shape)


@contextlib.contextmanager
def inject(eps_a=None, eps_z=None, gumbel=None, gen_z0=None, gen_z=None, gen_a=None, gen_gumbel=None, post_z=None, post_a=None,
           ll_a=None, pf_regime=None, pf_resample=None):
    old = dict(_slots)
    _slots.update(eps_a=eps_a, eps_z=eps_z, gumbel=gumbel, gen_z0=gen_z0, gen_z=gen_z, gen_a=gen_a, gen_gumbel=gen_gumbel,
                  post_z=post_z, post_a=post_a, ll_a=ll_a, pf_regime=pf_regime, pf_resample=pf_resample)
    try:
        yield
    finally:
        _slots.update(old)
