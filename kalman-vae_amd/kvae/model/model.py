"""KVAE — drop-in for kvae.model.model.KVAE of the reference (model.py:11-301 there).

Same constructor (`KVAE(config)`), sub-module names (encoder, decoder, kalman_filter[.dyn_params]),
parameter registration order and state_dict keys, same `forward` / `compute_loss` / `impute`
signatures and output dictionaries.  For the reference's default shapes every layer of the frame VAE runs on the
hand-written HIP kernels of csrc/vae_*.h (kvae/vae/fused.py; other shapes: MIOpen + fused epilogues), and everything
between `a_samples` and the LGSSM ELBO runs in the HIP kernels behind `self.kalman_filter`.
"""
import contextlib
import math
import os

import torch
from torch import nn

from kvae import _native
from kvae.kalman import dyn_param as base_dyn_param
from kvae.kalman import lgssm_ops, switch_dyn_param
from kvae.kalman.kalman_filter import KalmanFilter
from kvae.noise import gumbel as _gumbel, normal as _normal
from kvae.vae.losses import LinearScheduler, count_active_units, log_gaussian, vae_loss
from kvae.vae.vae import Decoder, Encoder


_FAST_PATH_NOTES = {
    "lgssm_specialised": "(z,u,a) is neither (4,4,2) nor (16,16,2): the LGSSM runs the run-time-dimension kernels",
    "lstm_registers": "alpha-net shape is not (hidden 50, a_dim 2): the LSTM runs the run-time-shape kernel",
    "bigru_registers": "regime posterior shape is not (hidden 50, a_dim 2): the bi-GRU runs on nn.GRU (MIOpen), "
                       "which cannot be captured into a hipGraph",
    "vae_default_shapes": "frame VAE is not the reference's default (32x32x1, channels [32,32,32], a_dim 2): "
                          "convolutions run on MIOpen with fused epilogues",
}


class _SideGradJoin(torch.autograd.Function):
    """Identity on a_samples for the frame branch; its backward adds the gradient the LGSSM branch has already produced on the
    side stream (`early_kf_backward`), after making the current stream wait for that stream."""

    @staticmethod
    def forward(ctx, a, holder):
        ctx.holder = holder
        return a.view_as(a)

    @staticmethod
    def backward(ctx, g):
        h = ctx.holder
        torch.cuda.current_stream().wait_stream(h["side"])
        ga = h["a_side"].grad
        if ga is None:   # the frame branch is being differentiated but nobody ran the LGSSM branch's backward
            raise RuntimeError("KVAE.early_kf_backward is on but the LGSSM branch has no gradient yet: call "
                               "compute_loss() (which runs that branch's backward) before loss.backward(), or clear the flag")
        return g + ga, None


# A/B switch for the scalar head of the objective, read ONCE (None: chosen per call from the step's schedule):
# 2 = frame terms through the fused head, 1 = LGSSM term too, 0 = torch's element-wise ops.
_LOSS_HEAD = os.environ.get("KVAE_LOSS_HEAD")


class KVAE(nn.Module):
    # Training-step schedule (addition over the reference; set by kvae.train.Trainer): the gradient of the LGSSM term w.r.t. the
    # encodings and the dynamics parameters does not depend on the frame terms, so compute_loss() can run that branch's backward
    # on the side stream right behind its forward; loss.backward() then only walks the frame branch and picks the result up.
    # The Trainer sets these three for the duration of its own forward+backward only (Trainer._schedule) and restores them:
    # a training-mode forward / compute_loss / backward outside a Trainer always takes the plain single-backward route.
    early_kf_backward = False
    lgssm_stream = None     # second HIP stream for the LGSSM chain: it is latency-bound (256 of ~8000 wave slots at configs[1])
    #                         and independent of the decoder, so it overlaps with the decoder convolutions; compute_loss() joins
    # The LGSSM term of the objective: "elbo" = the reference's one-sample ELBO (z_t drawn from the smoothing marginals), "marginal"
    # = the exact log p(a | u) of the prediction-error decomposition (KalmanFilter.marginal: zero variance, no RTS sweep, no eps_z).
    # With "marginal" a TRAINING-mode forward runs the filter only: outputs["mus_smooth"] / ["Sigmas_smooth"] are None.
    # "regime_marginal" (switching dynamics) = log p(a | u) with the regimes summed out under GPB2 (KalmanFilter.regime_marginal): the
    # regime posterior network plays no part; a TRAINING-mode forward runs neither it nor the filter, every LGSSM output is None.
    kf_objective = "elbo"
    kf_value_only = False   # "vae" phase (reference train.py:246-250: kf_weight = 0, every LGSSM parameter frozen): the chain runs
    #                         forward only, without a tape, for the logged elbo_kf; nothing of it is differentiated

    def __init__(self, config):
        super().__init__()
        if hasattr(config, "validate"):
            config.validate()   # dimension limits of the HIP kernels (n, m, p, K <= 16) fail here, not at the first launch
            slow = [k for k, v in config.fast_path().items() if not v and k in _FAST_PATH_NOTES]
            if slow:   # shapes outside the hand-specialised kernels still run, on generic kernels / MIOpen: say so once
                import warnings
                warnings.warn("KVAE: " + "; ".join(_FAST_PATH_NOTES[k] for k in slow), stacklevel=2)
        self.config = config
        self.encoder = Encoder(config)
        self.decoder = Decoder(config)
        self.scheduler = LinearScheduler(config)
        self.beta = self.scheduler.get_beta(0) if config.scheduled_beta else 1.0
        self.K, self.z_dim, self.a_dim, self.u_dim = config.num_modes, config.z_dim, config.a_dim, config.u_dim

        # LGSSM initialisation: A_k = I, B_k, C_k ~ N(0, init_kf_matrices^2)  (reference model.py:33-45)
        A0 = torch.eye(self.z_dim).repeat(self.K, 1, 1)
        B0 = torch.randn(self.K, self.z_dim, self.u_dim) * config.init_kf_matrices
        C0 = torch.randn(self.K, self.a_dim, self.z_dim) * config.init_kf_matrices
        kind = config.dynamics_model.lower()
        if kind == "switching":
            prior = switch_dyn_param.StickyRegimePrior(self.K, p_stay=config.sticky_p_stay)
            posterior = switch_dyn_param.MarkovVariationalRegimePosterior(
                self.K, input_dim=self.a_dim, hidden_size=config.dynamics_hidden_dim)
            Q0 = torch.eye(self.z_dim).repeat(self.K, 1, 1) * config.noise_transition
            dynamics = switch_dyn_param.SwitchingDynamicsParameter(
                A0, B0, C0, Q=Q0, prior=prior, hidden_lstm=config.dynamics_hidden_dim,
                markov_regime_posterior=posterior)
            dynamics.tau = config.tau_init
        elif kind == "lstm":
            dynamics = base_dyn_param.DynamicsParameter(A0, B0, C0, hidden_lstm=config.dynamics_hidden_dim)
        else:
            raise ValueError(f"Unknown dynamics model: {config.dynamics_model}")
        # config noise values are variances
        self.kalman_filter = KalmanFilter(config.noise_transition ** 0.5, config.noise_emission ** 0.5,
                                          torch.zeros(self.z_dim), torch.eye(self.z_dim) * config.init_cov, dynamics)

    # -- VAE halves -----------------------------------------------------------------------------
    def reparameterize(self, mu, var):
        std = torch.sqrt(var + 1e-6)
        return mu + _normal("eps_a", std.shape, std.device, std.dtype) * std

    def encode_sequence(self, x, sample=True):
        """`sample=False`: a = a_mu (the heads kernel with eps = 0, no draw taken)."""
        lead = x.shape[:2]
        feat = self.encoder.features(x.flatten(0, 1))
        shape = (feat.shape[0], self.config.a_dim)
        eps = (_normal("eps_a", shape, feat.device, feat.dtype) if sample
               else torch.zeros(shape, device=feat.device, dtype=feat.dtype))
        a, mu, var = self.encoder.heads(feat, eps)   # both heads + reparameterisation: one kernel on the GPU path
        return a.unflatten(0, lead), mu.unflatten(0, lead), var.unflatten(0, lead)

    def decode_sequence(self, a):
        return self.decoder(a.flatten(0, 1)).unflatten(0, a.shape[:2])

    def _kf_objective(self, value=None):
        value = self.kf_objective if value is None else value
        if value not in ("elbo", "marginal", "regime_marginal"):
            raise ValueError(f"kf_objective must be 'elbo', 'marginal' or 'regime_marginal', got {value!r}")
        if value == "regime_marginal" and not self.kalman_filter.dyn_params.is_switching_dynamics:
            raise ValueError("kf_objective 'regime_marginal' needs switching dynamics: the lstm dynamics have no regimes to sum out")
        return value

    def _to_pixels(self, logits):
        return torch.sigmoid(logits) if self.config.out_distr.lower() == "bernoulli" else logits

    def _zero_u(self, like):
        return torch.zeros(like.shape[0], like.shape[1], self.u_dim, device=like.device, dtype=like.dtype)

    # -- what the eval-mode read-outs share ------------------------------------------------------
    def _check_mask_u(self, who, x, mask, u, required=False, horizon=0):
        """mask [B,T] (`required`: None is an error too) and u [B,T,m] - [B,T0+H,m] with a `horizon` - or None."""
        Bsz, T = x.shape[:2]
        if (required and mask is None) or (mask is not None and tuple(mask.shape) != (Bsz, T)):
            raise ValueError(f"{who}: mask must be [B, T] = [{Bsz}, {T}], got {None if mask is None else list(mask.shape)}")
        steps, name = (T + horizon, "T0+H") if horizon else (T, "T")
        if u is not None and (u.dim() != 3 or u.shape[0] != Bsz or u.shape[1] != steps or u.shape[2] != self.u_dim):
            raise ValueError(f"{who}: u must be [B, {name}, m] = [{Bsz}, {steps}, {self.u_dim}], got {list(u.shape)}")

    def _readout(self, who, x, u, mask, sample=True, **check):
        """Prelude of a read-out: `with self._readout(...) as (a_vae, a_mu, a_var, u, mask)`.  mask and u are checked HERE, at
        the call (_check_mask_u); entering the block puts the model in eval mode - whatever way the block is left restores the
        mode it was in - and encodes x (sample=False: a_vae = a_mu, no draw taken); u (zeros for None) and mask (None stays
        None) come back on the encodings' device and dtype.  No host synchronisation."""
        self._check_mask_u(who, x, mask, u, **check)

        @contextlib.contextmanager
        def block():
            was_training = self.training
            self.eval()
            try:
                a_vae, a_mu, a_var = self.encode_sequence(x, sample=sample)
                dev, dt = a_vae.device, a_vae.dtype
                yield (a_vae, a_mu, a_var, self._zero_u(a_vae) if u is None else u.to(device=dev, dtype=dt),
                       None if mask is None else mask.to(device=dev, dtype=dt))
            finally:
                self.train(was_training)
        return block()

    def _needs_switching(self, who):
        if not self.kalman_filter.dyn_params.is_switching_dynamics:
            raise ValueError(f'{who} needs a model with dynamics = "switching" (config.dynamics_model); this one has '
                             f'"{self.config.dynamics_model}"')

    def _switching_readout(self, who, x, u, mask, sample_a):
        """Prelude of a read-out of the switching model: the dynamics are checked first, then _readout's mask and u."""
        self._needs_switching(who)
        return self._readout(who, x, u, mask, sample=bool(sample_a))

    def _close_readout(self, out, a_vae, mask, decode, key, latents):
        """What the read-outs of the generative switching model close with: a_vae, n_obs [B] and - `decode` - out[key] = the
        decoder's frames of `latents`."""
        out["a_vae"] = a_vae
        out["n_obs"] = self._n_obs(mask, a_vae)
        if decode:
            out[key] = self._decode_latents(latents, a_vae.dtype)
        return out

    @staticmethod
    def _argmax_lowest(p):
        """argmax over the last axis, the lowest index among the maxima."""
        return (p == p.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)

    @staticmethod
    def _n_obs(mask, a):
        """Observed steps per sequence [B] of latents a [B,T,p] under mask [B,T] or None, on the device."""
        return torch.full((a.shape[0],), float(a.shape[1]), device=a.device, dtype=a.dtype) if mask is None else mask.sum(1)

    def _decode_latents(self, a, dtype):
        """Pixels [B, ..., C, h, w] of latents a [B, ..., p]: one decoder pass over all of them."""
        x = self._to_pixels(self.decode_sequence(a.reshape(a.shape[0], -1, a.shape[-1]).to(dtype)))
        return x.unflatten(1, a.shape[1:-1])

    # -- full pass ------------------------------------------------------------------------------
    def forward(self, x, u=None, mask=None, with_recon=True):
        """`with_recon=False` (addition over the reference) skips sigmoid(x_logits): the training loss only
        needs the logits, so the step saves one full pass over the frame tensor.
        With switching dynamics `state_probs` is a single draw of the regime chain (one-hot in eval mode), not
        probabilities: decode_regimes() gives the marginals and the most likely path."""
        a_samples, a_mu, a_var = self.encode_sequence(x)
        if u is None:
            u = self._zero_u(x)
        self.kalman_filter.dyn_params.reset_state()
        side = self.lgssm_stream if (self.training and a_samples.is_cuda) else None
        a_side = None
        value_only = self.kf_value_only and self.training
        kf = self.kalman_filter
        objective = self._kf_objective()
        if objective == "regime_marginal" and self.training:   # compute_loss sums the regimes out over a_samples: nothing to run here
            run = lambda y, uu, mask=None: (None,) * 9
        elif objective == "marginal" and self.training:   # the exact objective reads the one-step-ahead beliefs only
            run = lambda y, uu, mask=None: (None, None) + kf.filter(y, uu, mask=mask)
        else:
            run = kf.smooth
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
            a_lgssm = a_samples.detach() if value_only else a_samples
            if self.early_kf_backward and not value_only and torch.is_grad_enabled() and a_samples.requires_grad:
                a_side = a_lgssm = a_samples.detach().requires_grad_(True)
                a_samples = _SideGradJoin.apply(a_samples, {"a_side": a_side, "side": side})
            with torch.cuda.stream(side), torch.set_grad_enabled(torch.is_grad_enabled() and not value_only):
                smoothed = run(a_lgssm, u, mask=mask)
        elif value_only:
            with torch.no_grad():
                smoothed = run(a_samples.detach(), u, mask=mask)
        else:
            smoothed = run(a_samples, u, mask=mask)
        (mus_smooth, Sigmas_smooth, mus_filt, Sigmas_filt, mus_pred, Sigmas_pred, A_list, B_list, C_list) = smoothed
        # the decoder sees its own target frames: the head's kernels also give sigmoid(x_logits) and the per-frame Bernoulli term
        # (fused.DecoderHeadBernoulli), or None for both where they do not apply
        lead = a_samples.shape[:2]
        x_logits, x_recon, frame_ll = self.decoder.forward_with_frames(a_samples.flatten(0, 1), x.flatten(0, 1), with_recon)
        x_logits = x_logits.unflatten(0, lead)
        if frame_ll is not None:
            frame_ll = frame_ll.unflatten(0, lead)
            x_recon = x_recon.unflatten(0, lead) if with_recon else None
        else:
            x_recon = self._to_pixels(x_logits) if with_recon else None
        return {
            "x_recon": x_recon, "x_logits": x_logits, "frame_ll": frame_ll, "frame_ll_x": x if frame_ll is not None else None,
            "a_samples": a_samples, "a_mu": a_mu, "a_var": a_var, "a_side": a_side,
            "mus_smooth": mus_smooth, "Sigmas_smooth": Sigmas_smooth,
            "mus_filt": mus_filt, "Sigmas_filt": Sigmas_filt,
            "mus_pred": mus_pred, "Sigmas_pred": Sigmas_pred,
            "ABC": (A_list, B_list, C_list), "u": u,
            "state_probs": self.kalman_filter.dyn_params.state_seq,
        }

    def compute_loss(self, x, outputs, kf_weight=1.0, vae_weight=1.0, mask=None, with_metrics=True, weights_dev=None,
                     kf_objective=None):
        """`with_metrics` (addition over the reference): True = the reference's behaviour (active-unit count and the
        two latent variances as Python numbers: three host syncs); "device" = the same statistics as device tensors
        (`active_units`, `latent_variances`), no sync, capturable into a hipGraph; False = skip them.
        `weights_dev` (addition): fp32 device tensor (vae_weight, kf_weight) that replaces the two floats - the kernels read it
        at run time, so a step captured into a hipGraph follows the reference's phase weights (train.py:246-260).
        `kf_objective` (addition): None = self.kf_objective; "elbo" = the reference's one-sample ELBO; "marginal" = elbo_kf is the
        exact (seq_ll.sum() [+ switching: log_p.sum() - log_q.sum()]) / num_el over outputs["mus_pred"], ["Sigmas_pred"], ["ABC"] and
        a_samples (KalmanFilter.marginal), num_el as in KalmanFilter.elbo; "regime_marginal" (switching dynamics) = elbo_kf is
        seq_ll.sum() / num_el of KalmanFilter.regime_log_marginal over a_samples and u: the regimes summed out, no regime-chain term."""
        objective = self._kf_objective(kf_objective)
        if weights_dev is not None:
            vae_weight, kf_weight = weights_dev[0], weights_dev[1]
        B, T = x.shape[:2]
        a, a_mu, a_var = outputs["a_samples"], outputs["a_mu"], outputs["a_var"]
        A_list, B_list, C_list = outputs["ABC"]
        u = outputs.get("u")
        if u is None:
            u = self._zero_u(x)
        x_mu = outputs["x_logits"] if outputs.get("x_logits") is not None else outputs["x_recon"]
        side = self.lgssm_stream if (self.training and a.is_cuda) else None

        a_side = outputs.get("a_side")
        stats = None
        if with_metrics == "device":   # before the LGSSM term is awaited: the main stream has this to do while the side stream finishes
            variances = a_mu.detach().reshape(-1, a_mu.shape[-1]).var(dim=0)
            stats = ((variances > 1e-2).sum(), variances)

        def kf_term(a_in):
            if objective == "regime_marginal":
                return self.kalman_filter.regime_marginal(a_in, u, mask=mask)
            if objective == "marginal":
                return self.kalman_filter.marginal(outputs["mus_pred"], outputs["Sigmas_pred"], a_in, C_list, mask=mask)
            return self.kalman_filter.elbo(outputs["mus_smooth"], outputs["Sigmas_smooth"], a_in, u, A_list, B_list, C_list, mask=mask)

        def kf_elbo():
            if self.kf_value_only and self.training:   # no tape, nothing to differentiate: the value for the log
                with torch.no_grad():
                    if side is None:
                        return kf_term(a.detach())
                    with torch.cuda.stream(side):
                        v = kf_term(a.detach())
                    torch.cuda.current_stream().wait_stream(side)
                    return v
            if a_side is not None:   # early_kf_backward: value and gradients of the LGSSM term on the side stream, now
                with torch.cuda.stream(side):
                    v = kf_term(a_side)
                    done = torch.cuda.Event()
                    done.record(side)
                    # d loss / d elbo_kf = -kf_weight
                    v.backward((-kf_weight).reshape(v.shape) if torch.is_tensor(kf_weight) else torch.full_like(v, -float(kf_weight)))
                torch.cuda.current_stream().wait_event(done)   # the value only; _SideGradJoin waits for the gradients
                return v.detach()
            if side is None:
                return kf_term(a)
            with torch.cuda.stream(side):
                v = kf_term(a)
            torch.cuda.current_stream().wait_stream(side)   # join before the two ELBOs are combined
            return v

        head = _LOSS_HEAD
        if head is None and (a_side is not None or (self.kf_value_only and self.training and side is not None)):
            head = "2"
        if ((head in ("1", "2") or (head is None and side is None)) and self.config.out_distr.lower() == "bernoulli"
                and _native.fused_ok(x_mu) and x_mu.dtype == torch.float32
                and x.dtype == torch.float32 and a.dtype == torch.float32 and not x.requires_grad):
            # The two per-frame terms are one kernel each and the whole scalar head of the objective (masking, sums,
            # normalisation, beta / scale / weights, sign) is ONE launch each way (csrc/vae_heads.h) instead of ~40 dependent
            # element-wise launches.  With the LGSSM chain on a side stream and ONE backward, the ~40 launches were what gave
            # that chain's backward its head start over the decoder's Winograd kernels (which leave no registers for a
            # second kernel on their CUs): the fused head made the replayed graph slower.  With
            # early_kf_backward the side chain no longer needs that head start and the frame terms take the fused head ("2").
            from kvae.vae.fused import BernoulliFrameLogLik, LatentReg, LossHead
            # log p(x_t | a_t) came with the decoder's forward if these are the very frames it decoded against
            lpx = outputs["frame_ll"] if outputs.get("frame_ll") is not None and outputs.get("frame_ll_x") is x \
                else BernoulliFrameLogLik.apply(x_mu, x)
            regf = LatentReg.apply(a, a_mu, a_var)
            mk = None if mask is None else mask.to(device=x.device, dtype=torch.float32).reshape(B, T)
            if head == "2":
                # frame terms only through the fused head (main stream, before the join); the LGSSM term joins with torch ops, so
                # its gradient reaches the side stream without waiting for the head's backward
                z = getattr(self, "_zero_kf", None)
                if z is None or z.device != x.device:
                    z = self._zero_kf = torch.zeros(1, device=x.device, dtype=torch.float32)
                wd = weights_dev   # its kf_weight multiplies the zero standing in for the LGSSM term here
                vae_loss_w, _, _, vae_elbo, recon, reg = LossHead.apply(
                    lpx, regf, z, mk, self.beta, self.config.scale_reconstruction, 0.0 if wd is not None else vae_weight, 0.0, wd)
                elbo_kf = kf_elbo()
                loss = vae_loss_w - kf_weight * elbo_kf
                out = {"loss": loss, "elbo_total": -loss.detach(), "elbo_kf": elbo_kf, "elbo_vae_total": vae_elbo,
                       "recon": recon, "kl": reg}
            else:
                elbo_kf = kf_elbo()
                loss, elbo_total, elbo_kf_v, vae_elbo, recon, reg = LossHead.apply(
                    lpx, regf, elbo_kf, mk, self.beta, self.config.scale_reconstruction,
                    0.0 if weights_dev is not None else vae_weight, 0.0 if weights_dev is not None else kf_weight, weights_dev)
                out = {"loss": loss, "elbo_total": elbo_total, "elbo_kf": elbo_kf_v, "elbo_vae_total": vae_elbo,
                       "recon": recon, "kl": reg}
        else:
            x_var = torch.tensor(self.config.noise_pixel_var, device=x.device, dtype=x_mu.dtype) \
                if self.config.out_distr.lower() != "bernoulli" else None
            vae_elbo, recon, reg = vae_loss(x, x_mu, x_var, a, a_mu, a_var,
                                            scale_reconstruction=self.config.scale_reconstruction, mask=mask,
                                            out_distr=self.config.out_distr, beta=self.beta)
            elbo_kf = kf_elbo()
            elbo_total = vae_weight * vae_elbo + kf_weight * elbo_kf
            out = {"loss": -elbo_total, "elbo_total": elbo_total, "elbo_kf": elbo_kf, "elbo_vae_total": vae_elbo,
                   "recon": recon, "kl": reg}
        if with_metrics == "device":
            out.update(active_units=stats[0], latent_variances=stats[1])
        elif with_metrics:
            active, variances = count_active_units(a_mu)
            out.update(active_units=active, latent_var_0=variances[0].item(), latent_var_1=variances[1].item())
        return out

    @torch.no_grad()
    def impute(self, x, mask, u=None):
        """Eval-mode imputation: decode C_t mu_{t|T} (smoothed) and C_t mu_{t|t} (filtered).
        With switching dynamics `state_probs` is a single draw of the regime chain (a hard one-hot sequence), not
        probabilities: decode_regimes() gives the marginals and the most likely path."""
        self.eval()
        mask = mask.to(device=x.device, dtype=x.dtype)
        out = self.forward(x, u=u, mask=mask)
        _, _, C_list = out["ABC"]
        a_imputed, a_filtered = self.kalman_filter.emission_means(out["mus_smooth"], out["mus_filt"], C_list)
        # The reference decodes a_vae again (forward already did: the same pixels) and then the two read-outs one after the other
        # (model.py:275-290 there).  Frames are independent: forward's reconstruction is returned as it is, and ONE decoder pass
        # over the concatenated read-outs gives the other two - two decoder passes in all instead of four.
        x2 = self._to_pixels(self.decode_sequence(torch.cat([a_imputed, a_filtered], 0)))
        x_imputed, x_filtered = x2.chunk(2, 0)
        return {"x_recon": out["x_recon"], "x_imputed": x_imputed, "x_filtered": x_filtered,
                "a_vae": out["a_samples"], "a_imputed": a_imputed, "a_filtered": a_filtered,
                "state_probs": out["state_probs"]}

    @torch.no_grad()
    def sample_imputations(self, x, mask, num_samples=1, u=None, noise=True, emission_noise=False, decode=True):
        """Sampled completions of hidden frames: `num_samples` COHERENT latent paths per sequence from the smoothing posterior
        p(z_{0:T-1} | a_{0:T-1}, u), decoded (no counterpart in the reference; impute() decodes their mean, C_t mu_{t|T}).
        B sequences of T frames, S = num_samples, mask [B,T] (1 = observed).

        1. Encode x (as forward does) and run the eval-mode filter with the mask: mu_{t|t}, Sigma_{t|t}, mu_{t|t-1}, Sigma_{t|t-1},
           A_t, C_t (and Q_t of the switching model).  The dynamics depend on the observations only, so given this pass the model
           is linear-Gaussian and backward sampling is exact.  With switching dynamics the pass holds ONE draw of the regime
           sequence (hard one-hot in eval mode), as impute()'s does: the S paths share it.
        2. z_{T-1} = mu_{T-1|T-1} + chol(Sigma_{T-1|T-1}) eps_{T-1}; for t = T-2 .. 0
               J_t = Sigma_{t|t} A_{t+1}^T Sigma_{t+1|t}^{-1}
               P_t = (I - J_t A_{t+1}) Sigma_{t|t} (I - J_t A_{t+1})^T + J_t Q_{t+1} J_t^T      (symmetrised)
               z_t = mu_{t|t} + J_t (z_{t+1} - mu_{t+1|t}) + chol(P_t) eps_t
           with chol the reference's _safe_cholesky ladder applied per (b, t).  a_t = C_t z_t (+ chol(R) eta_t with
           emission_noise).  noise=False: z_t = mu_{t|T} and a_t = impute()'s a_imputed on every path.
        3. x = decoder(a) through the frame VAE, one pass over the B*S*T frames.

        Draws are made here with torch before the two launches (kvae.noise.inject: post_z, post_a).  u: [B,T,m] or None (zeros).
        Returns x [B,S,T,C,h,w] (None with decode=False), a [B,S,T,p], z [B,S,T,n], a_vae [B,T,p], state_probs (and levels
        [B,T], the ladder level of each chol(P_t)).  Training mode and parameters are left as they were."""
        num_samples = int(num_samples)
        if num_samples < 1:
            raise ValueError(f"sample_imputations: num_samples must be >= 1, got {num_samples}")
        with self._readout("sample_imputations", x, u, mask, required=True) as (a_vae, _, _, u, mask):
            self.kalman_filter.dyn_params.reset_state()
            post = self.kalman_filter.sample_posterior(a_vae, u, mask, num_samples, noise=noise, emission_noise=emission_noise)
            return {"x": self._decode_latents(post["a"], a_vae.dtype) if decode else None, "a": post["a"], "z": post["z"],
                    "a_vae": a_vae, "state_probs": post["state_probs"], "levels": post["levels"]}

    @torch.no_grad()
    def decode_regimes(self, x, u=None, mask=None, sample_a=False, smooth=True, decode=False):
        """Segment each sequence into regimes, exactly (switching dynamics only; no counterpart in the reference, whose
        plot_state_probabilities is fed single Gumbel draws).  The regime posterior is a Markov chain, q(s_0) = softmax(init),
        q(s_t | s_{t-1}) = row-softmax(logits[t]) with the evidence already folded into the logits by the bi-GRU, so its
        marginals, its most likely path and its KL against the sticky prior are one forward sweep (kvae_regime_decode).

        1. Encode x.  sample_a=False: a = a_mu, the call is deterministic; True: a is drawn as forward() draws it.
        2. regime_probs [B,T,K] = q(s_t); regimes [B,T] (int64) = argmax over paths of log q(s_{0:T-1}) (Viterbi, lowest index
           on ties); regimes_logq [B] = its log q; regime_kl [B,T], summing to KL(q || p), the quantity the ELBO estimates from
           one sample.
        3. smooth=True: the eval-mode smoother with A_t, B_t, Q_t of the most likely path (mask [B,T] optional, 1 = observed;
           u [B,T,m] or None = zeros): mus_smooth, Sigmas_smooth, mus_filt, ABC and a_imputed = C_t mu_{t|T}.
        4. decode=True (needs smooth): x_imputed = decoder(a_imputed).
        Also returns a_vae.  Training mode, tau and parameters are left as they were."""
        dyn = self.kalman_filter.dyn_params
        prelude = self._switching_readout("decode_regimes", x, u, mask, sample_a)   # its shape checks come before this one
        if decode and not smooth:
            raise ValueError("decode_regimes: decode=True needs smooth=True (x_imputed is decoded from the smoothed latents)")
        with prelude as (a_vae, _, _, u, mask):
            dyn.reset_state()
            out = dict(dyn.decode(a_vae), a_vae=a_vae)
            if smooth:
                y_map = torch.nn.functional.one_hot(out["regimes"], self.K).to(a_vae.dtype)
                with dyn.pinned(y_map):
                    sm = self.kalman_filter.smooth(a_vae, u, mask=mask)
                ms, Ss, mf, _, _, _, A_list, B_list, C_list = sm
                a_imputed, _ = self.kalman_filter.emission_means(ms, mf, C_list)
                out.update(mus_smooth=ms, Sigmas_smooth=Ss, mus_filt=mf, ABC=(A_list, B_list, C_list), a_imputed=a_imputed)
                if decode:
                    out["x_imputed"] = self._to_pixels(self.decode_sequence(a_imputed))
            return out

    @torch.no_grad()
    def score(self, x, u=None, mask=None, sample_a=False, regimes="map", decode=False):
        """How probable the encoded sequence is under the learned dynamics, exactly (no counterpart in the reference, whose only
        likelihood-like number is the one-sample training ELBO): the prediction-error decomposition of the linear-Gaussian
        state-space model over the eval-mode filter's own outputs (kvae_lgssm_predictive).

        1. Encode x.  sample_a=False: a = a_mu, the call is deterministic; True: a is drawn as forward() draws it.
        2. Dynamics.  lstm: the alpha-network, as the filter runs it (`regimes` is ignored).  switching, regimes="map": the most
           likely regime path (decode_regimes' Viterbi path) is pinned and the density is conditional on it - the result carries
           `regimes` [B,T] and `regimes_logq` [B]; regimes="draw": one eval-mode draw of the regime chain.
        3. For every step: a_pred_t = C_t mu_{t|t-1}, S_t = sym(C_t Sigma_{t|t-1} C_t^T + R), nis_t = r_t^T S_t^{-1} r_t with
           r_t = a_t - a_pred_t, log_lik_t = -0.5 (nis_t + log det S_t + p log 2 pi) = log p(a_t | a_{0:t-1}, u); log_lik_seq =
           sum_t mask_t log_lik_t = log p(observed a).  mask [B,T] optional (1 = observed): hidden steps have log_lik = nis = 0,
           a_pred and S are still the model's forecast of the hidden frame.  u [B,T,m] or None = zeros.
        4. decode=True: x_pred = decoder(a_pred), the one-step-ahead predicted frames.
        Returns log_lik [B,T], log_lik_seq [B], nis [B,T], a_pred [B,T,p], S [B,T,p,p], levels [B,T] (ladder level of each
        chol(S_t)), a_vae, state_probs, n_obs [B].  No host synchronisation: the call can be captured into a hipGraph.
        Training mode, tau and parameters are left as they were."""
        if regimes not in ("map", "draw"):
            raise ValueError(f'score: regimes must be "map" or "draw", got {regimes!r}')
        dyn = self.kalman_filter.dyn_params
        with self._readout("score", x, u, mask, sample=bool(sample_a)) as (a_vae, _, _, u, mask):
            dyn.reset_state()
            out = {}
            if dyn.is_switching_dynamics and regimes == "map":
                dec = dyn.decode(a_vae)
                with dyn.pinned(torch.nn.functional.one_hot(dec["regimes"], self.K).to(a_vae.dtype)):
                    pred = self.kalman_filter.predictive(a_vae, u, mask)
                out.update(regimes=dec["regimes"], regimes_logq=dec["regimes_logq"])
            else:
                pred = self.kalman_filter.predictive(a_vae, u, mask)
            out.update(log_lik=pred["ll"], log_lik_seq=pred["seq_ll"], nis=pred["nis"], a_pred=pred["a_pred"], S=pred["S"],
                       levels=pred["levels"], a_vae=a_vae, state_probs=pred["state_probs"], n_obs=self._n_obs(mask, a_vae))
            if decode:
                out["x_pred"] = self._decode_latents(pred["a_pred"], a_vae.dtype)
            return out

    @torch.no_grad()
    def filter_regimes(self, x, u=None, mask=None, sample_a=False, state=None, decode=False):
        """What the generative switching model believes on its own, causally (switching dynamics only; no counterpart in the
        reference): the switching Kalman filter with second-order generalised pseudo-Bayes collapse (GPB2) over A_k, B_k, Q_k,
        the shared C and R, the sticky prior P (unclamped) and (mu0, Sigma0) - kvae_lgssm_switching_filter.  The bidirectional
        regime posterior network, which reads the whole sequence, plays no part: every output of step t has seen a_{0:t} only.

        1. Encode x.  sample_a=False: a = a_mu, the call is deterministic; True: a is drawn as forward() draws it.
        2. regime_filt [B,T,K] = p(s_t | a_{0:t}), regime_pred [B,T,K] = p(s_t | a_{0:t-1}), regimes [B,T] (int64) = argmax of
           regime_filt (lowest index on ties).
        3. log_lik [B,T] = log p(a_t | a_{0:t-1}, u) with the regimes summed out (0 on hidden steps; mask [B,T] optional,
           1 = observed), log_lik_seq [B] its sum; a_pred [B,T,p], S [B,T,p,p] the moment-matched one-step-ahead forecast;
           mus_filt [B,T,n], Sigmas_filt [B,T,n,n] the moment-matched filtered belief; levels [B,T] the largest ladder level of
           the pair densities.  u [B,T,m] or None = zeros.
        4. state: the K collapsed Gaussians and their log weights after the last step; state=prev["state"] continues a stream,
           and the outputs of the chunks, concatenated, are the bits of the whole-sequence call.
        5. decode=True: x_pred = decoder(a_pred), the one-step-ahead predicted frames.
        Also returns a_vae and n_obs [B].  Exact through t = 1, at every step when P is the identity or when all regimes share
        A, B, Q; otherwise the GPB2 approximation.  No host synchronisation.  Training mode, tau and
        parameters are left as they were."""
        with self._switching_readout("filter_regimes", x, u, mask, sample_a) as (a_vae, _, _, u, mask):
            out = self.kalman_filter.filter_regimes(a_vae, u, mask, state=state)
            out["regimes"] = self._argmax_lowest(out["regime_filt"])
            return self._close_readout(out, a_vae, mask, decode, "x_pred", out["a_pred"])

    @torch.no_grad()
    def particle_filter_regimes(self, x, u=None, mask=None, num_particles=256, replicates=1, ess_threshold=0.5, sample_a=False,
                                state=None, decode=False):
        """filter_regimes without its GPB2 approximation (switching dynamics only; no counterpart in the reference): a
        Rao-Blackwellised particle filter over the same generative switching model - `replicates` (G) independent filters of
        `num_particles` (N) particles per sequence, every particle a regime history with an exact Kalman belief -
        kvae_lgssm_switching_pf.  It is the yardstick of the GPB2 read-outs, and its lineages are joint samples of regime paths.

        1. Encode x, as filter_regimes does.  u [B,T,m] or None = zeros; mask [B,T] optional (1 = observed).
        2. Per replicate: log_lik [B,G,T] (0 on hidden steps), log_lik_seq [B,G] - exp of it is an UNBIASED estimate of
           p(a | u) for any N -, regime_filt [B,G,T,K] (consistent in N), mus_filt [B,G,T,n], Sigmas_filt [B,G,T,n,n], ess
           [B,G,T], resampled [B,G,T] (bool), regimes / ancestors [B,G,T,N] (int32), levels [B,G,T], paths [B,G,N,T] (int32: the
           regime lineage of every final slot) with path_log_w [B,G,N], state.
        3. Combined: log_lik_seq_mean [B] = the logmeanexp of log_lik_seq over the replicates (still unbiased); regime_filt_mean
           [B,T,K] = the replicate average of regime_filt weighted by exp(cumulative log_lik) (the plain average is biased);
           regimes_map [B,T] (int64) = its argmax (lowest index on ties); a_filt [B,T,p] = C mus_filt under the same weights.
        4. ess_threshold in [0,1]: 0 never resamples, 1 resamples at every step, else when ess_t < ess_threshold N.  N in
           {64, 128, 256} runs the HIP kernel, anything else its restatement in torch ops.
        5. state=prev["state"] continues a stream; with injected draws (kvae.noise pf_regime / pf_resample) the chunks give the
           bits of the whole-sequence call.  decode=True: x_filt = decoder(a_filt).
        Also returns a_vae and n_obs [B].  No host synchronisation.  Training mode, tau and parameters are left as they were."""
        dyn = self.kalman_filter.dyn_params
        with self._switching_readout("particle_filter_regimes", x, u, mask, sample_a) as (a_vae, _, _, u, mask):
            out = self.kalman_filter.particle_filter_regimes(a_vae, u, mask, num_particles=num_particles, replicates=replicates,
                                                             ess_threshold=ess_threshold, state=state)
            out["log_lik_seq_mean"], w = lgssm_ops.combine_replicates(out["log_lik"])
            rf = (w.unsqueeze(-1) * out["regime_filt"]).sum(1)
            out["regime_filt_mean"] = rf
            out["regimes_map"] = self._argmax_lowest(rf)
            out["a_filt"] = (w.unsqueeze(-1) * out["mus_filt"]).sum(1) @ dyn.C[0].detach().to(rf.dtype).mT
            return self._close_readout(out, a_vae, mask, decode, "x_filt", out["a_filt"])

    @torch.no_grad()
    def smooth_regimes(self, x, u=None, mask=None, sample_a=False, state=None, decode=False):
        """What the generative switching model believes on its own, given the WHOLE sequence (switching dynamics only; no
        counterpart in the reference): filter_regimes forwards, then the GPB2 smoothing pass backwards over the beliefs and pair
        weights the filter kept - kvae_lgssm_switching_smoother.  The bidirectional regime posterior network plays no part.

        1. Encode x, as filter_regimes does.  Every output of filter_regimes but x_pred is returned, with the bits of that call.
        2. regime_smooth [B,T,K] = p(s_t | a_{0:T-1}); regimes [B,T] (int64) = its argmax (lowest index on ties);
           regime_pairs [B,T-1,K,K] = p(s_t = j, s_{t+1} = k | a_{0:T-1}), whose sums over k and j are regime_smooth_t and
           regime_smooth_{t+1}: the expected transition counts of an EM step for P.
        3. mus_smooth [B,T,n], Sigmas_smooth [B,T,n,n]: the smoothed z_t with the regimes summed out (moment-matched);
           a_smooth [B,T,p] = C mus_smooth - on hidden steps (mask [B,T], 1 = observed) it uses the frames after the gap.
        4. decode=True: x_smooth = decoder(a_smooth).
        Also returns a_vae and n_obs [B].  state=prev["state"] starts from an earlier chunk's filter state; the smoothing is then
        conditional on this window alone.  Every Q_k must be positive definite.  Exact when P is the identity or when all
        regimes share A, B, Q; regime_smooth and regime_pairs are exact at T = 2; otherwise the GPB2 approximation (DESIGN.md
        section 15).  No host synchronisation.  Training mode, tau and parameters are left as they were."""
        dyn = self.kalman_filter.dyn_params
        with self._switching_readout("smooth_regimes", x, u, mask, sample_a) as (a_vae, _, _, u, mask):
            out = self.kalman_filter.smooth_regimes(a_vae, u, mask, state=state)
            out["regimes"] = self._argmax_lowest(out["regime_smooth"])
            out["a_smooth"] = out["mus_smooth"] @ dyn.C[0].detach().to(out["regime_smooth"].dtype).mT
            return self._close_readout(out, a_vae, mask, decode, "x_smooth", out["a_smooth"])

    @torch.no_grad()
    def forecast_regimes(self, x, horizon, u=None, mask=None, sample_a=False, origins="all", state=None, decode=False):
        """What the generative switching model expects AHEAD, from every step of a sequence (switching dynamics only; no
        counterpart in the reference): filter_regimes over the T frames, then from the filter's state at every origin t the
        forecast of steps t+1 .. t+H, H = horizon - kvae_lgssm_switching_forecast.  No measurement enters between origin and
        target, so one horizon step is the filter's hidden step; the regime posterior network plays no part and nothing is drawn.

        1. Encode x, as filter_regimes does.  Every output of filter_regimes but x_pred is returned, with the bits of that call.
        2. origins="all": t = 0 .. T-1 (T_o = T); "last": t = T-1 (T_o = 1), the online case after a carried `state`.  A hidden
           origin (mask [B,T], 1 = observed) is legitimate: its state is whatever the filter holds there.  u [B,T+H,m] or None =
           zeros (generate's convention).
        3. Indexed [b, origin, h-1]: regime_fore [B,T_o,H,K] = p(s_{t+h} | a_{0:t}) = regime_filt_t P^h; regimes_fore [B,T_o,H]
           (int64) its argmax (lowest index on ties); a_fore [B,T_o,H,p], S_fore [B,T_o,H,p,p] the mean and covariance of
           a_{t+h} | a_{0:t}; mus_fore [B,T_o,H,n], Sigmas_fore [B,T_o,H,n,n] those of z_{t+h}: all exact under the model.
        4. log_lik_fore [B,T_o,H] = log p(a_{t+h} | a_{0:t}, u), the held-out density of the encoded target frame: exact at h = 1,
           the GPB2 mixture of K^2 Gaussians beyond; exactly 0 where valid [B,T_o,H] (bool: t+h < T and the target is observed)
           is False.  levels_fore [B,T_o,H]: the largest ladder level of the pair densities.
        5. decode=True: x_fore [B,H,C,h,w] = decoder(a_fore) of the LAST origin only.
        Also returns a_vae and n_obs [B].  No host synchronisation.  Training mode, tau and parameters are left as they were."""
        self._needs_switching("forecast_regimes")   # before the checks of horizon and origins; _readout's of mask and u after them
        H = int(horizon)
        if H < 1:
            raise ValueError(f"forecast_regimes: horizon must be >= 1, got {horizon}")
        if origins not in ("all", "last"):
            raise ValueError(f"forecast_regimes: origins must be 'all' or 'last', got {origins!r}")
        T = x.shape[1]
        with self._readout("forecast_regimes", x, u, mask, sample=bool(sample_a), horizon=H) as (a_vae, _, _, u_all, mask):
            out = self.kalman_filter.forecast_regimes(a_vae, None if u is None else u_all, H, mask, origins=origins, state=state)
            out["regimes_fore"] = self._argmax_lowest(out["regime_fore"])
            dev = a_vae.device
            target = torch.arange(0 if origins == "all" else T - 1, T, device=dev)[:, None] + torch.arange(1, H + 1, device=dev)[None, :]
            inside = (target < T).expand(x.shape[0], -1, -1)
            out["valid"] = inside if mask is None else inside & (mask[:, target.clamp(max=T - 1)] != 0)
            return self._close_readout(out, a_vae, mask, decode, "x_fore", out["a_fore"][:, -1])

    @torch.no_grad()
    def viterbi_regimes(self, x, u=None, mask=None, sample_a=False, state=None, smooth=True, decode=False):
        """Segment each sequence into regimes with the generative switching model itself (switching dynamics only; no counterpart
        in the reference): ONE coherent regime path and its exact joint score, by the approximate Viterbi decoder of Pavlovic,
        Rehg & MacCormick (2000) - kvae_lgssm_switching_viterbi.  decode_regimes decodes the amortised q(s | a) of the
        bidirectional posterior network, which has to be trained (after fit_dynamics_em or kf_objective="regime_marginal" it is
        not); the per-step argmax of regime_filt / regime_smooth is not a path - it may use transitions P forbids and has no score.

        1. Encode x, as filter_regimes does.  u [B,T,m] or None = zeros; mask [B,T] optional (1 = observed).
        2. One survivor path per regime, each with its score J_t(j) and the exact Kalman belief along it; every step extends each
           survivor by the best predecessor (lowest index on ties).  regimes [B,T] (int64) = the path that ends in the best final
           score; regimes_log_joint [B] = log p(a, s = regimes | u), EXACT for that path (kalman_filter.path_log_joint gives the
           same number for any path); only the search is approximate.  Also path (int32), path_log_joint, scores [B,T,K],
           backptr [B,T,K], mus_filt [B,T,n], Sigmas_filt [B,T,n,n] (the Kalman-filtered belief given regimes_{0:t}), levels.
        3. state: the survivors after the last step; state=prev["state"] continues a stream - scores, backptr and state of the
           chunks are the bits of the whole-sequence call; a chunk's regimes are conditional on the chunk's own end, the path of
           the stream follows the concatenated backptr back from the last chunk (backptr[:, 0] of a chunk points into the one
           before).  A carried state needs smooth=False: the smoother below starts at (mu0, Sigma0).
        4. smooth=True: the eval-mode smoother pinned to the path, as decode_regimes step 3: mus_smooth, Sigmas_smooth, ABC and
           a_imputed = C_t mu_{t|T}.  decode=True (needs smooth): x_imputed = decoder(a_imputed).
        Also returns a_vae and n_obs [B].  No host synchronisation.  Training mode, tau and parameters are left as they were."""
        dyn = self.kalman_filter.dyn_params
        prelude = self._switching_readout("viterbi_regimes", x, u, mask, sample_a)   # its shape checks come before these
        if decode and not smooth:
            raise ValueError("viterbi_regimes: decode=True needs smooth=True (x_imputed is decoded from the smoothed latents)")
        if smooth and state is not None:
            raise ValueError("viterbi_regimes: a carried state needs smooth=False (the pinned smoother starts at (mu0, Sigma0))")
        with prelude as (a_vae, _, _, u, mask):
            out = self.kalman_filter.viterbi_regimes(a_vae, u, mask, state=state)
            out["regimes"], out["regimes_log_joint"] = out["path"].long(), out["path_log_joint"]
            if smooth:
                dyn.reset_state()
                with dyn.pinned(torch.nn.functional.one_hot(out["regimes"], self.K).to(a_vae.dtype)):
                    ms, Ss, mf, _, _, _, A_list, B_list, C_list = self.kalman_filter.smooth(a_vae, u, mask=mask)
                a_imputed, _ = self.kalman_filter.emission_means(ms, mf, C_list)
                out.update(mus_smooth=ms, Sigmas_smooth=Ss, ABC=(A_list, B_list, C_list), a_imputed=a_imputed)
            return self._close_readout(out, a_vae, mask, decode, "x_imputed", out.get("a_imputed"))

    def fit_dynamics_em(self, batches, iters, update=("A", "B", "Q", "C", "P"), sample_a=False, min_count=None):
        """Closed-form EM for the generative switching model on the encoded sequences (switching dynamics only):
        kvae.train.em.fit_dynamics_em.  The encoder, the decoder and the regime posterior network are not touched.  Returns the
        log-likelihood history, one value per iteration."""
        from kvae.train.em import fit_dynamics_em
        return fit_dynamics_em(self, batches, iters, update=update, sample_a=sample_a, min_count=min_count)

    @torch.no_grad()
    def log_likelihood(self, x, num_samples=1, u=None, mask=None):
        """Importance-weighted bound on log p(x_observed) per sequence under the generative model p(x | a) p_LGSSM(a), with the
        encoder as proposal (no counterpart in the reference).  B sequences of T frames, S = num_samples.

        1. Encode once: a_mu, a_var [B,T,p].  a_s = a_mu + sqrt(a_var) eps_s, eps from kvae.noise.inject(ll_a=[B,S,T,p]) or fresh.
        2. The B*S rows go through the eval-mode filter (mask and u repeated per sample) and kvae_lgssm_predictive:
           log_pa [B,S] = log p_LGSSM(observed a_s), exact.  Switching dynamics take one hard draw of the regime chain per row;
           argmax(logits + Gumbel) is an exact sample of q whatever tau is, so log_ps_qs [B,S] = sum_t (log p(s_t | s_{t-1}) -
           log q(s_t | s_{t-1})) is a valid importance weight.  lstm dynamics give zeros.
        3. One decoder pass over the B*S*T frames: log_px_a [B,S] = sum_t mask_t log p(x_t | a_{s,t}) with the frame model of
           config.out_distr, UNWEIGHTED (scale_reconstruction and beta are training weights and play no part).
        4. log_qa [B,S] = sum_t mask_t log N(a_{s,t}; a_mu_t, a_var_t);  log_w = log_px_a + log_pa - log_qa + log_ps_qs.
        Returns log_px [B] = logsumexp_s log_w - log S, elbo [B] = mean_s log_w (<= log_px), log_w and its four parts [B,S],
        ess [B] = exp(2 lse(log_w) - lse(2 log_w)) in [1, S], n_obs [B].  Training mode and parameters are left as they were."""
        S = int(num_samples)
        if S < 1:
            raise ValueError(f"log_likelihood: num_samples must be >= 1, got {num_samples}")
        dyn = self.kalman_filter.dyn_params
        Bsz, T = x.shape[:2]
        with self._readout("log_likelihood", x, u, mask, sample=False) as (_, a_mu, a_var, u, mask):
            dev, dt = a_mu.device, a_mu.dtype
            eps = _normal("ll_a", (Bsz, S, T, self.a_dim), dev, dt)
            a_s = a_mu.unsqueeze(1) + torch.sqrt(a_var).unsqueeze(1) * eps                      # [B,S,T,p]
            rows = a_s.reshape(Bsz * S, T, self.a_dim)
            mk = torch.ones(Bsz, T, device=dev, dtype=dt) if mask is None else mask
            rep = lambda t: t.repeat_interleave(S, 0)
            dyn.reset_state()
            pred = self.kalman_filter.predictive(rows, rep(u), None if mask is None else rep(mk), want=("seq_ll",))
            log_pa = pred["seq_ll"].to(dt).view(Bsz, S)
            if dyn.is_switching_dynamics:
                lq, lp = dyn.elbo_terms()
                log_ps_qs = (lp - lq).sum(-1).view(Bsz, S)
            else:
                log_ps_qs = torch.zeros(Bsz, S, device=dev, dtype=dt)
            x_logits = self.decode_sequence(rows)
            x_rep = x.to(dt).unsqueeze(1).expand(Bsz, S, *x.shape[1:]).reshape(Bsz * S, *x.shape[1:])
            if self.config.out_distr.lower() == "bernoulli":
                if _native.fused_ok(x_logits) and x_logits.dtype == torch.float32 and x_rep.dtype == torch.float32:
                    from kvae.vae.fused import BernoulliFrameLogLik
                    lpx = BernoulliFrameLogLik.apply(x_logits, x_rep)
                else:
                    lpx = -torch.nn.functional.binary_cross_entropy_with_logits(x_logits, x_rep, reduction="none").sum(dim=(2, 3, 4))
            else:
                x_var = torch.tensor(self.config.noise_pixel_var, device=dev, dtype=dt)
                lpx = log_gaussian(x_rep, x_logits, x_var).sum(dim=(2, 3, 4))
            log_px_a = (lpx.to(dt).view(Bsz, S, T) * mk.unsqueeze(1)).sum(-1)
            log_qa = (log_gaussian(a_s, a_mu.unsqueeze(1), a_var.unsqueeze(1)).sum(-1) * mk.unsqueeze(1)).sum(-1)
            log_w = log_px_a + log_pa - log_qa + log_ps_qs
            lse = torch.logsumexp(log_w, 1)
            return {"log_px": lse - math.log(S), "elbo": log_w.mean(1), "log_w": log_w, "log_px_a": log_px_a, "log_pa": log_pa,
                    "log_qa": log_qa, "log_ps_qs": log_ps_qs, "ess": torch.exp(2.0 * lse - torch.logsumexp(2.0 * log_w, 1)),
                    "n_obs": mk.sum(1)}

    @torch.no_grad()
    def generate(self, x, horizon, num_samples=1, u=None, mask=None, noise=True, decode=True):
        """Continue each sequence: `num_samples` sampled futures of `horizon` frames from the learned dynamics (no counterpart in
        the reference).  B sequences, T0 = x.shape[1] conditioning frames, S = num_samples, H = horizon.

        1. Conditioning: encode x (as forward does) and run the eval-mode filter over it (optional `mask` [B,T0], controls
           u[:, :T0]); hand over mu, Sigma of step T0-1 and, for lstm dynamics, the alpha-network's cell state and next input
           (the frame, or C mu_{t|t-1} where it is hidden), for switching dynamics the regime of step T0-1.
        2. Start: z = mu + L_Sigma eps0 (L_Sigma: the reference's _safe_cholesky ladder); z = mu without noise.
        3. Steps t = T0 .. T0+H-1.  lstm: alpha_t = softmax(head(LSTM(y_{t-1}))) (alpha = 1 for K = 1), A_t|B_t|C_t mixed by
           alpha_t, Q = kalman_filter.Q.  switching: pi_t = s_{t-1} P (sticky prior); with noise s_t = one_hot(argmax(log pi_t +
           Gumbel)), without noise s_t = pi_t - a mean-field read-out, not a sample; A_t|B_t|Q_t mixed by s_t, C_t = C_0.
           Both: z_t = A_t z_{t-1} + B_t u_t + L_{Q_t} eps_t, a_t = C_t z_t + L_R eta_t, and y_t = a_t feeds the next step.
           Without noise the lstm rollout is the filter with the tail hidden: a_t = C_t mu_{t|t-1}.  For the forecast of a
           switching model (exact mean, covariance and regime probabilities at every horizon) use forecast_regimes, not noise=False.
        4. x = decoder(a) through the frame VAE.

        Every draw is made here with torch before the one rollout launch (kvae.noise.inject: gen_z0, gen_z, gen_a, gen_gumbel).
        u: [B, T0+H, m] or None (zeros).  Returns a [B,S,H,p], z [B,S,H,n], weights [B,S,H,K] (alpha or regimes),
        x [B,S,H,C,h,w] (None with decode=False) and a_vae [B,T0,p].  Training mode and parameters are left as they were."""
        horizon, num_samples = int(horizon), int(num_samples)
        if horizon < 1:
            raise ValueError(f"generate: horizon must be >= 1, got {horizon}")
        if num_samples < 1:
            raise ValueError(f"generate: num_samples must be >= 1, got {num_samples}")
        Bsz, T0 = x.shape[:2]
        H, S = horizon, num_samples
        # the conditioning mask goes to condition() as it came, which takes any shape of B*T0 elements
        with self._readout("generate", x, u, None, horizon=H) as (a_vae, _, _, u_all, _):
            kf, dyn = self.kalman_filter, self.kalman_filter.dyn_params
            dev, dt = a_vae.device, a_vae.dtype
            u_cond, u_fut = (u_all, None) if u is None else (u_all[:, :T0], u_all[:, T0:])   # without u: zeros [B,T0,m]
            hand = kf.condition(a_vae, u_cond, mask)
            n, p, K = self.z_dim, self.a_dim, self.K
            switching = dyn.is_switching_dynamics
            draws = dict(eps0=None, eps_z=None, eps_a=None, gumbel=None)
            L0 = LQ = LR = None
            if noise:
                draws.update(eps0=_normal("gen_z0", (Bsz, S, n), dev, dt), eps_z=_normal("gen_z", (Bsz, S, H, n), dev, dt),
                             eps_a=_normal("gen_a", (Bsz, S, H, p), dev, dt))
                if switching:
                    draws["gumbel"] = _gumbel("gen_gumbel", (Bsz, S, H, K), dev, dt)
                L0 = lgssm_ops.safe_cholesky(hand["Sigma"])
                LQ = lgssm_ops.safe_cholesky(dyn.Q.detach() if switching else kf.Q)
                LR = lgssm_ops.safe_cholesky(kf.R)
            if switching:
                kind, extra = "switching", dict(P=dyn._prior_matrix(dev, dt), s0=hand["s"])
            elif K > 1:
                lstm = dyn.lstm
                kind, extra = "lstm", dict(lstm=tuple(t.detach() for t in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0,
                                                                         lstm.bias_hh_l0, dyn.head_w.weight, dyn.head_w.bias)),
                                           h0=hand["h"], c0=hand["c"], y0=hand["y"])
            else:
                kind, extra = "lstm", {}
            a, z, w = lgssm_ops.rollout(kind, dyn.A.detach(), dyn.B.detach(), dyn.C.detach(), hand["mu"], L0, u_fut, LQ, LR, S, H,
                                        **extra, **draws)
            return {"a": a, "z": z, "weights": w, "x": self._decode_latents(a, dt) if decode else None, "a_vae": a_vae}
