"""KalmanFilter — drop-in for kvae.kalman.kalman_filter.KalmanFilter of the reference
(kalman_filter.py:7-401 there) whose filter / smooth / elbo run as HIP kernels on gfx950.

Same constructor, buffers (Q, R, I, mu0, Sigma0 -> identical state_dict keys), method names,
argument order, tuple layouts and tensor shapes:
    filter(Y,U,mask)  -> (mus_filt[B,T,n,1], Sigmas_filt[B,T,n,n], mus_pred, Sigmas_pred, A_list, B_list, C_list)
    smooth(Y,U,mask)  -> (mus_smooth, Sigmas_smooth) + the seven above
    elbo(mu,Sigma,y,u,A_list,B_list,C_list,Q_list=None,mask=None) -> 0-d tensor
Additions over the reference: condition, sample_posterior, predictive (exact log p(a_t | a_{0:t-1}, u), no tape),
log_marginal / marginal (the same density, differentiable: the exact LGSSM training objective) and filter_regimes (the causal
switching Kalman filter over the generative switching model) with its siblings, among them viterbi_regimes / path_log_joint.
What differs is the execution: one launch (sixteen sequences per wavefront at (4,4,2), one wavefront
per sequence at the other shapes; the whole T loop and the RTS sweep inside the kernel) replaces ~580 aten calls per time step, and the backward is a
hand-derived adjoint kernel instead of an autograd tape.  Inputs must live on a HIP device.
Everything native is reached through lgssm_ops (the bridge; it also lays out the packed step record: Slots, alpha_lstm_slots,
slot_view); the read-outs' torch restatements it falls back to are lgssm_torch's.  Which operand form a pass used - a packed
step record or plain stacks - is StepOperands' business (operands.py): every pass leaves its bundle in self._last, and the
read-outs and the ELBO ask that bundle for their operands.
"""
import math

import torch
import torch.nn as nn

from ..noise import normal as _normal
from ..noise import uniform as _uniform
from . import lgssm_ops
from .lgssm_ops import LgssmElbo, LgssmSmooth
from .operands import NO_PASS, StepOperands

# why a read-out of the generative switching model needs switching dynamics (_switching_operands' `why`)
_NO_CHAIN = "the alpha-network of the lstm dynamics has no regime chain to "
_EM_ONLY = "EM is built for the generative switching model, not for the alpha-network of the lstm dynamics"


class KalmanFilter(nn.Module):
    def __init__(self, std_dyn, std_obs, mu0, Sigma0, dyn_params):
        super().__init__()
        self.dyn_params = dyn_params
        n, m, p = dyn_params.A.size(1), dyn_params.B.size(2), dyn_params.C.size(1)
        self.n, self.m, self.p = n, m, p
        dev, dtp = Sigma0.device, Sigma0.dtype
        self.register_buffer("Q", (std_dyn ** 2) * torch.eye(n, dtype=dtp, device=dev))
        self.register_buffer("R", (std_obs ** 2) * torch.eye(p, dtype=dtp, device=dev))
        self.register_buffer("I", torch.eye(n, dtype=dtp, device=dev))
        self.register_buffer("mu0", mu0.clone())
        self.register_buffer("Sigma0", Sigma0.clone())
        self._last = NO_PASS   # StepOperands of the most recent filter pass

    # ------------------------------------------------------------------------------------------
    # per-step operands
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _mask(mask, Y):
        if mask is None:
            return None
        return mask.to(device=Y.device, dtype=Y.dtype).reshape(Y.shape[0], Y.shape[1])

    def _all_observed(self, mask):
        if mask is None:
            return True
        if mask.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lstm dynamics with an explicit mask on a shape outside the in-kernel alpha-network "
                               "(hidden 50, a_dim 2, K <= 16) needs a host check of the mask; pass mask=None inside capture")
        return bool((mask != 0).all())

    def _operands(self, Y, mask):
        """StepOperands of a whole sequence; None if the lstm alpha-net must be stepped because some frames are missing."""
        dyn = self.dyn_params
        Bsz, T, _ = Y.shape
        if dyn.is_switching_dynamics:
            A_seq, B_seq, C_seq, Q_seq = dyn.compute_batch(Y, is_training=self.training)
            packed = dyn.packed_record()
            if packed is None:
                return StepOperands.plain(A_seq, B_seq, C_seq, Q_seq)
            return StepOperands.packed(*packed, views=(A_seq, B_seq, C_seq), C=dyn.C[0], Q_view=Q_seq)
        if dyn.K == 1:
            A, Bm, C = dyn.A[0], dyn.B[0], dyn.C[0]
            ex = lambda M: M.expand(Bsz, T, -1, -1)
            dyn.state_seq = torch.ones(Bsz, T, 1, device=Y.device, dtype=Y.dtype)
            return StepOperands.plain(A, Bm, C, self.Q, views=(ex(A), ex(Bm), ex(C)))
        if not self._all_observed(mask):
            return None
        alpha = dyn.alpha_sequence(Y)
        rec, slots, views = dyn.step_record(alpha)
        dyn.state_seq = alpha
        return StepOperands.packed(rec, slots, views, Q=self.Q)

    # ------------------------------------------------------------------------------------------
    # filter / smooth
    # ------------------------------------------------------------------------------------------
    def filter_step(self, mu_t_t, Sigma_t_t, y_t, u_t, A, B, C, Q, mask_t=None):
        """One predict+update through the HIP filter kernel with T = 1 (reference :31-104).
        Returns (mu_t|t [B,n,1], Sigma_t|t, mu_t|t-1 [B,n,1], Sigma_t|t-1, A, B, C)."""
        Bsz = y_t.size(0)
        mu = mu_t_t.reshape(Bsz, self.n)
        u = u_t.reshape(Bsz, 1, self.m)
        y = y_t.reshape(Bsz, 1, self.p)
        if mask_t is not None:
            mask_t = mask_t.to(device=y.device, dtype=y.dtype).expand(Bsz).reshape(Bsz, 1)
        st = lambda M, r, c: (M if M.dim() == 2 else M.reshape(Bsz, 1, r, c))
        ops = StepOperands.plain(st(A, self.n, self.n), st(B, self.n, self.m), st(C, self.p, self.n), st(Q, self.n, self.n))
        mf, Sf, mp, Sp = LgssmSmooth.apply(y, u, mask_t, *ops.lgssm(self.R, mu.contiguous(),
                                                                     Sigma_t_t.expand(Bsz, -1, -1).contiguous()), False)
        return mf[:, 0].unsqueeze(-1), Sf[:, 0], mp[:, 0].unsqueeze(-1), Sp[:, 0], A, B, C

    def _filter_stepwise(self, Y, U, mask):
        """lstm alpha-net with missing frames: alpha_t needs C mu_{t|t-1} of hidden steps
        (reference :151-185), so the recurrent cell is stepped in PyTorch and every predict+update
        is a T=1 launch of the filter kernel (differentiable end to end)."""
        dyn = self.dyn_params
        Bsz, T, _ = Y.shape
        mu = self.mu0.expand(Bsz, -1)
        Sig = self.Sigma0.expand(Bsz, -1, -1)
        y_for_dyn = Y.new_zeros(Bsz, self.p)
        if dyn.state_seq is None:
            dyn.reset_state()
        outs = [[] for _ in range(7)]
        for t in range(T):
            A, Bm, C = dyn.compute_step(y_for_dyn)
            m_t = mask[:, t]
            mf, Sf, mp, Sp, _, _, _ = self.filter_step(mu, Sig, Y[:, t], U[:, t], A, Bm, C, self.Q, mask_t=m_t)
            for lst, v in zip(outs, (mf, Sf, mp, Sp, A, Bm, C)):
                lst.append(v)
            mu, Sig = mf, Sf
            y_pred = (C @ mp).squeeze(-1)
            y_for_dyn = m_t.view(Bsz, 1) * Y[:, t] + (1.0 - m_t.view(Bsz, 1)) * y_pred
        if isinstance(dyn.state_seq, list) and dyn.state_seq:
            dyn.state_seq = torch.stack(dyn.state_seq, 1)
        return tuple(torch.stack(v, 1) for v in outs)

    @staticmethod
    def _six(outs, with_rts):
        """(ms, Ss, mf, Sf, mp, Sp), the means as [B,T,n,1] columns, of a launch's (ms, Ss,) mf, Sf, mp, Sp; without the RTS sweep
        ms and Ss are None."""
        ms, Ss, mf, Sf, mp, Sp = outs if with_rts else (None, None) + tuple(outs)
        return None if ms is None else ms.unsqueeze(-1), Ss, mf.unsqueeze(-1), Sf, mp.unsqueeze(-1), Sp

    def _alpha_lstm(self, Y, U, mask, with_rts, keep_cell=False):
        """The filter (+ RTS sweep) with the lstm alpha-network run inside the kernel, forward AND backward
        (kvae_lgssm_filter_alpha_lstm / kvae_lgssm_alpha_lstm_bwd).  Leaves the pass's StepOperands in self._last and alpha in
        dyn.state_seq; returns _six of the states and, with keep_cell, the cell's (h_seq, c_seq) [B,T,H]."""
        dyn, n, m, p = self.dyn_params, self.n, self.m, self.p
        outs = lgssm_ops.AlphaLstmSmooth.apply(Y, U, mask, dyn.lstm.weight_ih_l0, dyn.lstm.weight_hh_l0, dyn.lstm.bias_ih_l0,
                                               dyn.lstm.bias_hh_l0, dyn.head_w.weight, dyn.head_w.bias, dyn.A, dyn.B, dyn.C,
                                               self.Q, self.R, self.mu0, self.Sigma0, with_rts, keep_cell)
        k = 6 if with_rts else 4
        rec, dyn.state_seq = outs[k], outs[k + 1]
        slots, _ = lgssm_ops.alpha_lstm_slots(n, m, p)
        views = (lgssm_ops.slot_view(rec, slots.A, n, n), lgssm_ops.slot_view(rec, slots.B, n, m),
                 lgssm_ops.slot_view(rec, slots.C, p, n))
        self._last = StepOperands.packed(rec, slots, views, Q=self.Q)
        return self._six(outs[:k], with_rts), outs[k + 2:]

    def _run(self, Y, U, mask, with_rts):
        if not Y.is_cuda:
            from .. import _native
            _native.lib_for(Y)  # raises: no CPU fallback (unless a test injected the host simulator)
        mask = self._mask(mask, Y)
        dyn = self.dyn_params
        if (mask is not None and not dyn.is_switching_dynamics and dyn.K > 1
                and lgssm_ops.alpha_lstm_supported(Y, dyn.lstm, dyn.K)):
            # lstm dynamics with an explicit mask: whether the mask hides anything is never asked on the host - no sync,
            # capturable, and a mask of ones (the reference's training loop) gives the same numbers as the precomputed-alpha path.
            return self._alpha_lstm(Y, U, mask, with_rts)[0]
        ops = self._operands(Y, mask)
        stepped = ops is None   # lstm + missing frames on shapes outside the fused kernel (or host tensors in the test tier)
        if stepped:
            mf, Sf, mp, Sp, A_l, B_l, C_l = self._filter_stepwise(Y, U, mask)
            ops = StepOperands.plain(A_l, B_l, C_l, self.Q)
        self._last = ops
        if stepped and not with_rts:
            return None, None, mf, Sf, mp, Sp
        # the smoother over stepped filter results too: RTS has no alpha dependence, so the fused op re-runs filter+RTS in one
        # launch on the per-step stacks
        return self._six(LgssmSmooth.apply(Y, U, mask, *ops.lgssm(self.R, self.mu0, self.Sigma0), with_rts), with_rts)

    def filter(self, Y, U, mask=None):
        _, _, mf, Sf, mp, Sp = self._run(Y, U, mask, with_rts=False)
        return (mf, Sf, mp, Sp) + self._last.views

    def smooth(self, Y, U, mask=None):
        ms, Ss, mf, Sf, mp, Sp = self._run(Y, U, mask, with_rts=True)
        return (ms, Ss, mf, Sf, mp, Sp) + self._last.views

    @torch.no_grad()
    def condition(self, Y, U, mask=None):
        """Hand-over of the filter over the conditioning frames Y [B,T0,p] to KVAE.generate: mu_{T0-1|T0-1} [B,n],
        Sigma_{T0-1|T0-1} [B,n,n] and what the dynamics carry across the boundary - lstm (K > 1): the cell state (h, c)
        [B,H] after step T0-1 and the next alpha-network input y [B,p] (the frame if observed, else C_t mu_{t|t-1}:
        reference kalman_filter.py:183-185); switching: the regime s [B,K] of step T0-1."""
        dyn = self.dyn_params
        Bsz, T0, _ = Y.shape
        mask = self._mask(mask, Y)
        dyn.reset_state()
        out = {}
        if (not dyn.is_switching_dynamics and dyn.K > 1 and lgssm_ops.alpha_lstm_supported(Y, dyn.lstm, dyn.K)):
            m = mask if mask is not None else torch.ones(Bsz, T0, device=Y.device, dtype=Y.dtype)
            (_, _, mf, Sf, mp, Sp), (h_seq, c_seq) = self._alpha_lstm(Y, U, m, False, keep_cell=True)
            C_last = self._last.views[2][:, -1]
            out.update(h=h_seq[:, -1], c=c_seq[:, -1])
        else:
            mf, Sf, mp, Sp, _, _, C_list = self.filter(Y, U, mask)
            C_last = C_list[:, -1]
            if not dyn.is_switching_dynamics and dyn.K > 1:   # the cell state: the LSTM over the inputs the filter fed it
                y_dyn = Y if mask is None else (mask.unsqueeze(-1) * Y
                                                + (1.0 - mask.unsqueeze(-1)) * (C_list @ mp).squeeze(-1))
                x = torch.cat([Y.new_zeros(Bsz, 1, self.p), y_dyn[:, :-1]], 1)
                _, (h, c) = dyn.lstm(x)
                out.update(h=h[0], c=c[0])
        if dyn.is_switching_dynamics:
            out["s"] = dyn.state_seq[:, -1]
        elif dyn.K > 1:
            y = Y[:, -1]
            if mask is not None:
                mt = mask[:, -1:]
                y = mt * y + (1.0 - mt) * (C_last @ mp[:, -1]).squeeze(-1)
            out["y"] = y
        out.update(mu=mf[:, -1].squeeze(-1), Sigma=Sf[:, -1])
        return out

    @torch.no_grad()
    def sample_posterior(self, Y, U, mask=None, num_samples=1, noise=True, emission_noise=False):
        """`num_samples` joint samples z_{0:T-1} per sequence from the smoothing posterior p(z_{0:T-1} | a_{0:T-1}, u) (no
        counterpart in the reference, whose smoother returns marginals only): the eval-path filter (as filter(); lstm dynamics
        with a mask step the alpha-network inside the filter kernel, switching dynamics draw ONE regime sequence for the pass),
        then backward sampling over its outputs (lgssm_ops.posterior_paths; include/kvae_lgssm.h kvae_lgssm_posterior_sample).
        The paths are conditional on that one filter pass.  Draws: kvae.noise.inject(post_z=[B,S,T,n], post_a=[B,S,T,p]) or
        fresh ones; noise=False gives the RTS mean mu_{t|T} on every path, emission_noise adds chol(R) eta_t to a_t = C_t z_t.
        Returns dict(z [B,S,T,n], a [B,S,T,p], levels [B,T] (ladder level of each chol(P_t)), filter = filter()'s 7-tuple,
        state_probs)."""
        S = int(num_samples)
        if S < 1:
            raise ValueError(f"sample_posterior: num_samples must be >= 1, got {num_samples}")
        Bsz, T, _ = Y.shape
        _, _, mf, Sf, mp, Sp = self._run(Y, U, mask, with_rts=False)
        eps = _normal("post_z", (Bsz, S, T, self.n), Y.device, Y.dtype) if noise else None
        eta = _normal("post_a", (Bsz, S, T, self.p), Y.device, Y.dtype) if emission_noise else None
        LR = lgssm_ops.safe_cholesky(self.R) if emission_noise else None
        A, Cm, Q, packed, slots = self._last.posterior()
        z, a, levels = lgssm_ops.posterior_paths(mf, Sf, mp, Sp, A, Cm, Q, S, LR, eps, eta, packed=packed, slots=slots)
        return {"z": z, "a": a, "levels": levels, "filter": (mf, Sf, mp, Sp) + self._last.views,
                "state_probs": self.dyn_params.state_seq}

    @torch.no_grad()
    def predictive(self, Y, U, mask=None, want=("ll", "nis", "a_pred", "S", "levels", "seq_ll")):
        """log p(a_t | a_{0:t-1}, u) of every step, exactly: the eval-path filter (as sample_posterior runs it - lstm dynamics
        with a mask step the alpha-network inside the filter kernel, switching dynamics hold ONE regime sequence for the pass),
        then the prediction-error decomposition over its one-step-ahead beliefs (lgssm_ops.predictive; include/kvae_lgssm.h
        kvae_lgssm_predictive).  The filter's (mu0, Sigma0) is the belief before step 0 (reference kalman_filter.py:124-168).
        Returns dict(ll [B,T], nis [B,T], a_pred [B,T,p], S [B,T,p,p], levels [B,T], seq_ll [B], filter = filter()'s 7-tuple,
        state_probs); ll and nis are 0 on hidden steps, a_pred and S are the forecast of every step."""
        _, _, mf, Sf, mp, Sp = self._run(Y, U, mask, with_rts=False)
        Cm, packed, slots = self._last.emission()
        out = lgssm_ops.predictive(mp, Sp, Cm, self.R, Y, self._mask(mask, Y), packed=packed, slots=slots, want=want)
        out.update(filter=(mf, Sf, mp, Sp) + self._last.views, state_probs=self.dyn_params.state_seq)
        return out

    @torch.no_grad()
    def filter_regimes(self, Y, U, mask=None, state=None, want=lgssm_ops._SWF_OUTPUTS):
        """The generative switching model filtered on its own, causally (switching dynamics only): the switching Kalman filter
        with GPB2 collapse over (A_k, B_k, Q_k), the shared C and R, the prior's transition matrix P (unclamped) and
        (mu0, Sigma0) - lgssm_ops.switching_filter; include/kvae_lgssm.h kvae_lgssm_switching_filter.  The regime posterior
        network plays no part and no regime is drawn.  state: the "state" entry of an earlier call continues that stream.
        Returns switching_filter's dict: regime_filt / regime_pred [B,T,K] = p(s_t | a_{0:t}) / p(s_t | a_{0:t-1}), log_lik [B,T]
        = log p(a_t | a_{0:t-1}, u) with the regimes summed out (0 on hidden steps), log_lik_seq [B], a_pred, S, mus_filt,
        Sigmas_filt, levels, state; entries not named in `want` are None."""
        ops = self._switching_operands("filter_regimes", Y, _NO_CHAIN + "filter")
        return lgssm_ops.switching_filter(*ops, Y, U, self._mask(mask, Y), want=want, state=state)

    @torch.no_grad()
    def particle_filter_regimes(self, Y, U, mask=None, num_particles=256, replicates=1, ess_threshold=0.5, state=None,
                                want=lgssm_ops._SPF_OUTPUTS):
        """The generative switching model filtered on its own WITHOUT the GPB2 collapse (switching dynamics only): a
        Rao-Blackwellised particle filter over the model of filter_regimes - `replicates` independent filters of `num_particles`
        particles per sequence, each particle a regime history and an exact Kalman belief - lgssm_ops.switching_pf;
        include/kvae_lgssm.h kvae_lgssm_switching_pf.  exp(log_lik_seq) is an unbiased estimate of p(a | u) for any number of
        particles, regime_filt is consistent, and `paths` are joint draws of regime paths from the model's own posterior.  The
        uniform draws are made here, before the launch (noise slots pf_regime [B,G,T,N], pf_resample [B,G,T]).  state: the "state"
        entry of an earlier call continues that stream.  Returns switching_pf's dict, per replicate; entries not named in `want`
        are None."""
        ops = self._switching_operands("particle_filter_regimes", Y, _NO_CHAIN + "filter")
        if int(num_particles) < 1 or int(replicates) < 1:
            raise ValueError(f"particle_filter_regimes: num_particles and replicates must be >= 1, got {num_particles}, {replicates}")
        dev, dt = Y.device, Y.dtype
        Bsz, T = Y.shape[0], Y.shape[1]
        theta = _uniform("pf_regime", (Bsz, int(replicates), T, int(num_particles)), dev, dt)
        phi = _uniform("pf_resample", (Bsz, int(replicates), T), dev, dt)
        return lgssm_ops.switching_pf(*ops, Y, U, theta, phi, self._mask(mask, Y), ess_threshold=ess_threshold, want=want, state=state)

    @torch.no_grad()
    def smooth_regimes(self, Y, U, mask=None, state=None, want=lgssm_ops._SWS_OUTPUTS):
        """The generative switching model smoothed on its own (switching dynamics only): filter_regimes forwards, then the GPB2
        backward pass over the beliefs and pair weights the filter kept - lgssm_ops.switching_smoother; include/kvae_lgssm.h
        kvae_lgssm_switching_smoother.  The regime posterior network plays no part.  Every Q_k must be positive definite.
        state: as filter_regimes; the smoothing is then conditional on this window alone.  Returns filter_regimes' dict (the
        same bits) plus regime_smooth [B,T,K] = p(s_t | a_{0:T-1}), regime_pairs [B,T-1,K,K] = p(s_t, s_{t+1} | a_{0:T-1}),
        mus_smooth [B,T,n], Sigmas_smooth [B,T,n,n]; entries not named in `want` are None."""
        ops = self._switching_operands("smooth_regimes", Y, _NO_CHAIN + "smooth")
        return lgssm_ops.switching_smoother(*ops, Y, U, self._mask(mask, Y), want=want, state=state)

    @torch.no_grad()
    def forecast_regimes(self, Y, U, horizon, mask=None, origins="all", state=None, want=lgssm_ops._SWH_OUTPUTS):
        """The generative switching model looking ahead (switching dynamics only): filter_regimes over Y [B,T,p], then from the
        filter's state at every origin t the forecast of steps t+1 .. t+horizon, each horizon step the filter's hidden step -
        lgssm_ops.switching_forecast; include/kvae_lgssm.h kvae_lgssm_switching_forecast.  U [B,T+horizon,m] or None = zeros.
        origins: "all" (T_o = T) or "last" (T_o = 1).  state: as filter_regimes.  Returns filter_regimes' dict (the same bits) plus,
        indexed [b, origin, h-1], regime_fore [B,T_o,H,K], a_fore [B,T_o,H,p], S_fore [B,T_o,H,p,p], mus_fore [B,T_o,H,n],
        Sigmas_fore [B,T_o,H,n,n] (exact under the model), log_lik_fore [B,T_o,H] = log p(a_{t+h} | a_{0:t}, u) (0 where the target
        is hidden or past the end), levels_fore [B,T_o,H]; entries not named in `want` are None."""
        ops = self._switching_operands("forecast_regimes", Y, _NO_CHAIN + "forecast")
        return lgssm_ops.switching_forecast(*ops, Y, U, horizon, self._mask(mask, Y), origins=origins, want=want, state=state)

    @torch.no_grad()
    def viterbi_regimes(self, Y, U, mask=None, state=None, want=lgssm_ops._SWV_OUTPUTS):
        """The most likely regime path of the generative switching model on its own (switching dynamics only): the approximate
        Viterbi decoder of Pavlovic, Rehg & MacCormick over the model of filter_regimes - one survivor path per regime, each with
        its score and exact Kalman belief - lgssm_ops.switching_viterbi; include/kvae_lgssm.h kvae_lgssm_switching_viterbi.  The
        regime posterior network plays no part.  state: the "state" entry of an earlier call continues that stream.  Returns
        switching_viterbi's dict: path [B,T] (int32), path_log_joint [B] = the exact log p(a, s = path | u) (path_log_joint()
        recomputes it for any path), scores [B,T,K], backptr [B,T,K], mus_filt, Sigmas_filt (the Kalman-filtered belief given
        path_{0:t}), levels, state; entries not named in `want` are None."""
        ops = self._switching_operands("viterbi_regimes", Y, _NO_CHAIN + "decode")
        return lgssm_ops.switching_viterbi(*ops, Y, U, self._mask(mask, Y), want=want, state=state)

    @torch.no_grad()
    def path_log_joint(self, Y, U, path, mask=None):
        """log p(a, s = path | u) [B] of ANY regime path [B,T] (integers below K) under the generative switching model, exactly
        (switching dynamics only): the chain term -log K + sum_t log P[path_{t-1}, path_t] with the prior's unclamped P, plus the
        prediction-error decomposition of the filter pinned to that path (predictive).  It is the yardstick of a segmentation:
        viterbi_regimes' path_log_joint is this number for its own path."""
        self._switching_operands("path_log_joint", Y, _NO_CHAIN + "score a path of")
        dyn = self.dyn_params
        Bsz, T = Y.shape[0], Y.shape[1]
        path = path.to(device=Y.device, dtype=torch.long)
        if tuple(path.shape) != (Bsz, T):
            raise ValueError(f"path_log_joint: path must be [B, T] = [{Bsz}, {T}], got {list(path.shape)}")
        dyn.reset_state()
        with dyn.pinned(torch.nn.functional.one_hot(path, dyn.K).to(Y.dtype)):
            seq_ll = self.predictive(Y, U, mask, want=("seq_ll",))["seq_ll"]
        logP = dyn._prior_matrix(Y.device, Y.dtype).log()
        chain = logP[path[:, :-1], path[:, 1:]].sum(1) - math.log(dyn.K)   # (a Python constant: nothing is copied to the device)
        return seq_ll.to(Y.dtype) + chain

    def regime_log_marginal(self, Y, U, mask=None):
        """log p(a | u) of the generative switching model with the regimes summed out under GPB2 collapse, DIFFERENTIABLY (switching
        dynamics only): filter_regimes' log_lik / log_lik_seq / levels - the same bits - with a tape through A_k, B_k, Q_k, the
        shared C, (mu0, Sigma0), Y and U - lgssm_ops.switching_log_marginal; include/kvae_lgssm.h kvae_lgssm_switching_marginal and
        its adjoint.  The regime posterior network plays no part and no regime is drawn: zero variance, no tau.  It is the gradient
        of the GPB2 value: exact where the filter is exact (P = I, shared A / B / Q, t <= 1), elsewhere the gradient of the
        approximation.  R and the prior's P are constants.  Returns dict(ll [B,T], seq_ll [B], levels [B,T]); ll is 0 on hidden steps."""
        ops = self._switching_operands("regime_log_marginal", Y, _NO_CHAIN + "sum out", detach=False)   # the tape runs through them
        return lgssm_ops.switching_log_marginal(*ops, Y, U, self._mask(mask, Y))

    def _switching_operands(self, who, Y, why, detach=True):
        """What every lgssm_ops.switching_* call opens with: (A_k, B_k, Q_k, the shared C, R, the prior's P on Y's device, mu0, Sigma0)
        of the generative switching model, the parameters detached unless `detach` is False.  Without switching dynamics: ValueError,
        `who` needs them because `why`."""
        dyn = self.dyn_params
        if not dyn.is_switching_dynamics:
            raise ValueError(f"{who} needs switching dynamics (SwitchingDynamicsParameter): {why}")
        params = (dyn.A, dyn.B, dyn.Q, dyn.C[0])
        return (*(t.detach() if detach else t for t in params), self.R, dyn._prior_matrix(Y.device, Y.dtype), self.mu0, self.Sigma0)

    @torch.no_grad()
    def em_statistics(self, Y, U, mask=None, want=lgssm_ops._EM_OUTPUTS):
        """The E-step of EM for the generative switching model (switching dynamics only; K = 1 is allowed): smooth_regimes, whose
        backward pass also crosses the transition into t = 0 and accumulates the expected sufficient statistics of (A_k, B_k,
        Q_k), (C, R), P and (mu0, Sigma0) - lgssm_ops.switching_em_statistics; include/kvae_lgssm.h kvae_lgssm_switching_em.  The
        regime posterior network plays no part.  Returns the sums over the batch (additive over batches: lgssm_ops.em_add),
        log_lik_seq [B] and smooth_regimes' four outputs; entries not named in `want` are None.  No host synchronisation: the call
        can be captured into a hipGraph."""
        ops = self._switching_operands("em_statistics", Y, _EM_ONLY)
        return lgssm_ops.switching_em_statistics(*ops, Y, U, self._mask(mask, Y), want=want)

    @torch.no_grad()
    def em_step(self, Y, U, mask=None, update=("A", "B", "Q", "C", "P"), stats=None, min_count=None):
        """One EM iteration of the generative switching model in closed form (switching dynamics only): em_statistics over
        (Y, U, mask) - or the `stats` given, e.g. added over several batches with lgssm_ops.em_add - then
        lgssm_ops.switching_em_mstep.  update: which of "A", "B", "Q", "C", "R", "P", "mu0", "Sigma0" to re-estimate.  The new values
        are copied into dyn_params.A / B / Q / C (the one shared C into every slice), a new prior.transition_matrix is assigned (so
        that its cached device copy is rebuilt), and the buffers R, mu0, Sigma0 are written only when they are named.  A regime
        with fewer than min_count (default n + m + 1) expected visits, or whose new Q_k is not positive definite, keeps its
        parameters; a row of P without counts keeps its values; without a control input (u identically 0) B_k is held and A_k
        is fitted given it.  Returns dict(log_lik = sum_b log p(a_b | u_b) BEFORE the step - None if `stats` holds no log_lik_seq -
        stats, skipped = switching_em_mstep's {"regimes": [...], "rows": [...], "B_held": [...], "emission": bool}).  The M-step
        reads the skipped lists back: it synchronises with the host and cannot be captured into a hipGraph (em_statistics can)."""
        update = lgssm_ops._want("em_step", lgssm_ops._EM_PARAMS, update)
        ops = self._switching_operands("em_step", self.mu0 if Y is None else Y, _EM_ONLY)   # Y, U may be None when `stats` is given
        if stats is None:
            stats = self.em_statistics(Y, U, mask, want=lgssm_ops._EM_STATS + ("log_lik_seq",))
        dyn = self.dyn_params
        old = dict(zip(("A", "B", "Q", "C", "R", "P", "mu0", "Sigma0"), ops))
        new, skipped = lgssm_ops.switching_em_mstep(stats, old, update, min_count)
        for k in ("A", "B", "Q"):
            if k in update:
                getattr(dyn, k).copy_(new[k].to(getattr(dyn, k)))
        if "C" in update:
            dyn.C.copy_(new["C"].to(dyn.C).expand_as(dyn.C))
        if "P" in update:
            P_old = dyn.prior.transition_matrix
            dyn.prior.transition_matrix = new["P"].to(device=P_old.device, dtype=P_old.dtype)
        for k in ("R", "mu0", "Sigma0"):
            if k in update:
                getattr(self, k).copy_(new[k].to(getattr(self, k)))
        lls = stats.get("log_lik_seq")   # None when the caller's statistics were made without it
        return {"log_lik": None if lls is None else lls.double().sum(), "stats": stats, "skipped": skipped}

    def regime_marginal(self, y_t, u_t, mask=None):
        """The regime-marginal objective, normalised as elbo(): sum_b log p(a_b | u_b) / num_el with the regimes summed out
        (regime_log_marginal) - no log_p - log_q term, no draw of any kind."""
        Bsz, T = y_t.size(0), y_t.size(1)
        mask = self._mask(mask, y_t)
        out = self.regime_log_marginal(y_t, u_t, mask)
        self.last_marginal_levels = out["levels"]
        num_el = mask.sum().clamp(min=1.0) if mask is not None else float(Bsz * T)
        return out["seq_ll"].sum() / num_el

    def log_marginal(self, Y, U, mask=None):
        """log p(a | u), exactly and DIFFERENTIABLY: the filter (training or eval dynamics as self.training says; no RTS sweep),
        then lgssm_ops.log_marginal over its one-step-ahead beliefs - C_t out of the packed step record where there is one.
        predictive() is the eval-only, no-grad read-out of the same density.  Gradients reach Y, U, A / B / C, the alpha-LSTM
        and the switching model's bi-GRU and regime chain through the filter's own Functions (the in-kernel alpha-LSTM path takes
        the C-slot gradient as the upstream of its record).  Returns dict(ll [B,T], seq_ll [B], levels [B,T], filter = filter()'s
        7-tuple, state_probs); ll is 0 on hidden steps."""
        _, _, mf, Sf, mp, Sp = self._run(Y, U, mask, with_rts=False)
        out = self._log_marginal(mp, Sp, Y, self._last.views[2], mask)
        out.update(filter=(mf, Sf, mp, Sp) + self._last.views, state_probs=self.dyn_params.state_seq)
        return out

    def _log_marginal(self, mus_pred, Sigmas_pred, y_t, C_list, mask=None):
        Cm, packed, slots = self._last.emission(C_list)
        return lgssm_ops.log_marginal(mus_pred, Sigmas_pred, Cm, self.R, y_t, self._mask(mask, y_t), packed=packed, slots=slots)

    def marginal(self, mus_pred, Sigmas_pred, y_t, C_list, mask=None):
        """The exact LGSSM objective, normalised as elbo(): (sum_b log p(a_b | u_b) [+ log_p - log_q of the regime chain]) / num_el,
        over the filter's one-step-ahead beliefs - no smoothed stacks, no eps_z draw."""
        Bsz, T = y_t.size(0), y_t.size(1)
        mask = self._mask(mask, y_t)
        out = self._log_marginal(mus_pred, Sigmas_pred, y_t, C_list, mask)
        self.last_marginal_levels = out["levels"]
        total = out["seq_ll"].sum()
        if self.dyn_params.is_switching_dynamics:
            log_q, log_p = self.dyn_params.elbo_terms()
            total = total + log_p.sum() - log_q.sum()
        num_el = mask.sum().clamp(min=1.0) if mask is not None else float(Bsz * T)
        return total / num_el

    def emission_means(self, mus_smooth, mus_filt, C_list):
        """(C_t mu_t|T, C_t mu_t|t): the two latent read-outs KVAE.impute decodes (reference model.py:279-288), one launch."""
        _, packed, slots = self._last.emission(C_list)
        return lgssm_ops.emission_means(mus_smooth, mus_filt, C_list, packed, slots.C)

    # ------------------------------------------------------------------------------------------
    # ELBO
    # ------------------------------------------------------------------------------------------
    def elbo(self, mu_t_T, Sigma_t_T, y_t, u_t, A_list, B_list, C_list, Q_list=None, mask=None, eps=None):
        Bsz, T = y_t.size(0), y_t.size(1)
        mask = self._mask(mask, y_t)
        ops = self._last
        if Q_list is not None or not ops.owns(A_list, B_list, C_list):   # operands of the caller's own: plain stacks
            Q = Q_list if Q_list is not None else getattr(self.dyn_params, "Q_seq", None)
            ops = StepOperands.plain(A_list, B_list, C_list, self.Q if Q is None else Q)
        if eps is None:
            eps = _normal("eps_z", (Bsz, T, self.n), y_t.device, y_t.dtype)
        else:
            eps = eps.to(device=y_t.device, dtype=y_t.dtype)
        total, self.last_elbo_terms, self.last_chol_levels = LgssmElbo.apply(
            mu_t_T, Sigma_t_T, eps, y_t, u_t, mask, *ops.lgssm(self.R, self.mu0, self.Sigma0))
        if self.dyn_params.is_switching_dynamics:
            log_q, log_p = self.dyn_params.elbo_terms()
            total = total + log_p.sum() - log_q.sum()
        num_el = mask.sum().clamp(min=1.0) if mask is not None else float(Bsz * T)
        return total / num_el
