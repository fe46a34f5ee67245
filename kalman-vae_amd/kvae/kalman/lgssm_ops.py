"""torch.autograd bridge to the HIP LGSSM kernels (C ABI: include/kvae_lgssm.h).

PyTorch is plumbing here: it owns device memory, the current HIP stream and the autograd graph.
Every numerical step of filter / RTS smoother / ELBO / mixing / recurrences / linear heads — forward and backward,
including the weight gradients of the LSTM / bi-GRU / heads (`kvae_rnn_wgrad`: no library GEMM on the path) — runs in
libkvae_lgssm.so; only trivial reductions (`terms.sum`) stay torch ops on the same stream.  Nothing computes on the host.

Per-step operands (A_t, B_t, C_t, Q_t) reach the kernels as strided "stacks": either slots of ONE
packed record tensor [B,T,E] produced by `mix_dynamics` (mixture-of-K case: a single launch writes
a whole step record, a single tensor carries its gradient) or a plain tensor that is broadcast
([r,c]) or per-step ([B,T,r,c]).

This module is the bridge only.  The read-outs (regime_decode, rollout, posterior_paths, predictive, log_marginal,
switching_filter, switching_smoother, switching_log_marginal, switching_em_statistics, switching_pf, switching_forecast, switching_viterbi) dispatch between their kernel and its restatement in torch ops;
the restatements - also the float64 references of the tests - and safe_cholesky / safe_cholesky_items live in lgssm_torch (no
native library behind it) and are re-exported here.
"""
import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from .. import _native as N
from .lgssm_torch import (_DECODE_OUTPUTS, _EM_OUTPUTS, _EM_PARAMS, _EM_STATS, _LOG_2PI, _PRED_OUTPUTS, _SPF_OUTPUTS, _SWF_OUTPUTS, _SWH_FORE, _SWH_OUTPUTS, _SWS_OUTPUTS, _SWS_SMOOTH, _SWV_OUTPUTS, _bt,  # noqa: F401 (re-exported)
                          SPF_PARTICLES, _spf_draws, _spf_state, _swf_state, _swh_args, _swv_state, _want, lineages, switching_pf_torch, log_marginal_torch, posterior_paths_torch, predictive_torch, regime_decode_torch,
                          rollout_torch, safe_cholesky, safe_cholesky_items, switching_em_mstep, switching_em_statistics_torch,
                          switching_filter_torch, switching_forecast_torch, switching_log_marginal_torch, switching_smoother_torch, switching_viterbi_torch)


class Slots(NamedTuple):
    """Float offsets of A|B|C|Q inside one packed step record (None = operand is not packed)."""
    A: Optional[int] = None
    B: Optional[int] = None
    C: Optional[int] = None
    Q: Optional[int] = None


def alpha_lstm_slots(n, m, p):
    """(Slots, record width E) of the step record A | B | C the in-kernel alpha-LSTM writes (AlphaLstmSmooth)."""
    return Slots(A=0, B=n * n, C=n * n + n * m), n * n + n * m + p * n


def slot_view(packed, off, r, c):
    """The [..., r, c] view of the slot at float offset `off` of a packed step record [..., E]."""
    return packed[..., off:off + r * c].unflatten(-1, (r, c))


def _empty(dev, *shape, dt=torch.float32):
    return torch.empty(*shape, device=dev, dtype=dt)


_INT32_OUTPUTS = ("levels", "levels_fore", "resampled", "regimes", "ancestors", "paths", "path", "backptr", "ws_bp")


def _wanted(dev, outputs, want, shapes):
    """{name: a fresh tensor of shapes[name] if the name is wanted, else None} over `outputs`; _INT32_OUTPUTS are int32."""
    return {k: _empty(dev, *shapes[k], dt=torch.int32 if k in _INT32_OUTPUTS else torch.float32) if (k in want and k in shapes) else None
            for k in outputs}


def _read_by(dev, out, name, readers, want, shape):
    """The buffer of an output that the launches of other outputs read (the sequence sums read log_lik, the lineage walk reads the
    regimes and ancestors): it exists when `name` or one of `readers` is wanted; out[name] holds it only when `name` itself is."""
    mine = name in want
    buf = _empty(dev, *shape, dt=torch.int32 if name in _INT32_OUTPUTS else torch.float32) if (mine or any(r in want for r in readers)) else None
    out[name] = buf if mine else None
    return buf


def _bind(pr, fields):
    """Point the ctypes struct `pr` at the tensors of {field: tensor or None} (None = NULL): the tensors, which must outlive the call."""
    for k, t in fields.items():
        setattr(pr, k, None if t is None else t.data_ptr())
    return tuple(fields.values())


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _stack(t, Bsz, T, r, c, packed=None, off=None):
    """(tensor_to_keep_alive, N.Stack) for one per-step operand."""
    if off is not None:
        E = packed.shape[-1]
        return packed, N.Stack(packed.data_ptr() + 4 * off, T * E, E)
    if t.dim() == 2:
        t = _f32c(t)
        return t, N.Stack(t.data_ptr(), 0, 0)
    if t.shape != (Bsz, T, r, c):
        t = t.expand(Bsz, T, r, c)
    if t.dtype != torch.float32 or t.stride(-1) != 1 or t.stride(-2) != c:
        t = t.float().contiguous()
    return t, N.Stack(t.data_ptr(), t.stride(0), t.stride(1))


class _Call:
    """Builds the kvae_lgssm_problem for one call and keeps every tensor alive until it returns."""

    def __init__(self, Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots):
        self.Y, self.U = _f32c(Y), _f32c(U)
        Bsz, T, p = self.Y.shape
        m = self.U.shape[-1]
        n = Sigma0.shape[-1]
        self.dims = (Bsz, T, n, m, p)
        self.mask = _f32c(mask)
        self.packed = _f32c(packed)
        self.R, self.mu0, self.Sigma0 = _f32c(R), _f32c(mu0), _f32c(Sigma0)
        self.keep = []
        prob = N.Problem()
        prob.B, prob.T, prob.n, prob.m, prob.p = Bsz, T, n, m, p
        for name, t, r, c, off in (("A", A, n, n, slots.A), ("Bm", Bm, n, m, slots.B),
                                   ("C", Cm, p, n, slots.C), ("Q", Q, n, n, slots.Q)):
            keep, st = _stack(t, Bsz, T, r, c, self.packed, off)
            self.keep.append(keep)
            setattr(prob, name, st)
        prob.R = self.R.data_ptr()
        prob.mu0 = self.mu0.data_ptr()
        prob.mu0_sb = n if self.mu0.dim() == 2 else 0
        prob.Sigma0 = self.Sigma0.data_ptr()
        prob.Sigma0_sb = n * n if self.Sigma0.dim() == 3 else 0
        prob.Y, prob.U = self.Y.data_ptr(), self.U.data_ptr()
        prob.mask = self.mask.data_ptr() if self.mask is not None else None
        self.prob = prob
        self.lib = N.lib_for(self.Y)
        self.stream = N.stream_for(self.Y)


def _states(mf, Sf, mp, Sp, ms=None, Ss=None, aux=None):
    st = N.States()
    for k, t in (("mus_filt", mf), ("Sigmas_filt", Sf), ("mus_pred", mp), ("Sigmas_pred", Sp),
                 ("mus_smooth", ms), ("Sigmas_smooth", Ss), ("aux", aux)):
        setattr(st, k, t.data_ptr() if t is not None else None)
    return st


def _reduce_to(buf, t):
    """The per-step gradient buf [B,T,r,c] reduced to the shape of the operand t the caller passed in."""
    if t.dim() == 2:
        return buf.sum((0, 1))
    return buf.sum_to_size(t.shape) if tuple(t.shape) != tuple(buf.shape) else buf


class _GradSink:
    """Gradient buffers for the per-step operands (and, where asked for, the prior) + the autograd return values built from them."""

    def __init__(self, call, packed, A, Bm, Cm, Q, slots, need_q, need_mu0=False, need_Sigma0=False):
        Bsz, T, n, m, p = call.dims
        dev = call.Y.device
        self.g = N.InputGrads()
        self.out = {}
        self.gpacked = torch.empty_like(call.packed) if packed is not None else None
        for name, t, r, c, off in (("gA", A, n, n, slots.A), ("gB", Bm, n, m, slots.B),
                                   ("gC", Cm, p, n, slots.C), ("gQ", Q, n, n, slots.Q)):
            if off is not None:
                E = self.gpacked.shape[-1]
                setattr(self.g, name, N.Stack(self.gpacked.data_ptr() + 4 * off, T * E, E))
            elif name == "gQ" and not need_q:
                setattr(self.g, name, N.Stack(None, 0, 0))
            else:
                buf = _empty(dev, Bsz, T, r, c)
                self.out[name] = (buf, t)
                setattr(self.g, name, N.Stack(buf.data_ptr(), T * r * c, r * c))
        self.gY = torch.empty_like(call.Y)
        self.gU = torch.empty_like(call.U)
        self.g.gY, self.g.gU = self.gY.data_ptr(), self.gU.data_ptr()
        self.g_mu0 = _empty(dev, Bsz, n) if need_mu0 else None
        self.g_Sigma0 = _empty(dev, Bsz, n, n) if need_Sigma0 else None
        self.g.g_mu0, self.g.g_Sigma0 = N.ptr(self.g_mu0), N.ptr(self.g_Sigma0)
        self.shared_prior = (call.mu0.dim() == 1, call.Sigma0.dim() == 2)

    def operand_grad(self, name, scale=None):
        """Gradient for a non-packed operand, reduced to the shape the caller passed in."""
        if name not in self.out:
            return None
        buf, t = self.out[name]
        return _reduce_to(buf if scale is None else buf * scale, t)

    def prior_grads(self):
        """(g_mu0, g_Sigma0) once the launch has written them per sequence: summed over the batch where the prior was shared."""
        return tuple(N.colsum(g) if (g is not None and shared) else g
                     for g, shared in zip((self.g_mu0, self.g_Sigma0), self.shared_prior))


# ------------------------------------------------------------------------------------------------
# filter (+ RTS smoother)
# ------------------------------------------------------------------------------------------------
class LgssmSmooth(torch.autograd.Function):
    """KalmanFilter.filter / .smooth (reference kalman_filter.py:107-201, 240-279) in one launch."""

    @staticmethod
    def forward(ctx, Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots, with_rts):
        call = _Call(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots)
        Bsz, T, n, m, p = call.dims
        dev = call.Y.device
        mf, Sf, mp, Sp = _empty(dev, Bsz, T, n), _empty(dev, Bsz, T, n, n), _empty(dev, Bsz, T, n), _empty(dev, Bsz, T, n, n)
        ms, Ss = (_empty(dev, Bsz, T, n), _empty(dev, Bsz, T, n, n)) if with_rts else (None, None)
        # gains (K | S | J) kept for the backward; consumed by the n=4,p=2 fused-phase kernels
        aux = _empty(dev, Bsz, T, n * p + p * p + n * n) if any(ctx.needs_input_grad) else None
        st = _states(mf, Sf, mp, Sp, ms, Ss, aux)
        fn = call.lib.dll.kvae_lgssm_smooth_fwd if with_rts else call.lib.dll.kvae_lgssm_filter_fwd
        call.lib.check(N.timed("smooth_fwd" if with_rts else "filter_fwd", call.Y,
                               lambda: fn(C.byref(call.prob), C.byref(st), call.stream)), "kvae_lgssm_smooth_fwd")
        ctx.slots, ctx.with_rts = slots, with_rts
        # outputs nobody differentiates arrive as None in backward (not as materialised zero stacks): the kernels take
        # NULL for "no upstream gradient" and skip the loads
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, mf, Sf, mp, Sp, ms, Ss, aux)
        if with_rts:
            return ms, Ss, mf, Sf, mp, Sp
        return mf, Sf, mp, Sp

    @staticmethod
    def backward(ctx, *gouts):
        Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, mf, Sf, mp, Sp, ms, Ss, aux = ctx.saved_tensors
        slots, with_rts = ctx.slots, ctx.with_rts
        call = _Call(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots)
        Bsz, T, n, m, p = call.dims
        if with_rts:
            g_ms, g_Ss, g_mf, g_Sf, g_mp, g_Sp = (_f32c(g) for g in gouts)
        else:
            g_mf, g_Sf, g_mp, g_Sp = (_f32c(g) for g in gouts)
            g_ms = g_Ss = None
        need = ctx.needs_input_grad
        need_q = slots.Q is not None or (Q is not None and need[7])
        sink = _GradSink(call, packed, A, Bm, Cm, Q, slots, need_q, need[9], need[10])
        ws = _empty(Y.device, Bsz, T, 2 * (n + n * n))
        saved = _states(mf, Sf, mp, Sp, ms, Ss, aux)
        up = _states(g_mf, g_Sf, g_mp, g_Sp, g_ms, g_Ss)
        call.lib.check(N.timed("smooth_bwd", call.Y, lambda: call.lib.dll.kvae_lgssm_smooth_bwd(
            C.byref(call.prob), C.byref(saved), C.byref(up), C.byref(sink.g), N.ptr(ws), int(with_rts), call.stream)),
            "kvae_lgssm_smooth_bwd")
        g0, S0 = sink.prior_grads()
        return (sink.gY if need[0] else None, sink.gU if need[1] else None, None, sink.gpacked,
                sink.operand_grad("gA"), sink.operand_grad("gB"), sink.operand_grad("gC"),
                sink.operand_grad("gQ") if need_q else None, None, g0, S0, None, None)


# ------------------------------------------------------------------------------------------------
# ELBO
# ------------------------------------------------------------------------------------------------
class LgssmElbo(torch.autograd.Function):
    """The LGSSM terms of KalmanFilter.elbo (reference kalman_filter.py:347-389), summed over B and T.
    Returns (total, per_term[4], levels int32[3]); gradients are produced in the forward launch (unit upstream) and
    scaled by the incoming scalar gradient in backward.  levels (device, no host sync): the whole-batch _safe_cholesky level
    the launch resolved for Sigma_s and for Q_t (0..4 = jitter 1e-6 * 10^level, 5 = diagonal fallback) and the kernel family
    that computed the call (include/kvae_lgssm.h)."""

    @staticmethod
    def forward(ctx, mus, Sigs, eps, Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots):
        call = _Call(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots)
        Bsz, T, n, m, p = call.dims
        dev = call.Y.device
        mus_c = _f32c(mus.reshape(Bsz, T, n))
        Sigs_c, eps_c = _f32c(Sigs), _f32c(eps)
        terms = _empty(dev, Bsz, T, 4)
        levels = _empty(dev, 3, dt=torch.int32)   # (level of Sigma_s, level of Q_t, kernel family of the launch)
        ws_lz = _empty(dev, Bsz, T, n)   # z_t parked by the probe launch
        want = any(ctx.needs_input_grad)
        g_mus = g_Sigs = sink = None
        if want:
            need_q = slots.Q is not None or (Q is not None and ctx.needs_input_grad[10])
            sink = _GradSink(call, packed, A, Bm, Cm, Q, slots, need_q)
            g_mus, g_Sigs = torch.empty_like(mus_c), torch.empty_like(Sigs_c)
            ctx.need_q = need_q
        call.lib.check(N.timed("elbo", call.Y, lambda: call.lib.dll.kvae_lgssm_elbo(
            C.byref(call.prob), N.ptr(mus_c), N.ptr(Sigs_c), N.ptr(eps_c), N.ptr(terms), N.ptr(levels), N.ptr(ws_lz), N.ptr(g_mus),
            N.ptr(g_Sigs), C.byref(sink.g) if sink else None, call.stream)), "kvae_lgssm_elbo")
        per_term = terms.sum((0, 1))
        ctx.sink, ctx.g_mus, ctx.g_Sigs, ctx.mus_shape = sink, g_mus, g_Sigs, mus.shape
        ctx.mark_non_differentiable(per_term, levels)
        ctx.set_materialize_grads(False)
        return per_term.sum(), per_term, levels

    @staticmethod
    def backward(ctx, g_total, _g_terms, _g_levels):
        if g_total is None:
            return (None,) * 15
        sink, need = ctx.sink, ctx.needs_input_grad
        s = g_total
        gp = sink.gpacked * s if sink.gpacked is not None else None
        return ((ctx.g_mus * s).reshape(ctx.mus_shape) if need[0] else None,
                ctx.g_Sigs * s if need[1] else None, None,
                sink.gY * s if need[3] else None, sink.gU * s if need[4] else None, None, gp,
                sink.operand_grad("gA", s), sink.operand_grad("gB", s), sink.operand_grad("gC", s),
                sink.operand_grad("gQ", s) if ctx.need_q else None, None, None, None, None)


# ------------------------------------------------------------------------------------------------
# mixture-of-K dynamics
# ------------------------------------------------------------------------------------------------
class MixDynamics(torch.autograd.Function):
    """record[b,t,:] = sum_k alpha[b,t,k] base[k,:]  (reference dyn_param.py:58-60,
    switch_dyn_param.py:82-84), base = the K flattened matrices packed side by side."""

    @staticmethod
    def forward(ctx, alpha, base):
        a, bs = _f32c(alpha), _f32c(base)
        Bsz, T, K = a.shape
        E = bs.shape[1]
        out = _empty(a.device, Bsz, T, E)
        lib = N.lib_for(a)
        lib.check(lib.dll.kvae_mix_fwd(N.ptr(a), N.ptr(bs), N.ptr(out), Bsz * T, K, E, N.stream_for(a)), "kvae_mix_fwd")
        ctx.save_for_backward(a, bs)
        return out

    @staticmethod
    def backward(ctx, g_out):
        return _mix_bwd(*ctx.saved_tensors, _f32c(g_out))


def _mix_bwd(alpha, base, g_rec):
    """(g_alpha, g_base) of record = sum_k alpha_k base_k from g_rec [B,T,E]: kvae_mix_bwd with its partials workspace."""
    Bsz, T, K = alpha.shape
    E = base.shape[1]
    lib = N.lib_for(alpha)
    partials = _empty(alpha.device, lib.dll.kvae_mix_bwd_partials(Bsz * T), K, E)
    g_alpha, g_base = torch.empty_like(alpha), torch.empty_like(base)
    lib.check(lib.dll.kvae_mix_bwd(N.ptr(alpha), N.ptr(base), N.ptr(g_rec), N.ptr(g_alpha), N.ptr(g_base), N.ptr(partials),
                                   Bsz * T, K, E, 0, N.stream_for(alpha)), "kvae_mix_bwd")
    return g_alpha, g_base


def mix_dynamics(alpha, mats):
    """alpha [B,T,K]; mats: list of [K,r,c] parameters. Returns (record [B,T,E], offsets, views)."""
    base = torch.cat([mt.reshape(mt.shape[0], -1) for mt in mats], dim=1)
    rec = MixDynamics.apply(alpha, base)
    offs, views, o = [], [], 0
    for mt in mats:
        offs.append(o)
        views.append(slot_view(rec, o, mt.shape[1], mt.shape[2]))
        o += mt.shape[1] * mt.shape[2]
    return rec, offs, views


# ------------------------------------------------------------------------------------------------
# parameter gradients of the recurrences and heads (csrc/rnn_wgrad.h), linear heads (csrc/small_linear.h)
# ------------------------------------------------------------------------------------------------
def rnn_wgrad(ref, problems):
    """Up to four reductions G = D^T [h_shifted | x | 1] over the (sequence, step) rows in one pair of launches.
    problems: dicts with d [N,R]; optional h (2-D view, unit column stride) with `shift` and `T`; optional x [N,I]; `bias`.
    Returns one (g_wh [R,H] | None, g_wx [R,I] | None, g_b [R] | None) per problem."""
    lib = N.lib_for(ref)
    arr = (N.WgradProblem * len(problems))()
    outs, keep = [], []
    for slot, pr in zip(arr, problems):
        d, h, x = pr["d"], pr.get("h"), pr.get("x")
        n_rows, R = d.shape
        assert d.stride(1) == 1 and (h is None or h.stride(1) == 1) and (x is None or x.stride(1) == 1)
        H, I, bias = (h.shape[1] if h is not None else 0), (x.shape[1] if x is not None else 0), int(bool(pr.get("bias", True)))
        g_wh = _empty(d.device, R, H) if H else None
        g_wx = _empty(d.device, R, I) if I else None
        g_b = _empty(d.device, R) if bias else None
        slot.d, slot.h, slot.x = d.data_ptr(), (h.data_ptr() if H else None), (x.data_ptr() if I else None)
        slot.g_wh, slot.g_wx, slot.g_b = (t.data_ptr() if t is not None else None for t in (g_wh, g_wx, g_b))
        slot.d_stride, slot.h_stride, slot.x_stride = d.stride(0), (h.stride(0) if H else 0), (x.stride(0) if I else 0)
        slot.N, slot.R, slot.H, slot.I, slot.bias = n_rows, R, H, I, bias
        slot.T, slot.shift = int(pr.get("T", 1)), int(pr.get("shift", 0))
        outs.append((g_wh, g_wx, g_b))
        keep += [d, h, x]
    ws = _empty(ref.device, int(lib.dll.kvae_rnn_wgrad_ws_floats(arr, len(problems))))
    lib.check(N.timed("rnn_wgrad", ref, lambda: lib.dll.kvae_rnn_wgrad(arr, len(problems), N.ptr(ws), N.stream_for(ref))),
              "kvae_rnn_wgrad")
    return outs


def small_linear_supported(x, weight, softmax=False):
    O, F = weight.shape
    return (N.fused_ok(x) and x.dtype == torch.float32 and weight.dtype == torch.float32 and F <= 128 and O * F <= 12288
            and (not softmax or O <= 16) and x.shape[-1] == F and x.stride(-1) == 1
            and (x.dim() == 2 or x.is_contiguous()))


class SmallLinear(torch.autograd.Function):
    """y = x W^T + b (optionally followed by a softmax over the outputs) for the heads of the alpha-networks
    (reference dyn_param.py:53-56: head_w + softmax; switch_dyn_param.py:119-129: linear_head / init_head): one launch
    forward, one for the input gradient, and the rnn_wgrad reduction for dW | db - instead of addmm / softmax / two GEMMs /
    a column sum from the BLAS library.  x: [..., F] contiguous, or a 2-D view with unit column stride (h_seq[:, 0])."""

    @staticmethod
    def forward(ctx, x, weight, bias, softmax):
        w, b = _f32c(weight), _f32c(bias)
        O, F = w.shape
        x2 = x if x.dim() == 2 else x.reshape(-1, F)
        y = _empty(x.device, x2.shape[0], O)
        lib = N.lib_for(x)
        lib.check(N.timed("linear_fwd", x, lambda: lib.dll.kvae_linear_fwd(
            N.ptr(x2), x2.stride(0), x2.shape[0], F, N.ptr(w), N.ptr(b), O, int(softmax), N.ptr(y), N.stream_for(x))), "kvae_linear_fwd")
        ctx.softmax, ctx.lead = bool(softmax), x.shape[:-1]
        ctx.save_for_backward(x2, w, y if softmax else None)
        return y.reshape(*x.shape[:-1], O)

    @staticmethod
    def backward(ctx, g):
        x2, w, y = ctx.saved_tensors
        O, F = w.shape
        g2 = _f32c(g).reshape(-1, O)
        lib = N.lib_for(g2)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = gl = None
        if need_x or ctx.softmax:
            dx = _empty(g2.device, x2.shape[0], F)
            gl = torch.empty_like(g2) if ctx.softmax else None
            lib.check(N.timed("linear_bwd", g2, lambda: lib.dll.kvae_linear_bwd_input(
                N.ptr(g2), N.ptr(y), x2.shape[0], F, N.ptr(w), O, N.ptr(gl), N.ptr(dx), F, N.stream_for(g2))), "kvae_linear_bwd_input")
        g_w = g_b = None
        if need_w or need_b:
            (g_w, _, g_b), = rnn_wgrad(g2, [dict(d=gl if ctx.softmax else g2, h=x2, bias=True)])
        return (dx.reshape(*ctx.lead, F) if need_x else None), g_w, g_b, None


def small_linear(x, linear, softmax=False):
    """nn.Linear `linear` (+ softmax) through SmallLinear when the shapes fit the kernels, else through torch."""
    if small_linear_supported(x, linear.weight, softmax):
        return SmallLinear.apply(x, linear.weight, linear.bias, softmax)
    y = linear(x)
    return torch.softmax(y, dim=-1) if softmax else y


# ------------------------------------------------------------------------------------------------
# alpha-network LSTM
# ------------------------------------------------------------------------------------------------
class LstmSequence(torch.autograd.Function):
    """h_seq = LSTM(x) from a zero state (single layer, batch_first, torch gate order): the HIP replacement
    for stepping nn.LSTM T times (reference dyn_param.py:50-52).  Backward: one BPTT launch + the rnn_wgrad reduction."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh):
        x, w_ih, w_hh, b_ih, b_hh = (_f32c(t) for t in (x, w_ih, w_hh, b_ih, b_hh))
        Bsz, T, I = x.shape
        H = w_hh.shape[1]
        h, gates, c = _empty(x.device, Bsz, T, H), _empty(x.device, Bsz, T, 4 * H), _empty(x.device, Bsz, T, H)
        lib = N.lib_for(x)
        lib.check(N.timed("lstm_fwd", x, lambda: lib.dll.kvae_lstm_fwd(
            N.ptr(x), N.ptr(w_ih), N.ptr(w_hh), N.ptr(b_ih), N.ptr(b_hh), N.ptr(h), N.ptr(gates), N.ptr(c),
            Bsz, T, I, H, N.stream_for(x))), "kvae_lstm_fwd")
        ctx.save_for_backward(x, w_ih, w_hh, h, gates, c)
        return h

    @staticmethod
    def backward(ctx, g_h):
        x, w_ih, w_hh, h, gates, c = ctx.saved_tensors
        g_h = _f32c(g_h)
        Bsz, T, I = x.shape
        H = w_hh.shape[1]
        d_pre = _empty(x.device, Bsz, T, 4 * H)
        dx = torch.empty_like(x)
        lib = N.lib_for(x)
        lib.check(N.timed("lstm_bwd", x, lambda: lib.dll.kvae_lstm_bwd(
            N.ptr(g_h), N.ptr(gates), N.ptr(c), N.ptr(w_ih), N.ptr(w_hh), N.ptr(d_pre), N.ptr(dx),
            Bsz, T, I, H, N.stream_for(x))), "kvae_lstm_bwd")
        if not any(ctx.needs_input_grad[1:]):   # frozen alpha-network ("vae" / "warmup" phase): the input gradient only
            return dx, None, None, None, None
        (g_whh, g_wih, g_b), = rnn_wgrad(x, [dict(d=d_pre.reshape(Bsz * T, 4 * H), h=h.reshape(Bsz * T, H), shift=-1, T=T,
                                                  x=x.reshape(Bsz * T, I))])
        return dx, g_wih, g_whh, g_b, g_b


# ------------------------------------------------------------------------------------------------
# regime chain of the switching dynamics
# ------------------------------------------------------------------------------------------------
class RegimeChain(torch.autograd.Function):
    """(y_seq, log_q, log_p) of the Gumbel-softmax Markov chain (reference switch_dyn_param.py:52-79): one
    launch forward, one BPTT launch backward instead of T-1 Python iterations of ~10 aten ops."""

    @staticmethod
    def forward(ctx, logits, init_logits, gumbel, P, tau, hard):
        """`tau`: a float (baked into the launch) or a 0-d fp32 tensor on the logits' device, which the kernel reads
        at run time - the form that follows the reference's tau schedule (train.py:270-274) under hipGraph replay."""
        logits, init_logits, gumbel, P = (_f32c(t) for t in (logits, init_logits, gumbel, P))
        Bsz, T, K, _ = logits.shape
        y, lq, lp = _empty(logits.device, Bsz, T, K), _empty(logits.device, Bsz, T), _empty(logits.device, Bsz, T)
        lib = N.lib_for(logits)
        tau_t = tau if isinstance(tau, torch.Tensor) else None
        if tau_t is not None and (tau_t.device != logits.device or tau_t.dtype != torch.float32 or tau_t.numel() != 1):
            raise ValueError("RegimeChain: a tensor tau must be one fp32 element on the device of the logits")
        tau_f = 0.0 if tau_t is not None else float(tau)
        lib.check(N.timed("regime_fwd", logits, lambda: lib.dll.kvae_regime_fwd(
            N.ptr(logits), N.ptr(init_logits), N.ptr(gumbel), N.ptr(P), N.ptr(y), N.ptr(lq), N.ptr(lp), Bsz, T, K,
            tau_f, N.ptr(tau_t), int(hard), N.stream_for(logits))), "kvae_regime_fwd")
        ctx.tau, ctx.tau_t = tau_f, tau_t
        ctx.save_for_backward(logits, init_logits, gumbel, P, y)
        return y, lq, lp

    @staticmethod
    def backward(ctx, g_y, g_lq, g_lp):
        logits, init_logits, gumbel, P, y = ctx.saved_tensors
        Bsz, T, K, _ = logits.shape
        z = lambda t, *s: _f32c(t) if t is not None else torch.zeros(*s, device=logits.device, dtype=torch.float32)
        g_y, g_lq, g_lp = z(g_y, Bsz, T, K), z(g_lq, Bsz, T), z(g_lp, Bsz, T)
        g_logits, g_init = torch.empty_like(logits), torch.empty_like(init_logits)
        lib = N.lib_for(logits)
        lib.check(N.timed("regime_bwd", logits, lambda: lib.dll.kvae_regime_bwd(
            N.ptr(logits), N.ptr(init_logits), N.ptr(gumbel), N.ptr(P), N.ptr(y), N.ptr(g_y), N.ptr(g_lq), N.ptr(g_lp),
            N.ptr(g_logits), N.ptr(g_init), Bsz, T, K, ctx.tau, N.ptr(ctx.tau_t), N.stream_for(logits))), "kvae_regime_bwd")
        return g_logits, g_init, None, None, None, None


def regime_decode_supported(K, ref=None):
    """Shapes / dtypes kvae_regime_decode is built for (include/kvae_lgssm.h: fp32, K <= 16); the rest takes regime_decode_torch.
    The device is not asked about: fp32 host tensors go to the kernel's binding, which raises (kvae._native.lib_for)."""
    if ref is not None and ref.dtype != torch.float32:
        return False
    return 1 <= K <= N.KVAE_MAX_K


def regime_decode(logits, init_logits, P, want=_DECODE_OUTPUTS, impl=None):
    """Exact inference over the Markov regime posterior q(s_0) = softmax(init_logits), q(s_t | s_{t-1}) = row-softmax(logits[t])
    (semantics: include/kvae_lgssm.h, kvae_regime_decode).  logits [B,T,K,K] (slice 0 unused), init_logits
    [B,K], P [K,K] the prior's transition matrix.  want: which of "marginals", "path", "kl" to compute.  Returns a dict with
    marginals [B,T,K], path [B,T] (int64: the most likely regime sequence, lowest index on ties) and path_logq [B] (its log q),
    kl [B,T] (sum over t = KL(q || p)); entries not asked for are None.  One launch, no host synchronisation.
    impl: None = the HIP kernel where it is built (fp32, K <= 16), else regime_decode_torch; "kernel" / "torch" force one."""
    want = _want("regime_decode", _DECODE_OUTPUTS, want)
    Bsz, T, K, _ = logits.shape
    use_kernel = impl == "kernel" or (impl is None and regime_decode_supported(K, logits))
    if not use_kernel:
        return regime_decode_torch(logits, init_logits, P, want)
    dev = logits.device
    logits, init_logits, P = (_f32c(t.detach().to(dev)) for t in (logits, init_logits, P))
    marg = _empty(dev, Bsz, T, K) if "marginals" in want else None
    kl = _empty(dev, Bsz, T) if "kl" in want else None
    path = plq = ws = None
    lib = N.lib_for(logits)
    if "path" in want:
        path, plq = _empty(dev, Bsz, T, dt=torch.int32), _empty(dev, Bsz)
        ws = _empty(dev, (lib.dll.kvae_regime_decode_ws_bytes(Bsz, T, K) + 7) // 8, dt=torch.int64)   # 8-byte aligned
    lib.check(N.timed("regime_decode", logits, lambda: lib.dll.kvae_regime_decode(
        N.ptr(logits), N.ptr(init_logits), N.ptr(P), N.ptr(marg), N.ptr(path), N.ptr(plq), N.ptr(kl), N.ptr(ws), Bsz, T, K,
        N.stream_for(logits))), "kvae_regime_decode")
    return {"marginals": marg, "path": None if path is None else path.long(), "path_logq": plq, "kl": kl}


# ------------------------------------------------------------------------------------------------
# bidirectional GRU of the regime posterior
# ------------------------------------------------------------------------------------------------
def _ptr2(a, b):
    return (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())


class BiGruSequence(torch.autograd.Function):
    """h_seq [B,T,2H] = nn.GRU(bidirectional, batch_first)(x) from zero states (reference switch_dyn_param.py:118,123):
    one launch for both directions forward, one BPTT launch backward, all eight parameter gradients in one rnn_wgrad call."""
    SUPPORTED = (50, 2)   # (hidden, input): the shape csrc/gru_fast.h is instantiated for

    @staticmethod
    def forward(ctx, x, wi0, wh0, bi0, bh0, wi1, wh1, bi1, bh1):
        x = _f32c(x)
        ws = [_f32c(t) for t in (wi0, wh0, bi0, bh0, wi1, wh1, bi1, bh1)]
        Bsz, T, I = x.shape
        H = ws[1].shape[1]
        h = _empty(x.device, Bsz, T, 2 * H)
        gates = _empty(x.device, 2, Bsz, T, 4 * H)
        lib = N.lib_for(x)
        lib.check(N.timed("bigru_fwd", x, lambda: lib.dll.kvae_bigru_fwd(
            N.ptr(x), _ptr2(ws[0], ws[4]), _ptr2(ws[1], ws[5]), _ptr2(ws[2], ws[6]), _ptr2(ws[3], ws[7]), N.ptr(h),
            N.ptr(gates), Bsz, T, I, H, N.stream_for(x))), "kvae_bigru_fwd")
        ctx.save_for_backward(x, ws[0], ws[1], ws[4], ws[5], h, gates)
        return h

    @staticmethod
    def backward(ctx, g_h):
        x, wi0, wh0, wi1, wh1, h, gates = ctx.saved_tensors
        g_h = _f32c(g_h)
        Bsz, T, I = x.shape
        H = wh0.shape[1]
        dpi, dph, dx = _empty(x.device, 2, Bsz, T, 3 * H), _empty(x.device, 2, Bsz, T, 3 * H), _empty(x.device, 2, Bsz, T, I)
        lib = N.lib_for(x)
        lib.check(N.timed("bigru_bwd", x, lambda: lib.dll.kvae_bigru_bwd(
            N.ptr(g_h), N.ptr(gates), N.ptr(h), _ptr2(wi0, wi1), _ptr2(wh0, wh1), N.ptr(dpi), N.ptr(dph), N.ptr(dx),
            Bsz, T, I, H, N.stream_for(x))), "kvae_bigru_bwd")
        if not any(ctx.needs_input_grad[1:]):   # frozen regime posterior: the input gradient only
            return (dx.sum(0),) + (None,) * 8
        x2, h2 = x.reshape(Bsz * T, I), h.reshape(Bsz * T, 2 * H)
        probs = []
        for d in (0, 1):   # h_prev of the forward direction is h_{t-1}, of the reverse direction h_{t+1}
            probs.append(dict(d=dpi[d].reshape(Bsz * T, 3 * H), x=x2))
            probs.append(dict(d=dph[d].reshape(Bsz * T, 3 * H), h=h2[:, d * H:(d + 1) * H], shift=-1 if d == 0 else 1, T=T))
        res = rnn_wgrad(x, probs)
        out = [dx.sum(0)]
        for d in (0, 1):
            (_, g_wih, g_bih), (g_whh, _, g_bhh) = res[2 * d], res[2 * d + 1]
            out += [g_wih, g_whh, g_bih, g_bhh]
        return tuple(out)


# ------------------------------------------------------------------------------------------------
# masked sequences with the LSTM alpha-network: the network runs INSIDE the filter kernel, forward and backward
# ------------------------------------------------------------------------------------------------
ALPHA_LSTM_SUPPORTED = dict(hidden=50, p=2, max_K=16)


def alpha_lstm_supported(Y, lstm, K):
    """Shapes csrc/kvae_lgssm_wide.hip instantiates the in-kernel alpha-network for (KVAEConfig defaults)."""
    return (Y.is_cuda and K > 1 and K <= ALPHA_LSTM_SUPPORTED["max_K"] and lstm.hidden_size == ALPHA_LSTM_SUPPORTED["hidden"]
            and Y.shape[-1] == ALPHA_LSTM_SUPPORTED["p"] and lstm.input_size == Y.shape[-1])


class AlphaLstmSmooth(torch.autograd.Function):
    """Kalman filter (+ RTS smoother) whose per-step alpha comes from an LSTM fed with y_{t-1}, or with C mu_{t|t-1} on
    hidden frames (reference kalman_filter.py:151-185 + dyn_param.py:39-63): ONE launch forward (+ one for the smoother),
    ONE launch backward - the coupled adjoint of filter and cell (kvae_lgssm_alpha_lstm_bwd) - instead of T cell steps
    and T single-step filter launches each way.  Returns (ms, Ss,) mf, Sf, mp, Sp, record [B,T,A|B|C], alpha [B,T,K]."""

    @staticmethod
    def forward(ctx, Y, U, mask, w_ih, w_hh, b_ih, b_hh, head_w, head_b, A, Bm, Cm, Q, R, mu0, Sigma0, with_rts, keep_cell=False):
        """keep_cell (addition): also return the cell's h_seq, c_seq [B,T,H] - the hand-over KVAE.generate needs - even
        when nothing is differentiated."""
        Y, U, mask = _f32c(Y), _f32c(U), _f32c(mask)
        ws_ = [_f32c(t.detach()) for t in (w_ih, w_hh, b_ih, b_hh, head_w, head_b, A, Bm, Cm)]
        Bsz, T, p = Y.shape
        K, n, m = A.shape[0], A.shape[1], Bm.shape[2]
        H = w_hh.shape[1]
        slots, E = alpha_lstm_slots(n, m, p)
        dev = Y.device
        mf, Sf, mp, Sp = _empty(dev, Bsz, T, n), _empty(dev, Bsz, T, n, n), _empty(dev, Bsz, T, n), _empty(dev, Bsz, T, n, n)
        record, alpha = _empty(dev, Bsz, T, E), _empty(dev, Bsz, T, K)
        need = any(ctx.needs_input_grad)
        gates, c_seq, h_seq, x_seq = ((_empty(dev, Bsz, T, 4 * H), _empty(dev, Bsz, T, H), _empty(dev, Bsz, T, H), _empty(dev, Bsz, T, p))
                                      if need else (None,) * 4)
        if keep_cell and not need:
            c_seq, h_seq = _empty(dev, Bsz, T, H), _empty(dev, Bsz, T, H)
        call = _Call(Y, U, mask, record, None, None, None, Q, R, mu0, Sigma0, slots)
        ms, Ss = (_empty(dev, Bsz, T, n), _empty(dev, Bsz, T, n, n)) if with_rts else (None, None)
        st = _states(mf, Sf, mp, Sp, ms, Ss)
        call.lib.check(N.timed("alpha_lstm_fwd", Y, lambda: call.lib.dll.kvae_lgssm_filter_alpha_lstm(
            C.byref(call.prob), C.byref(st), *[N.ptr(w) for w in ws_], K, H, N.ptr(record), N.ptr(alpha), N.ptr(gates),
            N.ptr(c_seq), N.ptr(h_seq), N.ptr(x_seq), call.stream)), "kvae_lgssm_filter_alpha_lstm")
        if with_rts:
            call.lib.check(call.lib.dll.kvae_lgssm_rts_fwd(C.byref(call.prob), C.byref(st), call.stream), "kvae_lgssm_rts_fwd")
        ctx.with_rts, ctx.slots, ctx.keep_cell = with_rts, slots, keep_cell
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(Y, U, mask, *ws_, Q, R, mu0, Sigma0, mf, Sf, mp, Sp, ms, Ss, record, alpha, gates, c_seq, h_seq, x_seq)
        return ((ms, Ss) if with_rts else ()) + (mf, Sf, mp, Sp, record, alpha) + ((h_seq, c_seq) if keep_cell else ())

    @staticmethod
    def backward(ctx, *gouts):
        (Y, U, mask, w_ih, w_hh, b_ih, b_hh, head_w, head_b, A, Bm, Cm, Q, R, mu0, Sigma0, mf, Sf, mp, Sp, ms, Ss, record, alpha,
         gates, c_seq, h_seq, x_seq) = ctx.saved_tensors
        with_rts, slots = ctx.with_rts, ctx.slots
        if ctx.keep_cell:   # h_seq / c_seq are read-outs: no gradient flows back through them
            gouts = gouts[:-2]
        if with_rts:
            g_ms, g_Ss, g_mf, g_Sf, g_mp, g_Sp, g_rec, g_alpha = (_f32c(g) for g in gouts)
        else:
            g_mf, g_Sf, g_mp, g_Sp, g_rec, g_alpha = (_f32c(g) for g in gouts)
            g_ms = g_Ss = None
        call = _Call(Y, U, mask, record, None, None, None, Q, R, mu0, Sigma0, slots)
        Bsz, T, n, m, p = call.dims
        K, H = A.shape[0], w_hh.shape[1]
        dev = Y.device
        need = ctx.needs_input_grad
        sink = _GradSink(call, record, None, None, None, Q, slots, False, need[14], need[15])   # gA|gB|gC land in one g_record buffer
        ws, d_pre, g_logit = _empty(dev, Bsz, T, 2 * (n + n * n)), _empty(dev, Bsz, T, 4 * H), _empty(dev, Bsz, T, K)
        saved = _states(mf, Sf, mp, Sp, ms, Ss)
        up = _states(g_mf, g_Sf, g_mp, g_Sp, g_ms, g_Ss)
        call.lib.check(N.timed("alpha_lstm_bwd", Y, lambda: call.lib.dll.kvae_lgssm_alpha_lstm_bwd(
            C.byref(call.prob), C.byref(saved), C.byref(up), C.byref(sink.g), N.ptr(ws), int(with_rts), N.ptr(w_ih), N.ptr(w_hh),
            N.ptr(head_w), N.ptr(A), N.ptr(Bm), N.ptr(Cm), K, H, N.ptr(alpha), N.ptr(gates), N.ptr(c_seq), N.ptr(g_rec),
            N.ptr(g_alpha), N.ptr(sink.gpacked), N.ptr(d_pre), N.ptr(g_logit), call.stream)), "kvae_lgssm_alpha_lstm_bwd")
        # parameter gradients: reductions over (b,t) of what the launch wrote (none for a frozen alpha-network)
        g_whh = g_wih = g_b = g_hw = g_hb = None
        if any(need[3:9]):
            h2 = h_seq.reshape(Bsz * T, H)
            (g_whh, g_wih, g_b), (g_hw, _, g_hb) = rnn_wgrad(Y, [
                dict(d=d_pre.reshape(Bsz * T, 4 * H), h=h2, shift=-1, T=T, x=x_seq.reshape(Bsz * T, p)),
                dict(d=g_logit.reshape(Bsz * T, K), h=h2)])
        _, g_base = _mix_bwd(alpha, torch.cat([t.reshape(K, -1) for t in (A, Bm, Cm)], dim=1), sink.gpacked)
        gA, gB, gC = g_base.split([n * n, n * m, p * n], dim=1)
        gA, gB, gC = (g.reshape(t.shape) if nd else None for g, t, nd in zip((gA, gB, gC), (A, Bm, Cm), need[9:12]))
        g0, S0 = sink.prior_grads()
        return (sink.gY if need[0] else None, sink.gU if need[1] else None, None, g_wih, g_whh, g_b, g_b, g_hw, g_hb,
                gA, gB, gC, None, None, g0, S0, None, None)


@torch.no_grad()
def emission_means(mus_smooth, mus_filt, C_view, packed=None, c_off=None):
    """(C_t mu_t|T, C_t mu_t|t) [B,T,p] in one launch (reference model.py:279-288).  C_view: the [B,T,p,n] emission stack the
    caller holds (may be an expanded [p,n] or a slice of the packed step record `packed` at float offset `c_off`)."""
    ms, mf = _f32c(mus_smooth.squeeze(-1)), _f32c(mus_filt.squeeze(-1))
    Bsz, T, n = ms.shape
    p = C_view.shape[-2]
    prob = N.Problem()
    prob.B, prob.T, prob.n, prob.m, prob.p = Bsz, T, n, n, p
    keep, prob.C = _stack(C_view, Bsz, T, p, n, packed, c_off)
    a_s, a_f = _empty(ms.device, Bsz, T, p), _empty(ms.device, Bsz, T, p)
    lib = N.lib_for(ms)
    lib.check(lib.dll.kvae_lgssm_emission_means(C.byref(prob), N.ptr(ms), N.ptr(mf), N.ptr(a_s), N.ptr(a_f), N.stream_for(ms)),
              "kvae_lgssm_emission_means")
    return a_s, a_f


@torch.no_grad()
def rts_only(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots, mf, Sf, mp, Sp):
    """RTS smoother over already-filtered beliefs (kvae_lgssm_rts_fwd); no autograd."""
    call = _Call(Y, U, mask, packed, A, Bm, Cm, Q, R, mu0, Sigma0, slots)
    ms, Ss = torch.empty_like(mf), torch.empty_like(Sf)
    st = _states(mf, Sf, mp, Sp, ms, Ss)
    call.lib.check(call.lib.dll.kvae_lgssm_rts_fwd(C.byref(call.prob), C.byref(st), call.stream), "kvae_lgssm_rts_fwd")
    return ms, Ss


# ------------------------------------------------------------------------------------------------
# generation: the closed-loop rollout of KVAE.generate (kvae_lgssm_generate, csrc/lgssm_gen.h)
# ------------------------------------------------------------------------------------------------
GEN_LSTM = dict(hidden=50, p=2)   # the alpha-network shape csrc/lgssm_gen.h holds in LDS


def rollout_supported(kind, K, n, m, p, hidden=None, ref=None):
    """Shapes kvae_lgssm_generate is built for (include/kvae_lgssm.h); every other one takes rollout_torch."""
    if ref is not None and not (N.fused_ok(ref) and ref.dtype == torch.float32):
        return False
    if not all(1 <= d <= N.KVAE_MAX_DIM for d in (n, m, p)) or not 1 <= K <= N.KVAE_MAX_K:
        return False
    return kind == "switching" or K == 1 or (hidden == GEN_LSTM["hidden"] and p == GEN_LSTM["p"])


def rollout(kind, A, Bm, Cm, mu, L0, U, LQ, LR, S, H, lstm=None, h0=None, c0=None, y0=None, P=None, s0=None,
            eps0=None, eps_z=None, eps_a=None, gumbel=None, impl=None):
    """Closed-loop rollout of the learned dynamics for R = B*S rollouts and H steps (semantics: include/kvae_lgssm.h,
    kvae_lgssm_generate).  kind "lstm" | "switching"; A [K,n,n], Bm [K,n,m], Cm [K,p,n]; mu [B,n];
    L0 [B,n,n]; U [B,H,m] or None; LQ [n,n] (lstm) / [K,n,n] (switching); LR [p,p]; lstm = (w_ih, w_hh, b_ih, b_hh, head_w,
    head_b) with h0, c0 [B,hidden], y0 [B,p] (K > 1); P [K,K], s0 [B,K] (switching).  Noise tensors [B,S,(H,)d] or None.
    impl: None = the HIP kernel where the shape is built, else the torch recursion; "kernel" / "torch" force one.
    Returns a [B,S,H,p], z [B,S,H,n], weights [B,S,H,K]."""
    K, n, m, p = A.shape[0], A.shape[1], Bm.shape[2], Cm.shape[1]
    hidden = lstm[1].shape[1] if lstm is not None else None
    use_kernel = impl == "kernel" or (impl is None and rollout_supported(kind, K, n, m, p, hidden, mu))
    if not use_kernel:
        return rollout_torch(kind, A, Bm, Cm, mu, L0, U, LQ, LR, S, H, lstm, h0, c0, y0, P, s0, eps0, eps_z, eps_a, gumbel)
    Bsz = mu.shape[0]
    dev = mu.device
    a, z, w = _empty(dev, Bsz, S, H, p), _empty(dev, Bsz, S, H, n), _empty(dev, Bsz, S, H, K)
    keep = {}
    pr = N.GenProblem()
    pr.B, pr.S, pr.H, pr.n, pr.m, pr.p, pr.K = Bsz, S, H, n, m, p, K
    pr.kind = 1 if kind == "switching" else 0
    pr.hidden = hidden or 0
    named = dict(A=A, Bm=Bm, C=Cm, LQ=LQ, LR=LR, mu=mu, L0=L0, U=U, P=P, s0=s0, h0=h0, c0=c0, y0=y0,
                 eps0=eps0, eps_z=eps_z, eps_a=eps_a, gumbel=gumbel)
    if lstm is not None:
        named.update(zip(("w_ih", "w_hh", "b_ih", "b_hh", "head_w", "head_b"), lstm))
    for k, t in named.items():
        if t is not None:
            keep[k] = _f32c(t.detach().to(dev))
            setattr(pr, k, keep[k].data_ptr())
    pr.a_out, pr.z_out, pr.w_out = a.data_ptr(), z.data_ptr(), w.data_ptr()
    lib = N.lib_for(mu)
    lib.check(N.timed("generate", mu, lambda: lib.dll.kvae_lgssm_generate(C.byref(pr), N.stream_for(mu))), "kvae_lgssm_generate")
    return a, z, w


# ------------------------------------------------------------------------------------------------
# joint posterior samples of latent paths (kvae_lgssm_posterior_sample, csrc/lgssm_post.h)
# ------------------------------------------------------------------------------------------------
def posterior_supported(n, p, ref=None):
    """Shapes / tensors kvae_lgssm_posterior_sample is built for (include/kvae_lgssm.h); the rest takes posterior_paths_torch."""
    if ref is not None and not (N.fused_ok(ref) and ref.dtype == torch.float32):
        return False
    return all(1 <= d <= N.KVAE_MAX_DIM for d in (n, p))


def posterior_paths(mus_filt, Sigmas_filt, mus_pred, Sigmas_pred, A, Cm, Q, S, LR=None, eps=None, eta=None, packed=None,
                    slots=Slots(), impl=None):
    """S joint samples z_{0:T-1} per sequence from the smoothing posterior, by backward sampling over the filter's outputs
    (semantics: include/kvae_lgssm.h, kvae_lgssm_posterior_sample).  mus_* [B,T,n] (or [B,T,n,1]),
    Sigmas_* [B,T,n,n]; A [n,n] | [B,T,n,n], Cm [p,n] | [B,T,p,n], Q [n,n] | [B,T,n,n], or slots of the packed step record
    `packed` [B,T,E] at the float offsets `slots` (then A and Q are ignored; Cm is still read for p); LR [p,p] (with eta); eps [B,S,T,n],
    eta [B,S,T,p] or None.  impl: None = the HIP kernels where built, else the torch recursion; "kernel" / "torch" force one.
    Returns z [B,S,T,n], a [B,S,T,p], levels [B,T] (int32: the ladder level of chol(P_t), 5 = clamped diagonal)."""
    n = Sigmas_filt.shape[-1]
    Bsz, T = Sigmas_filt.shape[:2]
    p = Cm.shape[-2]   # Cm is always given (a view of the record when packed): it carries p
    use_kernel = impl == "kernel" or (impl is None and posterior_supported(n, p, Sigmas_filt))
    if not use_kernel:
        if packed is not None:
            pick = lambda t, off, r, c: t if off is None else slot_view(packed, off, r, c)
            A, Cm, Q = pick(A, slots.A, n, n), pick(Cm, slots.C, p, n), pick(Q, slots.Q, n, n)
        return posterior_paths_torch(mus_filt, Sigmas_filt, mus_pred, Sigmas_pred, A, Cm, Q, S, LR, eps, eta)
    call = PosteriorCall(mus_filt, Sigmas_filt, mus_pred, Sigmas_pred, A, Cm, Q, S, LR, eps, eta, packed, slots)
    call.run()
    return call.z, call.a, call.levels


class PosteriorCall:
    """The kvae_psample_problem of one posterior_paths call with its outputs and workspace, every tensor kept alive.  run(stages)
    runs the whole call (0) or a part: GAINS once, then PATHS (paths + emission) any number of times over the same workspace (new_draws)."""
    GAINS, PATHS = 1, 2

    def __init__(self, mus_filt, Sigmas_filt, mus_pred, Sigmas_pred, A, Cm, Q, S, LR=None, eps=None, eta=None, packed=None,
                 slots=Slots()):
        n, p = Sigmas_filt.shape[-1], Cm.shape[-2]
        Bsz, T = Sigmas_filt.shape[:2]
        dev = Sigmas_filt.device
        sq = lambda t: _f32c((t.squeeze(-1) if t.dim() == 4 else t).detach())
        mf, mp, Sf, Sp = sq(mus_filt), sq(mus_pred), _f32c(Sigmas_filt.detach()), _f32c(Sigmas_pred.detach())
        packed = _f32c(packed.detach()) if packed is not None else None
        pr = N.PsampleProblem()
        pr.B, pr.S, pr.T, pr.n, pr.p = Bsz, S, T, n, p
        pr.mus_filt, pr.Sigmas_filt, pr.mus_pred, pr.Sigmas_pred = mf.data_ptr(), Sf.data_ptr(), mp.data_ptr(), Sp.data_ptr()
        self.keep = [mf, mp, Sf, Sp, packed]
        for name, t, r, c, off in (("A", A, n, n, slots.A), ("C", Cm, p, n, slots.C), ("Q", Q, n, n, slots.Q)):
            k, st = _stack(t.detach() if (off is None and t is not None) else t, Bsz, T, r, c, packed, off)
            self.keep.append(k)
            setattr(pr, name, st)
        self.pr, self.dev, self.ref = pr, dev, Sf
        self.new_draws(LR=LR, eps=eps, eta=eta)
        self.z, self.a, self.levels = _empty(dev, Bsz, S, T, n), _empty(dev, Bsz, S, T, p), _empty(dev, Bsz, T, dt=torch.int32)
        self.lib = N.lib_for(Sf)
        self.ws = _empty(dev, int(self.lib.dll.kvae_lgssm_posterior_sample_ws_floats(C.byref(pr))))
        pr.z_out, pr.a_out, pr.levels_out, pr.ws = self.z.data_ptr(), self.a.data_ptr(), self.levels.data_ptr(), self.ws.data_ptr()

    def new_draws(self, LR=None, eps=None, eta=None):
        self.noise = {}
        for name, t in (("LR", LR), ("eps", eps), ("eta", eta)):
            self.noise[name] = _f32c(t.detach().to(self.dev)) if t is not None else None
            setattr(self.pr, name, self.noise[name].data_ptr() if t is not None else None)

    def run(self, stages=0):
        self.pr.stages = stages
        name = {0: "posterior_sample", 1: "posterior_gains", 2: "posterior_paths"}.get(stages, "posterior_sample")
        self.lib.check(N.timed(name, self.ref, lambda: self.lib.dll.kvae_lgssm_posterior_sample(C.byref(self.pr), N.stream_for(self.ref))),
                       "kvae_lgssm_posterior_sample")


# ------------------------------------------------------------------------------------------------
# predictive density of the latents (kvae_lgssm_predictive, csrc/lgssm_pred.h)
# ------------------------------------------------------------------------------------------------
def predictive_supported(n, p, ref=None):
    """Shapes / tensors kvae_lgssm_predictive is built for (include/kvae_lgssm.h: fp32, p == 2, n <= 16); the rest takes
    predictive_torch."""
    if ref is not None and not (N.fused_ok(ref) and ref.dtype == torch.float32):
        return False
    return p == 2 and 1 <= n <= N.KVAE_MAX_DIM


def _pred_problem(mp, Sp, Cm, packed, R, Y, mask, slots):
    """(kvae_pred_problem, tensors to keep alive) over contiguous fp32 inputs; the output pointers are left NULL."""
    Bsz, T, n = mp.shape
    p = Y.shape[-1]
    pr = N.PredProblem()
    pr.B, pr.T, pr.n, pr.p = Bsz, T, n, p
    keep, pr.C = _stack(Cm, Bsz, T, p, n, packed, slots.C)
    return pr, _bind(pr, dict(mus_pred=mp, Sigmas_pred=Sp, R=R, y=Y, mask=mask)) + (keep,)


@torch.no_grad()
def predictive(mus_pred, Sigmas_pred, Cm, R, Y, mask=None, packed=None, slots=Slots(), want=_PRED_OUTPUTS, impl=None):
    """log p(a_t | a_{0:t-1}, u) of every step from the filter's one-step-ahead beliefs (semantics: include/kvae_lgssm.h,
    kvae_lgssm_predictive).  mus_pred [B,T,n] (or [B,T,n,1]), Sigmas_pred [B,T,n,n]; Cm [p,n] | [B,T,p,n],
    or the C slot of the packed step record `packed` [B,T,E] at the float offset slots.C (Cm is still read for p); R [p,p];
    Y [B,T,p]; mask [B,T] (1 = observed) or None.  want: which of "ll", "nis", "a_pred", "S", "levels", "seq_ll" to compute.
    Returns a dict: ll [B,T], nis [B,T] (both 0 on hidden steps), a_pred [B,T,p], S [B,T,p,p], levels [B,T] (int32: the ladder
    level of chol(S_t), 5 = clamped diagonal), seq_ll [B] = sum_t ll; entries not asked for are None.  Two launches, no host
    synchronisation.  impl: None = the HIP kernels where built (fp32, p == 2), else predictive_torch; "kernel" / "torch" force one."""
    want = _want("predictive", _PRED_OUTPUTS, want)
    n = Sigmas_pred.shape[-1]
    Bsz, T = Sigmas_pred.shape[:2]
    p = Cm.shape[-2]
    use_kernel = impl == "kernel" or (impl is None and predictive_supported(n, p, Sigmas_pred))
    if not use_kernel:
        if packed is not None and slots.C is not None:
            Cm = slot_view(packed, slots.C, p, n)
        return predictive_torch(mus_pred, Sigmas_pred, Cm, R, Y, mask, want)
    dev = Sigmas_pred.device
    mp = _f32c((mus_pred.squeeze(-1) if mus_pred.dim() == 4 else mus_pred).detach())
    Sp, R, Y = _f32c(Sigmas_pred.detach()), _f32c(R.detach().to(dev)), _f32c(Y.detach())
    mask = None if mask is None else _f32c(mask.detach().to(dev).reshape(Bsz, T))
    packed = _f32c(packed.detach()) if packed is not None else None
    pr, keep = _pred_problem(mp, Sp, Cm.detach() if slots.C is None else Cm, packed, R, Y, mask, slots)
    out = _wanted(dev, _PRED_OUTPUTS, want, dict(nis=(Bsz, T), a_pred=(Bsz, T, p), S=(Bsz, T, p, p), levels=(Bsz, T), seq_ll=(Bsz,)))
    ll = _read_by(dev, out, "ll", ("seq_ll",), want, (Bsz, T))
    _bind(pr, dict(ll=ll, nis=out["nis"], a_pred=out["a_pred"], S_out=out["S"], levels=out["levels"], seq_ll=out["seq_ll"]))
    lib = N.lib_for(Sp)
    lib.check(N.timed("predictive", Sp, lambda: lib.dll.kvae_lgssm_predictive(C.byref(pr), N.stream_for(Sp))), "kvae_lgssm_predictive")
    del keep
    return out


# ------------------------------------------------------------------------------------------------
# log p(a | u), differentiable (kvae_lgssm_predictive + kvae_lgssm_predictive_bwd, csrc/lgssm_pred.h)
# ------------------------------------------------------------------------------------------------
class PredictiveLogLik(torch.autograd.Function):
    """(ll [B,T], seq_ll [B], levels [B,T]) of kvae_lgssm_predictive with the adjoint kvae_lgssm_predictive_bwd: one call each
    way.  Gradients for mus_pred, Sigmas_pred, Cm (or `packed`: a zero-filled record with the C slot written) and Y; a shared
    2-D Cm is reduced over the items.  R is a buffer of the model: no gradient."""

    @staticmethod
    def forward(ctx, mus_pred, Sigmas_pred, Cm, packed, R, Y, mask, slots):
        mp, Sp, Rc, Yc, mk = _f32c(mus_pred), _f32c(Sigmas_pred), _f32c(R), _f32c(Y), _f32c(mask)
        pk = _f32c(packed)
        Bsz, T, _ = mp.shape
        dev = Sp.device
        pr, keep = _pred_problem(mp, Sp, Cm, pk, Rc, Yc, mk, slots)
        ll, seq, levels = _empty(dev, Bsz, T), _empty(dev, Bsz), _empty(dev, Bsz, T, dt=torch.int32)
        pr.ll, pr.seq_ll, pr.levels = ll.data_ptr(), seq.data_ptr(), levels.data_ptr()
        lib = N.lib_for(Sp)
        lib.check(N.timed("predictive", Sp, lambda: lib.dll.kvae_lgssm_predictive(C.byref(pr), N.stream_for(Sp))), "kvae_lgssm_predictive")
        del keep
        ctx.slots = slots
        ctx.mark_non_differentiable(levels)
        ctx.set_materialize_grads(False)   # an output nobody differentiates arrives as None: NULL upstream, its loads skipped
        ctx.save_for_backward(mus_pred, Sigmas_pred, Cm, packed, R, Y, mask)
        return ll, seq, levels

    @staticmethod
    def backward(ctx, g_ll, g_seq, _g_levels):
        if g_ll is None and g_seq is None:
            return (None,) * 8
        mus_pred, Sigmas_pred, Cm, packed, R, Y, mask = ctx.saved_tensors
        slots, need = ctx.slots, ctx.needs_input_grad
        mp, Sp, Rc, Yc, mk = _f32c(mus_pred), _f32c(Sigmas_pred), _f32c(R), _f32c(Y), _f32c(mask)
        pk = _f32c(packed)
        Bsz, T, n = mp.shape
        p = Yc.shape[-1]
        dev = Sp.device
        pr, keep = _pred_problem(mp, Sp, Cm, pk, Rc, Yc, mk, slots)
        g_ll, g_seq = _f32c(g_ll), _f32c(g_seq)
        g = N.PredGrads()
        g.g_ll, g.g_seq = N.ptr(g_ll), N.ptr(g_seq)
        g_mp = torch.empty_like(mp) if need[0] else None
        g_Sp = torch.empty_like(Sp) if need[1] else None
        gY = torch.empty_like(Yc) if need[5] else None
        g.g_mus_pred, g.g_Sigmas_pred, g.gY = N.ptr(g_mp), N.ptr(g_Sp), N.ptr(gY)
        g_packed = g_Cbuf = None
        if slots.C is not None:
            if need[3]:
                g_packed = torch.zeros_like(pk)
                E = pk.shape[-1]
                g.gC = N.Stack(g_packed.data_ptr() + 4 * slots.C, T * E, E)
        elif need[2]:
            g_Cbuf = _empty(dev, Bsz, T, p, n)
            g.gC = N.Stack(g_Cbuf.data_ptr(), T * p * n, p * n)
        lib = N.lib_for(Sp)
        lib.check(N.timed("predictive_bwd", Sp, lambda: lib.dll.kvae_lgssm_predictive_bwd(C.byref(pr), C.byref(g), N.stream_for(Sp))),
                  "kvae_lgssm_predictive_bwd")
        del keep
        gC = _reduce_to(g_Cbuf, Cm) if g_Cbuf is not None else None
        return (g_mp.reshape(mus_pred.shape) if g_mp is not None else None, g_Sp, gC, g_packed, None, gY, None, None)


def log_marginal(mus_pred, Sigmas_pred, Cm, R, Y, mask=None, packed=None, slots=Slots(), impl=None):
    """log p(a_t | a_{0:t-1}, u) of every step and its per-sequence sum log p(a | u), DIFFERENTIABLE w.r.t. mus_pred, Sigmas_pred,
    C (Cm, or the C slot of `packed`) and Y (predictive is the no-grad read-out with more outputs).  Arguments as predictive.
    Returns dict(ll [B,T], seq_ll [B], levels [B,T] int32).  Forward two launches, backward one (kvae_lgssm_predictive_bwd), no
    host synchronisation.  impl: None = the HIP kernels where built (fp32, p == 2), else log_marginal_torch; "kernel" / "torch"
    force one."""
    n = Sigmas_pred.shape[-1]
    Bsz, T = Sigmas_pred.shape[:2]
    p = Cm.shape[-2]
    use_kernel = impl == "kernel" or (impl is None and predictive_supported(n, p, Sigmas_pred))
    if not use_kernel:
        if packed is not None and slots.C is not None:
            Cm = slot_view(packed, slots.C, p, n)
        return log_marginal_torch(mus_pred, Sigmas_pred, Cm, R, Y, mask)
    dev = Sigmas_pred.device
    mp = mus_pred.squeeze(-1) if mus_pred.dim() == 4 else mus_pred
    mask = None if mask is None else mask.detach().to(dev).reshape(Bsz, T)
    ll, seq, levels = PredictiveLogLik.apply(mp, Sigmas_pred, Cm, packed if slots.C is not None else None, R.detach().to(dev), Y,
                                             mask, Slots(C=slots.C))
    return {"ll": ll, "seq_ll": seq, "levels": levels}


# ------------------------------------------------------------------------------------------------
# causal switching Kalman filter, GPB2 (kvae_lgssm_switching_filter, csrc/lgssm_swf.h)
# ------------------------------------------------------------------------------------------------
SWF_SUPPORTED = dict(max_K=8, max_n=4, max_m=4, p=2)


def switching_filter_supported(K, n, m, p, ref=None):
    """Shapes / tensors kvae_lgssm_switching_filter is built for (include/kvae_lgssm.h: fp32, K <= 8, n <= 4, m <= 4, p == 2, a HIP
    device - or the host simulation a test injected); the rest takes switching_filter_torch."""
    if ref is not None and not (N.fused_ok(ref) and ref.dtype == torch.float32):
        return False
    s = SWF_SUPPORTED
    return 1 <= K <= s["max_K"] and 1 <= n <= s["max_n"] and 1 <= m <= s["max_m"] and p == s["p"]


@torch.no_grad()
def switching_filter(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, want=_SWF_OUTPUTS, state=None, impl=None):
    """The causal switching Kalman filter with GPB2 collapse over the generative switching model (semantics: include/kvae_lgssm.h,
    kvae_lgssm_switching_filter).  A [K,n,n], Bm [K,n,m], Q [K,n,n] per regime; Cm [p,n], R [p,p] shared;
    P [K,K] the transition matrix (unclamped: a zero is an impossible transition); mu0 [n], Sigma0 [n,n]; Y [B,T,p]; U [B,T,m];
    mask [B,T] (1 = observed) or None.  state: None (s_0 uniform, every regime starts at (mu0, Sigma0)) or the "state" entry of an
    earlier call, which continues that stream.  want: which of "regime_filt", "regime_pred" [B,T,K], "log_lik" [B,T],
    "log_lik_seq" [B], "a_pred" [B,T,p], "S" [B,T,p,p], "mus_filt" [B,T,n], "Sigmas_filt" [B,T,n,n], "levels" [B,T] (int32),
    "state" (dict log_w [B,K], mu [B,K,n], Sigma [B,K,n,n] after the last step) to compute; entries not asked for are None.
    One launch for the sweep (one more for log_lik_seq), no host synchronisation, no gradients.
    impl: None = the HIP kernel where it is built (switching_filter_supported), else switching_filter_torch; "hip" / "torch" force one."""
    want = _want("switching_filter", _SWF_OUTPUTS, want)
    if not _sw_route("switching_filter", impl, switching_filter_supported, A, Bm, Y):
        return switching_filter_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, want)
    out, pr, keep = _swf_problem(N.SwfProblem(), A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, want)
    lib = N.lib_for(Y)
    lib.check(N.timed("switching_filter", Y, lambda: lib.dll.kvae_lgssm_switching_filter(C.byref(pr), N.stream_for(Y))),
              "kvae_lgssm_switching_filter")
    return out


def _check_impl(op, impl):
    if impl not in (None, "hip", "torch"):
        raise ValueError(f"{op}: impl must be None, 'hip' or 'torch', got {impl!r}")


def _sw_route(op, impl, supported, A, Bm, Y, particles=None, fp32_model=False):
    """The routing rule of the switching read-outs: True when the HIP kernel runs, False for the restatement in torch ops.  ValueError
    for an impl that is not None, "hip" or "torch" (_check_impl: the ops that check other arguments between the two errors call it
    ahead of them), and for impl="hip" on what the kernel is not built for: supported(K, n, m, p, [particles,] Y) is False, or -
    fp32_model - the model is not fp32."""
    _check_impl(op, impl)
    dims = (A.shape[0], A.shape[1], Bm.shape[2], Y.shape[2]) + (() if particles is None else (particles,))
    ok = supported(*dims, Y) and not (fp32_model and A.dtype != torch.float32)
    if impl == "hip" and not ok:
        s, pf = SWF_SUPPORTED, ("", "") if particles is None else (f", {SPF_PARTICLES} particles", f", {particles} particles")
        raise ValueError(f"{op}: impl='hip' needs fp32 tensors on a HIP device, K <= {s['max_K']}, n <= {s['max_n']}, m <= {s['max_m']}, "
                         f"p == {s['p']}{pf[0]}; got K = {dims[0]}, n = {dims[1]}, m = {dims[2]}, p = {dims[3]}{pf[1]}, "
                         f"{A.dtype} model and {Y.dtype} data on {Y.device}")
    return ok and impl != "torch"


_SW_OPERANDS = ("A", "Bm", "Q", "C", "R", "P", "mu0", "Sigma0", "y", "u")   # the fields kvae_swf_problem and kvae_spf_problem share


def _sw_operands(pr, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, **draws):
    """Bind the ten model / data operands, the particle filter's `draws` (by field name) and the mask [B,T] (None = NULL) to the
    problem `pr`, as contiguous fp32 tensors on Y's device: those tensors, which must outlive the call."""
    dev = Y.device
    named = {k: _f32c(t.detach().to(dev) if (t.requires_grad or t.device != dev) else t)   # (most arrive detached and in place)
             for k, t in zip(_SW_OPERANDS + tuple(draws), (A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, *draws.values()))}
    named["mask"] = None if mask is None else _f32c(mask.detach().to(dev).reshape(Y.shape[0], Y.shape[1]))
    return _bind(pr, named)


def _swf_problem(pr, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, want):
    """Fill the kvae_swf_problem `pr` for the outputs of _SWF_OUTPUTS named in `want`: (the dict of outputs, pr, the tensors pr
    points to, which must outlive the call)."""
    K, n, m = A.shape[0], A.shape[1], Bm.shape[2]
    Bsz, T, p = Y.shape
    dev = Y.device
    keep = _sw_operands(pr, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask)
    st = _swf_state(state, Bsz, K, n)
    if st is not None:
        st = _bind(pr, {"state_" + k: _f32c(t.detach().to(dev)) for k, t in zip(("log_w", "mu", "Sigma"), st)})
    out = _wanted(dev, _SWF_OUTPUTS, want, dict(regime_filt=(Bsz, T, K), regime_pred=(Bsz, T, K), log_lik_seq=(Bsz,), a_pred=(Bsz, T, p),
                                                S=(Bsz, T, p, p), mus_filt=(Bsz, T, n), Sigmas_filt=(Bsz, T, n, n), levels=(Bsz, T)))
    ll = _read_by(dev, out, "log_lik", ("log_lik_seq",), want, (Bsz, T))
    if "state" in want:
        out["state"] = {"log_w": _empty(dev, Bsz, K), "mu": _empty(dev, Bsz, K, n), "Sigma": _empty(dev, Bsz, K, n, n)}
        _bind(pr, {"out_" + k: t for k, t in out["state"].items()})
    pr.B, pr.T, pr.K, pr.n, pr.m, pr.p = Bsz, T, K, n, m, p
    _bind(pr, dict(regime_filt=out["regime_filt"], regime_pred=out["regime_pred"], ll=ll, seq_ll=out["log_lik_seq"], a_pred=out["a_pred"],
                   S_out=out["S"], mus_filt=out["mus_filt"], Sigmas_filt=out["Sigmas_filt"], levels=out["levels"]))
    return out, pr, keep + (st, ll)


# ------------------------------------------------------------------------------------------------
# Rao-Blackwellised particle filter of the switching model (kvae_lgssm_switching_pf, csrc/lgssm_spf.h)
# ------------------------------------------------------------------------------------------------
def switching_pf_supported(K, n, m, p, num_particles, ref=None):
    """Shapes / tensors kvae_lgssm_switching_pf is built for (include/kvae_lgssm.h: the switching filter's, and 64, 128 or 256
    particles per replicate); the rest takes switching_pf_torch."""
    return switching_filter_supported(K, n, m, p, ref) and num_particles in SPF_PARTICLES


@torch.no_grad()
def switching_pf(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, pf_regime, pf_resample, mask=None, ess_threshold=0.5, want=_SPF_OUTPUTS,
                 state=None, impl=None):
    """The Rao-Blackwellised particle filter of the generative switching model (semantics: include/kvae_lgssm.h,
    kvae_lgssm_switching_pf): the model and operands of switching_filter, without the GPB2 collapse - G
    replicate filters of N particles per sequence, each particle a regime history and an exact Kalman belief.  pf_regime [B,G,T,N]
    and pf_resample [B,G,T] are the uniform draws in [0,1) of the regimes and of the systematic resampling (G and N are their
    shape).  ess_threshold in [0,1]: 0 never resamples, 1 always, else when ess_t < ess_threshold N.  state: None or the "state"
    entry of an earlier call (log_w [B,G,N], regime [B,G,N] int32, mu [B,G,N,n], Sigma [B,G,N,n,n]), which - with the matching
    slices of the draws - continues that stream with the same bits.  want: which of "log_lik" [B,G,T] (its exp-sum over t is an
    unbiased estimate of p(a | u)), "log_lik_seq" [B,G], "regime_filt" [B,G,T,K], "mus_filt" [B,G,T,n], "Sigmas_filt" [B,G,T,n,n],
    "ess" [B,G,T], "resampled" [B,G,T] (bool), "regimes" / "ancestors" [B,G,T,N] (int32: the draw of slot i at step t before
    resampling; the slot it was copied from), "levels" [B,G,T] (int32), "paths" [B,G,N,T] (int32: the regime lineage of every final
    slot - joint draws of regime paths), "path_log_w" [B,G,N] (their final log weights), "state" to compute; entries not asked for
    are None.  At most three launches, no host synchronisation, no gradients.
    impl: None = the HIP kernel where it is built (switching_pf_supported), else switching_pf_torch; "hip" / "torch" force one."""
    want = _want("switching_pf", _SPF_OUTPUTS, want)
    _check_impl("switching_pf", impl)
    if not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError(f"switching_pf: ess_threshold must be in [0, 1], got {ess_threshold}")
    K, n, m = A.shape[0], A.shape[1], Bm.shape[2]
    Bsz, T, p = Y.shape
    G, Np = _spf_draws(pf_regime, pf_resample, Bsz, T)
    if not _sw_route("switching_pf", impl, switching_pf_supported, A, Bm, Y, particles=Np):
        return switching_pf_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, pf_regime, pf_resample, mask, ess_threshold, state, want)
    dev = Y.device
    pr = N.SpfProblem()
    pr.B, pr.G, pr.T, pr.K, pr.N, pr.n, pr.m, pr.p, pr.ess_threshold = Bsz, G, T, K, Np, n, m, p, float(ess_threshold)
    keep = _sw_operands(pr, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, pf_regime=pf_regime, pf_resample=pf_resample)
    st = _spf_state(state, Bsz, G, Np, n)
    if st is not None:
        st = _bind(pr, {"state_" + k: t.detach().to(device=dev, dtype=torch.int32).contiguous() if k == "regime" else _f32c(t.detach().to(dev))
                        for k, t in zip(("log_w", "regime", "mu", "Sigma"), st)})
    out = _wanted(dev, _SPF_OUTPUTS, want, dict(log_lik_seq=(Bsz, G), regime_filt=(Bsz, G, T, K), mus_filt=(Bsz, G, T, n),
                                                Sigmas_filt=(Bsz, G, T, n, n), ess=(Bsz, G, T), resampled=(Bsz, G, T), levels=(Bsz, G, T),
                                                paths=(Bsz, G, Np, T)))
    ll = _read_by(dev, out, "log_lik", ("log_lik_seq",), want, (Bsz, G, T))
    regimes, ancestors = (_read_by(dev, out, k, ("paths",), want, (Bsz, G, T, Np)) for k in ("regimes", "ancestors"))
    so = {}
    if "state" in want or "path_log_w" in want:   # the final log weights are both the state's and the lineages'
        so["log_w"] = _empty(dev, Bsz, G, Np)
        if "state" in want:
            so.update(regime=_empty(dev, Bsz, G, Np, dt=torch.int32), mu=_empty(dev, Bsz, G, Np, n), Sigma=_empty(dev, Bsz, G, Np, n, n))
            out["state"] = so
        if "path_log_w" in want:
            out["path_log_w"] = so["log_w"]
    _bind(pr, dict(ll=ll, seq_ll=out["log_lik_seq"], regime_filt=out["regime_filt"], mus_filt=out["mus_filt"], Sigmas_filt=out["Sigmas_filt"],
                   ess=out["ess"], resampled=out["resampled"], regimes=regimes, ancestors=ancestors, levels=out["levels"], paths=out["paths"],
                   **{"out_" + k: t for k, t in so.items()}))
    lib = N.lib_for(Y)
    lib.check(N.timed("switching_pf", Y, lambda: lib.dll.kvae_lgssm_switching_pf(C.byref(pr), N.stream_for(Y))), "kvae_lgssm_switching_pf")
    del keep, st
    if out["resampled"] is not None:
        out["resampled"] = out["resampled"] != 0
    return out


def combine_replicates(log_lik):
    """What the replicates of one sequence say together, from log_lik [B,G,T]: (log_lik_seq_mean [B] = the logmeanexp over the
    replicates of their sums over t - still an unbiased estimate of p(a | u) after exp -, weights [B,G,T] = exp(cumulative log_lik)
    normalised over the replicates: the weights under which the replicate average of regime_filt is consistent)."""
    cum = log_lik.cumsum(-1)
    G = log_lik.shape[1]
    mean = torch.logsumexp(cum[..., -1], 1) - math.log(G)   # (a Python constant: nothing is copied to the device)
    return mean, torch.softmax(cum, 1)


# ------------------------------------------------------------------------------------------------
# switching Kalman smoother, GPB2 (kvae_lgssm_switching_smoother, csrc/lgssm_sws.h)
# ------------------------------------------------------------------------------------------------
def switching_smoother_supported(K, n, m, p, ref=None):
    """Shapes / tensors kvae_lgssm_switching_smoother is built for: the filter's (switching_filter_supported); the rest takes
    switching_smoother_torch."""
    return switching_filter_supported(K, n, m, p, ref)


@torch.no_grad()
def switching_smoother(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, want=_SWS_OUTPUTS, state=None, impl=None):
    """The switching Kalman smoother with GPB2 collapse over the generative switching model (semantics: include/kvae_lgssm.h,
    kvae_lgssm_switching_smoother): switching_filter forwards, with the same arguments, then a backward pass
    over the beliefs and pair weights the filter kept.  Every Q_k must be positive definite (the backward pass solves with
    Sigma_pred without pivoting).  want: any of switching_filter's outputs - the bits of that call's - and "regime_smooth" [B,T,K]
    = p(s_t | a_{0:T-1}), "regime_pairs" [B,T-1,K,K] = p(s_t = j, s_{t+1} = k | a_{0:T-1}) indexed (j, k), "mus_smooth" [B,T,n],
    "Sigmas_smooth" [B,T,n,n] the moment-matched smoothed belief; entries not asked for are None.  state: as switching_filter;
    the smoothing is then conditional on this window alone (nothing flows back into the earlier chunk).  At most three launches
    (forward, backward, log_lik_seq), no host synchronisation, no gradients.
    impl: None = the HIP kernel where it is built (switching_smoother_supported), else switching_smoother_torch; "hip" / "torch"
    force one."""
    want = _want("switching_smoother", _SWS_OUTPUTS, want)
    if not _sw_route("switching_smoother", impl, switching_smoother_supported, A, Bm, Y):
        return switching_smoother_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, want)
    sp = N.SwsProblem()
    out, _, keep = _swf_problem(sp.filt, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, tuple(w for w in want if w in _SWF_OUTPUTS))
    hist = _bind(sp, _sw_history(Y, A, pairs=True))
    out.update(_sws_outputs(sp, A, Y, want))
    lib = N.lib_for(Y)
    lib.check(N.timed("switching_smoother", Y, lambda: lib.dll.kvae_lgssm_switching_smoother(C.byref(sp), N.stream_for(Y))),
              "kvae_lgssm_switching_smoother")
    del keep, hist
    return out


def _sw_history(Y, A, pairs):
    """{field: a fresh buffer} of what the forward sweep keeps of every step for a second pass over it.  pairs: the smoother's and
    EM's form (the beliefs per regime, the pair weights, the final weights), else the forecast's and the marginal's (the log weights
    and the beliefs per regime)."""
    (Bsz, T), (K, n), dev = Y.shape[:2], A.shape[:2], Y.device
    if pairs:
        return dict(hist_mu=_empty(dev, Bsz, T, K, n), hist_Sigma=_empty(dev, Bsz, T, K, n, n), hist_W=_empty(dev, Bsz, T, K, K),
                    hist_w=_empty(dev, Bsz, K))
    return dict(hist_lw=_empty(dev, Bsz, T, K), hist_mu=_empty(dev, Bsz, T, K, n), hist_Sigma=_empty(dev, Bsz, T, K, n, n))


def _sws_outputs(sp, A, Y, want):
    """The smoother's four outputs named in `want`, bound to the kvae_sws_problem `sp`."""
    (Bsz, T), (K, n) = Y.shape[:2], A.shape[:2]
    out = _wanted(Y.device, _SWS_SMOOTH, want, dict(regime_smooth=(Bsz, T, K), regime_pairs=(Bsz, max(T - 1, 1), K, K),
                                                    mus_smooth=(Bsz, T, n), Sigmas_smooth=(Bsz, T, n, n)))
    _bind(sp, out)
    if out["regime_pairs"] is not None:
        out["regime_pairs"] = out["regime_pairs"][:, :T - 1]   # nothing is written at T = 1 (the view keeps the bound buffer alive)
    return out


# ------------------------------------------------------------------------------------------------
# multi-horizon forecasts of the switching model, GPB2 (kvae_lgssm_switching_forecast, csrc/lgssm_swh.h)
# ------------------------------------------------------------------------------------------------
def switching_forecast_supported(K, n, m, p, ref=None):
    """Shapes / tensors kvae_lgssm_switching_forecast is built for: the filter's (switching_filter_supported); the rest takes
    switching_forecast_torch."""
    return switching_filter_supported(K, n, m, p, ref)


@torch.no_grad()
def switching_forecast(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U_all, horizon, mask=None, origins="all", want=_SWH_OUTPUTS, state=None,
                       impl=None):
    """Forecasts of the generative switching model at the horizons h = 1 .. H from every step of a sequence (semantics:
    include/kvae_lgssm.h, kvae_lgssm_switching_forecast): switching_filter forwards over Y [B,T,p] with the
    same arguments, then from the filter's state at every origin t, H of the filter's hidden steps on U_all[:, t + h].  U_all
    [B,T+H,m], or None for zeros.  origins: "all" (t = 0 .. T-1, T_o = T) or "last" (t = T-1, T_o = 1: the online case after a
    carried state).  want: any of switching_filter's outputs - the bits of that call's - and, indexed [b, t - t0, h - 1],
    "regime_fore" [B,T_o,H,K] = p(s_{t+h} | a_{0:t}), "a_fore" [B,T_o,H,p], "S_fore" [B,T_o,H,p,p] the mean and covariance of
    a_{t+h} | a_{0:t}, "mus_fore" [B,T_o,H,n], "Sigmas_fore" [B,T_o,H,n,n] those of z_{t+h} (all exact under the model), "log_lik_fore"
    [B,T_o,H] = log p(a_{t+h} | a_{0:t}, u) where the target lies inside the sequence and is observed, else exactly 0 (exact at
    h = 1, the GPB2 mixture beyond), "levels_fore" [B,T_o,H] (int32); entries not asked for are None.  At most three launches
    (forward, forecast, log_lik_seq), no host synchronisation, no gradients.
    impl: None = the HIP kernel where it is built (switching_forecast_supported), else switching_forecast_torch; "hip" / "torch"
    force one."""
    want = _want("switching_forecast", _SWH_OUTPUTS, want)
    _check_impl("switching_forecast", impl)
    (K, n), (Bsz, T, p) = A.shape[:2], Y.shape
    H, t0, U_all = _swh_args("switching_forecast", Bm, Y, U_all, horizon, origins)
    if not _sw_route("switching_forecast", impl, switching_forecast_supported, A, Bm, Y):
        return switching_forecast_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U_all, H, mask, origins, state, want)
    dev = Y.device
    U_all = _f32c(U_all.detach().to(dev))
    fp = N.SwhProblem()
    out, _, keep = _swf_problem(fp.filt, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U_all[:, :T], mask, state,
                                tuple(w for w in want if w in _SWF_OUTPUTS))
    hist = _bind(fp, _sw_history(Y, A, pairs=False))
    fp.H, fp.t0 = H, t0
    shapes = dict(regime_fore=(K,), a_fore=(p,), S_fore=(p, p), mus_fore=(n,), Sigmas_fore=(n, n), log_lik_fore=(), levels_fore=())
    fore = _wanted(dev, _SWH_FORE, want, {k: (Bsz, T - t0, H, *s) for k, s in shapes.items()})
    _bind(fp, dict(u_all=U_all, **{"ll_fore" if k == "log_lik_fore" else k: t for k, t in fore.items()}))
    out.update(fore)
    lib = N.lib_for(Y)
    lib.check(N.timed("switching_forecast", Y, lambda: lib.dll.kvae_lgssm_switching_forecast(C.byref(fp), N.stream_for(Y))),
              "kvae_lgssm_switching_forecast")
    del keep, hist
    return out


# ------------------------------------------------------------------------------------------------
# approximate Viterbi decoder of the switching model (kvae_lgssm_switching_viterbi, csrc/lgssm_swv.h)
# ------------------------------------------------------------------------------------------------
def switching_viterbi_supported(K, n, m, p, ref=None):
    """Shapes / tensors kvae_lgssm_switching_viterbi is built for: the filter's (switching_filter_supported); the rest takes
    switching_viterbi_torch."""
    return switching_filter_supported(K, n, m, p, ref)


@torch.no_grad()
def switching_viterbi(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, want=_SWV_OUTPUTS, state=None, impl=None):
    """The most likely regime path of the generative switching model by the approximate Viterbi decoder of Pavlovic, Rehg &
    MacCormick (semantics: include/kvae_lgssm.h, kvae_lgssm_switching_viterbi): the model and operands of
    switching_filter; one survivor path per regime with its score and exact Kalman belief, a selection where the filter collapses.
    want: which of "path" [B,T] (int32), "path_log_joint" [B] = the exact log p(a, s = path | u), "scores" [B,T,K] = J_t(j),
    "backptr" [B,T,K] (int32), "mus_filt" [B,T,n], "Sigmas_filt" [B,T,n,n] (the Kalman-filtered belief given path_{0:t}), "levels"
    [B,T] (int32), "state" (dict score [B,K], mu [B,K,n], Sigma [B,K,n,n] after the last step) to compute; entries not asked for
    are None.  state: None or the "state" entry of an earlier call, which continues that stream: scores, backptr and state are then
    the bits of the whole-sequence call; a chunk's path is conditional on the chunk's own end, and the path of the whole stream
    follows the concatenated backptr from the lowest arg max of the last scores (backptr[:, 0] of a later chunk points into the
    chunk before it).  One launch, no host synchronisation, no gradients.
    impl: None = the HIP kernel where it is built (switching_viterbi_supported), else switching_viterbi_torch; "hip" / "torch"
    force one."""
    want = _want("switching_viterbi", _SWV_OUTPUTS, want)
    if not _sw_route("switching_viterbi", impl, switching_viterbi_supported, A, Bm, Y):
        return switching_viterbi_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, state, want)
    (K, n), (Bsz, T, _), dev = A.shape[:2], Y.shape, Y.device
    pr = N.SwvProblem()
    pr.B, pr.T, pr.K, pr.n, pr.m, pr.p = Bsz, T, K, n, Bm.shape[2], Y.shape[2]
    keep = _sw_operands(pr, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask)
    st = _swv_state(state, Bsz, K, n)
    if st is not None:
        st = _bind(pr, {"state_" + k: _f32c(t.detach().to(dev)) for k, t in zip(("score", "mu", "Sigma"), st)})
    out = _wanted(dev, _SWV_OUTPUTS, want, dict(path=(Bsz, T), path_log_joint=(Bsz,), scores=(Bsz, T, K), backptr=(Bsz, T, K),
                                                mus_filt=(Bsz, T, n), Sigmas_filt=(Bsz, T, n, n), levels=(Bsz, T)))
    if "state" in want:
        out["state"] = {"score": _empty(dev, Bsz, K), "mu": _empty(dev, Bsz, K, n), "Sigma": _empty(dev, Bsz, K, n, n)}
        _bind(pr, {"out_" + k: t for k, t in out["state"].items()})
    walked = {"path": (), "mus_filt": ("ws_mu",), "Sigmas_filt": ("ws_Sigma",)}   # what the backtrace writes: the workspace each reads besides the words
    ws = _wanted(dev, ("ws_bp", "ws_mu", "ws_Sigma"), {w for k, v in walked.items() if k in want for w in ("ws_bp",) + v},
                 dict(ws_bp=(Bsz, T), ws_mu=(Bsz, T, K, n), ws_Sigma=(Bsz, T, K, n, n)))
    _bind(pr, {k: out[k] for k in _SWV_OUTPUTS if k != "state"})
    _bind(pr, ws)
    lib = N.lib_for(Y)
    lib.check(N.timed("switching_viterbi", Y, lambda: lib.dll.kvae_lgssm_switching_viterbi(C.byref(pr), N.stream_for(Y))),
              "kvae_lgssm_switching_viterbi")
    del keep, st, ws
    return out


# ------------------------------------------------------------------------------------------------
# log p(a | u) with the regimes summed out, differentiable (kvae_lgssm_switching_marginal[_bwd], csrc/lgssm_swm.h)
# ------------------------------------------------------------------------------------------------
def _swm_problem(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, hist):
    """(kvae_swm_problem, tensors to keep alive) over the inputs and the history (lw, mu, Sigma); the output pointers are NULL."""
    sp = N.SwmProblem()
    _, _, keep = _swf_problem(sp.filt, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, None, ())
    return sp, keep[:-1] + _bind(sp, dict(zip(("hist_lw", "hist_mu", "hist_Sigma"), hist)))


class SwitchingLogLik(torch.autograd.Function):
    """(ll [B,T], seq_ll [B], levels [B,T]) of kvae_lgssm_switching_marginal with the adjoint kvae_lgssm_switching_marginal_bwd: one
    call each way (the backward: the sweep and the sum of its per-sequence partials).  Gradients for A, Bm, Q, Cm, P (g_logP / P
    where P > 0, else 0), mu0, Sigma0, Y and U.  R is a buffer of the model: no gradient."""

    @staticmethod
    def forward(ctx, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask):
        Bsz, T, _ = Y.shape
        dev = Y.device
        hist = tuple(_sw_history(Y, A, pairs=False).values())
        sp, keep = _swm_problem(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, hist)
        ll, seq, levels = _bind(sp.filt, dict(ll=_empty(dev, Bsz, T), seq_ll=_empty(dev, Bsz), levels=_empty(dev, Bsz, T, dt=torch.int32)))
        lib = N.lib_for(Y)
        lib.check(N.timed("switching_marginal", Y, lambda: lib.dll.kvae_lgssm_switching_marginal(C.byref(sp), N.stream_for(Y))),
                  "kvae_lgssm_switching_marginal")
        del keep
        ctx.mark_non_differentiable(levels)
        ctx.set_materialize_grads(False)   # an output nobody differentiates arrives as None: a NULL upstream
        ctx.has_mask = mask is not None
        ctx.save_for_backward(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, *hist, *(() if mask is None else (mask,)))
        return ll, seq, levels

    @staticmethod
    def backward(ctx, g_ll, g_seq, _g_levels):
        need = ctx.needs_input_grad
        if (g_ll is None and g_seq is None) or not any(need):
            return (None,) * 11
        A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, *rest = ctx.saved_tensors
        hist, mask = tuple(rest[:3]), (rest[3] if ctx.has_mask else None)
        K, n, m = A.shape[0], A.shape[1], Bm.shape[2]
        Bsz, T, p = Y.shape
        dev = Y.device
        sp, keep = _swm_problem(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, hist)
        g_ll, g_seq = _f32c(g_ll), _f32c(g_seq)
        lib = N.lib_for(Y)
        ws = _empty(dev, lib.dll.kvae_lgssm_switching_marginal_ws_floats(Bsz, K, n, m))
        shapes = ((K, n, n), (K, n, m), (K, n, n), None, None, (K, K), (n,), (n, n), (Bsz, T, p), (Bsz, T, m))
        outs = [None if s is None or not need[i] else _empty(dev, *s) for i, s in enumerate(shapes)]
        if need[3]:
            outs[3] = _empty(dev, p, n)
        g = N.SwmGrads()
        g.g_ll, g.g_seq, g.ws = N.ptr(g_ll), N.ptr(g_seq), ws.data_ptr()
        g.gA, g.gB, g.gQ, g.gC, _, g.g_logP, g.g_mu0, g.g_Sigma0, g.gY, g.gU = (N.ptr(o) for o in outs)
        lib.check(N.timed("switching_marginal_bwd", Y, lambda: lib.dll.kvae_lgssm_switching_marginal_bwd(C.byref(sp), C.byref(g),
                                                                                                        N.stream_for(Y))),
                  "kvae_lgssm_switching_marginal_bwd")
        del keep
        if outs[5] is not None:   # gP from the adjoint of log P: exactly 0 at the zeros of P
            Pd = P.detach().to(dev, torch.float32)
            outs[5] = torch.where(Pd > 0, outs[5] / torch.where(Pd > 0, Pd, torch.ones_like(Pd)), torch.zeros_like(Pd))
        cast = lambda o, ref: None if o is None else o.to(ref.dtype).reshape(ref.shape)
        return tuple(cast(o, ref) for o, ref in zip(outs, (A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U))) + (None,)


def switching_log_marginal(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, state=None, impl=None):
    """log p(a_t | a_{0:t-1}, u) of every step with the regimes summed out under GPB2 collapse, and its per-sequence sum,
    DIFFERENTIABLE w.r.t. A, Bm, Q, Cm, P, mu0, Sigma0, Y and U (switching_filter is the no-grad read-out with more outputs; its
    log_lik, log_lik_seq and levels are these bits).  Arguments as switching_filter; R is a buffer (no gradient); a carried
    `state` is not accepted (no truncated back-propagation through streams): ValueError.  It is the gradient of the GPB2 value:
    exact where the filter is exact (P = I, shared A / B / Q, t <= 1), elsewhere the gradient of the approximation.
    Returns dict(ll [B,T], seq_ll [B], levels [B,T] int32).  Forward two launches, backward two (the adjoint sweep, the sum of its
    per-sequence partials), no atomics, no host synchronisation.
    impl: None = the HIP kernels where built (switching_filter_supported), else switching_log_marginal_torch; "hip" / "torch" force one."""
    if state is not None:
        raise ValueError("switching_log_marginal: a carried state is not differentiable here (state must be None)")
    if not _sw_route("switching_log_marginal", impl, switching_filter_supported, A, Bm, Y, fp32_model=True):
        return switching_log_marginal_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask)
    dev = Y.device
    mask = None if mask is None else mask.detach().to(dev).reshape(Y.shape[0], Y.shape[1])
    ll, seq, levels = SwitchingLogLik.apply(*(t.to(dev) for t in (A, Bm, Q, Cm)), R.detach().to(dev), *(t.to(dev) for t in (P, mu0, Sigma0)), Y, U, mask)
    return {"ll": ll, "seq_ll": seq, "levels": levels}



# ------------------------------------------------------------------------------------------------
# EM for the switching dynamics: the expected sufficient statistics (kvae_lgssm_switching_em, csrc/lgssm_em.h)
# ------------------------------------------------------------------------------------------------
def switching_em_supported(K, n, m, p, ref=None):
    """Shapes / tensors kvae_lgssm_switching_em is built for: the filter's (switching_filter_supported); the rest takes
    switching_em_statistics_torch."""
    return switching_filter_supported(K, n, m, p, ref)


def _em_shapes(K, n, m):
    x = n + m
    return dict(N=(K,), S11=(K, n, n), S10=(K, n, x), S00=(K, x, x), counts=(K, K), Syz=(2, n), Szz=(n, n), Syy=(2, 2), Nobs=(1,),
                z0=(n,), z0z0=(n, n), nseq=(1,))


@torch.no_grad()
def switching_em_statistics(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask=None, want=_EM_OUTPUTS, state=None, impl=None, ws_out=None):
    """The E-step of EM for the generative switching model (semantics: include/kvae_lgssm.h, kvae_lgssm_switching_em; DESIGN.md
    section 17): switching_smoother, whose backward pass also crosses the transition into t = 0 and accumulates the expected
    sufficient statistics.  Arguments as switching_smoother; a carried `state` is not accepted: ValueError.  want: which of the
    sums over the sequences "N" [K], "S11" [K,n,n], "S10" [K,n,n+m], "S00" [K,n+m,n+m], "counts" [K,K], "Syz" [2,n], "Szz" [n,n],
    "Syy" [2,2], "Nobs" [1], "z0" [n], "z0z0" [n,n], "nseq" [1], of "log_lik_seq" [B] and of the four smoother outputs to compute;
    entries not asked for are None.  The statistics are additive over batches (em_add) and feed switching_em_mstep.  At most four
    launches (forward, backward, the sum over the sequences, log_lik_seq), no atomics, no host synchronisation, no gradients.
    ws_out: a list that receives the per-sequence rows [B, G] the kernel wrote (tests).
    impl: None = the HIP kernel where it is built (switching_em_supported), else switching_em_statistics_torch; "hip" / "torch"
    force one."""
    want = _want("switching_em_statistics", _EM_OUTPUTS, want)
    if state is not None:
        raise ValueError("switching_em_statistics: a carried state is not accepted (the step into t = 0 needs the prior; state must be None)")
    if not _sw_route("switching_em_statistics", impl, switching_em_supported, A, Bm, Y, fp32_model=True):
        return switching_em_statistics_torch(A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, want)
    K, n, m, Bsz, dev = A.shape[0], A.shape[1], Bm.shape[2], Y.shape[0], Y.device
    sp, es = N.SwsProblem(), N.EmStats()
    out, _, keep = _swf_problem(sp.filt, A, Bm, Q, Cm, R, P, mu0, Sigma0, Y, U, mask, None, tuple(w for w in want if w == "log_lik_seq"))
    out = {"log_lik_seq": out["log_lik_seq"]}
    hist = _bind(sp, _sw_history(Y, A, pairs=True))
    out.update(_sws_outputs(sp, A, Y, want))
    stats = _wanted(dev, _EM_STATS, want, _em_shapes(K, n, m))
    out.update(stats)
    lib = N.lib_for(Y)
    ws = _empty(dev, Bsz, lib.dll.kvae_lgssm_switching_em_ws_floats(Bsz, K, n, m) // Bsz)
    _bind(es, dict(stats, ws=ws))
    lib.check(N.timed("switching_em", Y, lambda: lib.dll.kvae_lgssm_switching_em(C.byref(sp), C.byref(es), N.stream_for(Y))),
              "kvae_lgssm_switching_em")
    del keep, hist
    if ws_out is not None:
        ws_out.append(ws)
    return {k: out[k] for k in _EM_OUTPUTS}


def em_ws_blocks(ws, K, n, m):
    """The per-sequence rows [B, G] of kvae_lgssm_switching_em's workspace as a dict of [B, ...] views, in the layout of
    include/kvae_lgssm.h."""
    out, off = {}, 0
    for k, shp in _em_shapes(K, n, m).items():
        if k == "nseq":
            continue
        size = 1
        for d in shp:
            size *= d
        out[k] = ws[:, off:off + size].reshape(ws.shape[0], *shp)
        off += size
    assert off == ws.shape[1], (off, ws.shape)
    return out


def em_add(a, b):
    """The sum of two statistics dicts of switching_em_statistics (the statistics are additive over batches); "log_lik_seq" is
    concatenated; the smoother outputs, which belong to one batch, are dropped."""
    out = {}
    for k in _EM_STATS:
        x, y = a.get(k), b.get(k)
        out[k] = None if x is None or y is None else x.double() + y.double().to(x.device)
    x, y = a.get("log_lik_seq"), b.get("log_lik_seq")
    out["log_lik_seq"] = None if x is None or y is None else torch.cat([x, y.to(x.device)])
    return out
