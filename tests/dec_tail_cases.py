"""Cases of the decoder head with the Bernoulli term folded in (csrc/vae_conv_edge.h: k_dec_head_fwd<true>, k_dec_head_bwd;
C ABI kvae_dec_head_loss_fwd / kvae_dec_head_loss_bwd; kvae.vae.fused.DecoderHeadBernoulli), shared by the CPU tier (the plain-loop
twins of tests/hostsim, tests/test_dec_tail.py) and the GPU tier (tests/test_gpu_dec_tail.py).

Reference: float64 - _conv_ref64 of parity_cases (no torch convolution), then float64 BCEWithLogits summed per frame and float64
sigmoid; gradients by autograd.  Quantities: `ll` (per frame), `recon` (per frame), `dx` (per (frame, channel) plane), `dw` (per
(output channel, input channel)), `db` (whole), each as the ratio of _per_step_ratio / rel_err.

Bars = 4 x TAIL_YARDSTICK, the rule of parity_cases.VAE_STEP_TOL: the yardstick of a quantity is the largest ratio of FLOAT32 TORCH
ON THE CPU (F.conv2d, F.pixel_shuffle, F.binary_cross_entropy_with_logits, torch.sigmoid in float32 on the same inputs) against
that float64 reference over every case below - TAIL_N with and without a gradient handed to the logits, and every probe
(rerun: tail_yardstick())."""
import functools

import torch
import torch.nn.functional as F

from parity_cases import _check_steps, _check_whole, _conv_ref64, _conv_torch, _rows

TAIL_N = (1, 3, 1023, 1025, 2049)   # one frame, a ragged small grid, both sides of the 1024-row persistent grid, three frames per workgroup
TAIL_YARDSTICK = {"ll": 1.66e-07, "recon": 4.10e-07, "dx": 5.68e-07, "dw": 1.95e-05, "db": 1.31e-05}   # tail_yardstick(), CPU
TAIL_TOL = {k: 4.0 * v for k, v in TAIL_YARDSTICK.items()}
PROBE_N, PROBE_FRAMES = 3, (0, 2)
PROBE_X = [(0, 0), (0, 31), (31, 0), (31, 31), (0, 17)]     # 32 x 32 frame: the four corners (all four sub-pixel channels) and an edge
PROBE_H = [(0, 0), (0, 15), (15, 0), (15, 15), (7, 15)]     # 16 x 16 activation
GUARD = 1024
SENTINEL = 1.5e30
OK, ERR_DIMS, ERR_NULL, ERR_ARG = 0, 1, 2, 4


def tail_inputs(N, seed=0):
    """h [N,32,16,16] (non-negative, like the ReLU output the head sees), W [4,32,3,3], b [4], x [N,1,32,32] in {0, 1}, the upstream
    gradients of frame_ll [N] and of the logits [N,1,32,32]; float32 on the host."""
    g = torch.Generator().manual_seed(6151 * seed + 13 * N + 5)
    h = torch.relu(torch.randn(N, 32, 16, 16, generator=g))
    W, b = 0.1 * torch.randn(4, 32, 3, 3, generator=g), torch.randn(4, generator=g)
    x = (torch.rand(N, 1, 32, 32, generator=g) < 0.2).float()
    return h, W, b, x, torch.randn(N, generator=g), torch.randn(N, 1, 32, 32, generator=g)


def probe_inputs(kind, frame, pos):
    """"x": the target frames are zero but for ONE pixel of one frame: that pixel alone adds -logit to frame_ll and g_frame to the
    gradient of the logits, so a wrong place in the PixelShuffle map is an O(1) term of ll, dx, dw and db.  (Logits pushed to -30
    to isolate the impulse would measure the rounding of a sum next to a large bias instead: 1e-5 of sigmoid = 1e-13.)
    "h": the activation is zero but for ONE element of one frame (channel 5)."""
    h, W, b, x, gll, gl = tail_inputs(PROBE_N, seed=11)
    if kind == "x":
        x = torch.zeros_like(x)
        x[frame, 0, pos[0], pos[1]] = 1.0
        gll = gll.abs() + 0.5
    else:
        hh = torch.zeros_like(h)
        hh[frame, 5, pos[0], pos[1]] = 2.5
        h = hh
    return h, W, b, x, gll, gl


def _chain(conv, h, W, b, x, gll, gl):
    logits, _ = conv(h, W, b, 1, 2, False)
    ll = -F.binary_cross_entropy_with_logits(logits, x.to(logits.dtype), reduction="none").sum(dim=(1, 2, 3))
    obj = (ll * gll.to(ll.dtype)).sum()
    if gl is not None:
        obj = obj + (logits * gl.to(logits.dtype)).sum()
    obj.backward()
    return dict(logits=logits.detach(), ll=ll.detach(), recon=torch.sigmoid(logits.detach()), dx=h.grad, dw=W.grad, db=b.grad)


def reference(h, W, b, x, gll, gl=None, dtype=torch.float64):
    """The float64 reference (dtype float32 + torch's own convolution: the yardstick)."""
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    return _chain(_conv_ref64 if dtype == torch.float64 else _conv_torch, leaf(h), leaf(W), leaf(b), x, gll, gl)


@functools.lru_cache(maxsize=None)
def case(N, general=False):
    """Inputs and float64 reference of one random case, computed once per process."""
    inp = tail_inputs(N)
    return inp, reference(*inp[:5], inp[5] if general else None)


def compare(got, want, out):
    """got: float32 results (logits / recon [N,1,32,32], ll [N], dx [N,32,16,16] or None, dw [4,32,3,3], db [4])."""
    _check_steps("ll", _rows(got["ll"]), _rows(want["ll"]), TAIL_TOL["ll"], out)
    if got.get("recon") is not None:
        _check_steps("recon", _rows(got["recon"]), _rows(want["recon"]), TAIL_TOL["recon"], out)
    if got.get("dx") is not None:
        _check_steps("dx", got["dx"].detach().cpu().flatten(2), want["dx"].flatten(2), TAIL_TOL["dx"], out)
    _check_steps("dw", got["dw"].detach().cpu().flatten(2), want["dw"].flatten(2), TAIL_TOL["dw"], out)
    _check_whole("db", got["db"], want["db"], TAIL_TOL["db"], out)
    return out


class Guarded:
    """An output buffer filled with a sentinel, GUARD floats of it on either side of the part the kernel may write."""

    def __init__(self, DEV, *shape):
        n = 1
        for s in shape:
            n *= s
        self.whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
        self.t = self.whole[GUARD:GUARD + n].view(*shape)

    def check(self, name):
        assert bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[-GUARD:] == SENTINEL).all()), f"{name}: wrote outside"
        assert not bool((self.t == SENTINEL).any()), f"{name}: left elements unwritten"
        return self.t


def _lib(t):
    from kvae import _native
    return _native, _native.lib_for(t)


def raw_fused(DEV, h, W, b, x, gll, with_recon=True, with_gin=True):
    """kvae_dec_head_loss_fwd + kvae_dec_head_loss_bwd through the C ABI, every output in a guarded buffer; the partial rows are
    summed here in float64 (kvae_colsum has tests of its own)."""
    h, W, b, x, gll = (t.to(DEV).contiguous() for t in (h, W, b, x, gll))
    Nn, lib = _lib(h)
    N = h.shape[0]
    rows = lib.dll.kvae_conv_edge_partial_rows(N)
    logits, ll = Guarded(DEV, N, 1, 32, 32), Guarded(DEV, N)
    recon = Guarded(DEV, N, 1, 32, 32) if with_recon else None
    g_in = Guarded(DEV, N, 32, 16, 16) if with_gin else None
    wp, bp, scratch = Guarded(DEV, rows, 1152), Guarded(DEV, rows, 4), Guarded(DEV, 2304)
    st = Nn.stream_for(h)
    rc = lib.dll.kvae_dec_head_loss_fwd(Nn.ptr(h), Nn.ptr(W), Nn.ptr(b), Nn.ptr(x), Nn.ptr(logits.t), Nn.ptr(recon.t) if recon else None,
                                        Nn.ptr(ll.t), Nn.ptr(scratch.t), N, 32, 16, st)
    assert rc == OK, rc
    rc = lib.dll.kvae_dec_head_loss_bwd(Nn.ptr(h), Nn.ptr(W), Nn.ptr(logits.t), Nn.ptr(x), Nn.ptr(gll), Nn.ptr(g_in.t) if g_in else None,
                                        Nn.ptr(wp.t), Nn.ptr(bp.t), Nn.ptr(scratch.t), N, 32, 16, st)
    assert rc == OK, rc
    return dict(logits=logits.check("logits"), ll=ll.check("frame_ll"), recon=recon.check("x_recon") if recon else None,
                dx=g_in.check("g_in") if g_in else None, wp=wp.check("w_partials"), bp=bp.check("b_partials"),
                dw=wp.t.double().sum(0).view(4, 32, 3, 3).float(), db=bp.t.double().sum(0).float())


def _leaf(t, DEV, grad=True):
    return t.detach().to(DEV).clone().requires_grad_(grad)   # a copy: on the CPU tier .to() hands back the cached input itself


def fused_function(DEV, h, W, b, x, gll, gl=None, with_recon=True, want_dx=True):
    """fused.DecoderHeadBernoulli with autograd: the trainer's case (gl None) or the general backward (a gradient on the logits too)."""
    from kvae.vae.fused import DecoderHeadBernoulli
    hd, Wd, bd = _leaf(h, DEV, want_dx), _leaf(W, DEV), _leaf(b, DEV)
    logits, recon, ll = DecoderHeadBernoulli.apply(hd, Wd, bd, x.to(DEV), with_recon)
    obj = (ll * gll.to(DEV)).sum()
    if gl is not None:
        obj = obj + (logits * gl.to(DEV)).sum()
    obj.backward()
    assert recon is None or not recon.requires_grad
    return dict(logits=logits.detach(), ll=ll.detach(), recon=recon, dx=hd.grad, dw=Wd.grad, db=bd.grad)


def unfused_function(DEV, h, W, b, x, gll, gl=None):
    """This build's unfused route: DecoderHead + BernoulliFrameLogLik + torch.sigmoid."""
    from kvae.vae.fused import BernoulliFrameLogLik, DecoderHead
    hd, Wd, bd = _leaf(h, DEV), _leaf(W, DEV), _leaf(b, DEV)
    logits = DecoderHead.apply(hd, Wd, bd)
    ll = BernoulliFrameLogLik.apply(logits.unsqueeze(1), x.to(DEV).unsqueeze(1)).reshape(-1)
    obj = (ll * gll.to(DEV)).sum()
    if gl is not None:
        obj = obj + (logits * gl.to(DEV)).sum()
    obj.backward()
    return dict(logits=logits.detach(), ll=ll.detach(), recon=torch.sigmoid(logits.detach()), dx=hd.grad, dw=Wd.grad, db=bd.grad)


def tail_random(DEV, N):
    """One random case through the C ABI (guarded buffers) against float64, and bitwise against the unfused route."""
    inp, want = case(N)
    h, W, b, x, gll, _ = inp
    got = raw_fused(DEV, h, W, b, x, gll)
    out = compare(got, want, {})
    un = unfused_function(DEV, h, W, b, x, gll)
    assert torch.equal(got["logits"], un["logits"]), "logits differ from kvae_dec_head_fwd"
    assert torch.equal(got["dx"], un["dx"]), "g_h differs from the unfused route"
    fn = fused_function(DEV, h, W, b, x, gll)
    assert torch.equal(fn["dx"], un["dx"]) and torch.equal(fn["dw"], un["dw"]) and torch.equal(fn["db"], un["db"]), "dW / db differ"
    assert torch.equal(fn["ll"], got["ll"]) and torch.equal(fn["recon"], got["recon"])
    compare(un, want, {})   # the replaced two-kernel backward's successor, through kvae_dec_head_bwd
    return out


def tail_optional_outputs(DEV, N):
    """x_recon == NULL and g_in == NULL: the other outputs are the same bits."""
    inp, want = case(N)
    h, W, b, x, gll, _ = inp
    full = raw_fused(DEV, h, W, b, x, gll)
    part = raw_fused(DEV, h, W, b, x, gll, with_recon=False, with_gin=False)
    assert part["recon"] is None and part["dx"] is None
    for k in ("logits", "ll", "wp", "bp"):
        assert torch.equal(full[k], part[k]), k
    fn = fused_function(DEV, h, W, b, x, gll, with_recon=False, want_dx=False)
    assert fn["recon"] is None and fn["dx"] is None
    return compare(fn, want, {})


def tail_general(DEV, N):
    """A gradient handed to the logits as well as to frame_ll: kvae_bce_frames_bwd + kvae_dec_head_bwd."""
    inp, want = case(N, general=True)
    got = fused_function(DEV, *inp)
    out = compare(got, want, {})
    only = fused_function(DEV, *inp[:4], torch.zeros_like(inp[4]), inp[5])   # ... and to the logits alone
    un = unfused_function(DEV, *inp[:4], torch.zeros_like(inp[4]), inp[5])
    for k in ("dx", "dw", "db"):
        assert torch.equal(only[k], un[k]), k
    return out


def tail_probe(DEV, kind, frame, pos):
    inp = probe_inputs(kind, frame, pos)
    h, W, b, x, gll, _ = inp
    want = reference(h, W, b, x, gll)
    got = raw_fused(DEV, h, W, b, x, gll)
    return compare(got, want, {})


def tail_refusals(DEV):
    h, W, b, x, gll, _ = (t.to(DEV) for t in tail_inputs(1))
    Nn, lib = _lib(h)
    p = Nn.ptr
    logits, recon, ll, gin = torch.empty_like(x), torch.empty_like(x), torch.empty(1, device=DEV), torch.empty_like(h)
    wp, bp, sc = torch.empty(1, 1152, device=DEV), torch.empty(1, 4, device=DEV), torch.empty(2304, device=DEV)
    st = Nn.stream_for(h)
    fwd = [p(h), p(W), p(b), p(x), p(logits), p(recon), p(ll), p(sc)]
    bwd = [p(h), p(W), p(logits), p(x), p(gll), p(gin), p(wp), p(bp), p(sc)]
    for fn, args, optional in ((lib.dll.kvae_dec_head_loss_fwd, fwd, 5), (lib.dll.kvae_dec_head_loss_bwd, bwd, 5)):
        for i in range(len(args)):
            if i != optional:
                a = list(args)
                a[i] = None
                assert fn(*a, 1, 32, 16, st) == ERR_NULL, (fn.__name__, i)
        assert fn(*args, 0, 32, 16, st) == ERR_ARG and fn(*args, -3, 32, 16, st) == ERR_ARG
        assert fn(*args, 1, 16, 16, st) == ERR_DIMS and fn(*args, 1, 32, 8, st) == ERR_DIMS


def tail_yardstick():
    """Float32 torch on the CPU against the float64 reference over every case: the numbers of TAIL_YARDSTICK."""
    worst = {}
    runs = [(case(N, g)[0][:5] + ((case(N, g)[0][5],) if g else (None,)), case(N, g)[1]) for N in TAIL_N for g in (False, True)]
    for kind, P in (("x", PROBE_X), ("h", PROBE_H)):
        for f in PROBE_FRAMES:
            for pos in P:
                inp = probe_inputs(kind, f, pos)
                runs.append((inp[:5] + (None,), reference(*inp[:5])))
    bars = dict(TAIL_TOL)
    TAIL_TOL.update({k: float("inf") for k in TAIL_TOL})   # measuring: no bars
    try:
        for inp, want in runs:
            for k, v in compare(reference(*inp, dtype=torch.float32), want, {}).items():
                worst[k] = max(worst.get(k, 0.0), v)
    finally:
        TAIL_TOL.update(bars)
    return worst


# ---- model level: B = 2, T = 3 ----
def small_model(DEV, seed=0):
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    torch.manual_seed(seed)
    m = KVAE(KVAEConfig(dynamics_model="lstm", num_modes=3))
    with torch.no_grad():
        m.kalman_filter.dyn_params.A.add_(0.05 * torch.randn_like(m.kalman_filter.dyn_params.A))
        m.kalman_filter.dyn_params.head_w.bias.zero_()
    m.beta = 0.5
    return m


def small_batch(B=2, T=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, T, 1, 32, 32, generator=g) < 0.1).float()
    return x, torch.randn(B * T, 2, generator=g), torch.randn(B, T, 4, generator=g)


def model_other_tensor(DEV):
    """compute_loss handed ANOTHER tensor than the one the forward decoded against (a copy: compute_loss cannot know that it holds
    the same frames) must not take the forward's frame_ll: it calls BernoulliFrameLogLik on the logits, the gradient reaches the
    head through its general backward, and the loss and two gradients agree with the float64 oracle at smoke()'s bars.  The very
    tensor handed over takes frame_ll, no BernoulliFrameLogLik call.  Returns the relative distances."""
    from kvae import noise
    from kvae.vae import fused
    from oracle import torch_oracle as O
    model = small_model(DEV)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(DEV).train()
    x, eps_a, eps_z = small_batch()
    xd = x.to(DEV)
    calls = []
    real = fused.BernoulliFrameLogLik.apply
    fused.BernoulliFrameLogLik.apply = lambda *a: (calls.append(1), real(*a))[1]
    try:
        with noise.inject(eps_a=eps_a.to(DEV), eps_z=eps_z.to(DEV)):
            out = model(xd)
            assert out["frame_ll"] is not None and out["frame_ll_x"] is xd
            same = model.compute_loss(xd, out, with_metrics=False)
            assert not calls, "the forward's frame_ll was not taken for the forward's own tensor"
            losses = model.compute_loss(xd.clone(), out, with_metrics=False)
            assert len(calls) == 1, "another tensor must take the fall-back"
    finally:
        del fused.BernoulliFrameLogLik.apply
    losses["loss"].backward()
    ref_sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k, v in ref_sd.items():
        v.requires_grad_(v.is_floating_point() and (not k.startswith("kalman_filter.") or "dyn_params" in k))
    ref = O.kvae_forward(ref_sd, x.double(), None, kind="lstm", eps_a=eps_a.double(), eps_z=eps_z.double(), beta=0.5)
    ref["loss"].backward()
    rel = lambda a, b: float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30))
    return {"loss": rel(losses["loss"], ref["loss"]), "loss_same": rel(same["loss"], ref["loss"]),
            "recon": rel(out["x_recon"], ref["x_recon"]),
            "grad_head": rel(model.decoder.deconv_layers[-2].weight.grad, ref_sd["decoder.deconv_layers.6.weight"].grad),
            "grad_enc": rel(model.encoder.fc_mu.weight.grad, ref_sd["encoder.fc_mu.weight"].grad)}


def trainer_graph_vs_eager(DEV, steps=2):
    """Trainer.step replayed from a captured hipGraph against the eager step from the same start with the same draws, with the
    reference's logging outputs on (x_recon comes from the head's kernel).  Returns the largest distances."""
    from kvae import noise
    from kvae.train.train import Trainer
    x, eps_a, eps_z = small_batch()
    xd = x.to(DEV)

    def run(use_graph):
        tr = Trainer(small_model(DEV).to(DEV).train(), lr=1e-3, use_graph=use_graph, reference_logging=True)
        with noise.inject(eps_a=eps_a.to(DEV), eps_z=eps_z.to(DEV)):
            outs = [{k: v.detach().clone() for k, v in tr.step(xd).items() if torch.is_tensor(v)} for _ in range(steps)]
        torch.cuda.synchronize()
        return outs, torch.cat([p.detach().flatten() for p in tr.model.parameters()]).cpu()

    (eo, ep), (go, gp) = run(False), run(True)
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))
    return {"loss": max(rel(g["loss"], e["loss"]) for g, e in zip(go, eo)),
            "x_recon": max(float((g["x_recon"] - e["x_recon"]).abs().max()) for g, e in zip(go, eo)),
            "params": float((gp - ep).abs().max())}
