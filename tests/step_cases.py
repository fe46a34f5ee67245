"""The kernels BETWEEN the compute kernels of a training step, one element at a time: kvae_clip_adam (k_grad_sumsq + k_clip_adam,
csrc/clip_adam.h), kvae_loss_head_fwd/bwd (csrc/vae_heads.h), kvae_colsum / kvae_colsum2 (csrc/colsum.h) with the two-pass folding
of _native.colsum / colsum_pair, kvae_lgssm_emission_means (csrc/emission_means.h) and kvae_bias_shuffle_act_fwd/bwd
(csrc/vae_epilogue.h).  Device-agnostic case functions taking (lib, DEV, ...): the GPU tier (tests/test_gpu_step_kernels.py) runs
them on the gfx950 library, the CPU tiers on the same kernels on emulated workgroups (tests/test_wave_emu_step.py) and on the
plain-loop twins of tests/hostsim/hostsim.cpp (tests/test_step_kernels.py).

Reference: a float64 restatement of the operation on the same float32 input values.  For clip_adam every scalar (lr, beta1, beta2,
eps, weight_decay, clip) is first rounded through float32 - that is what ctypes.c_float hands the kernel, and with the exact
beta2 = 0.999 every bar would sit near 1e-5 ("the beta2 constant").  adam_anchor() pins the restatement against
torch.optim.Adam itself, in float64.

Every output lives inside a larger buffer filled with SENTINEL (Guarded): nothing outside the output may change, the workspace
past its min(ceil(n / 1024), 512) partials included.

`python tests/step_cases.py` prints the yardsticks."""
import ctypes as C
import math

import numpy as np
import torch

from parity_cases import _per_step_ratio

SENTINEL = -12345.0
KVAE_ERR_DIMS, KVAE_ERR_NULL, KVAE_ERR_ARG = 1, 2, 4

# Bars = 4 x YARDSTICK (the rule of parity_cases.RNN_YARDSTICK), where the yardstick of a quantity is the largest ratio of the
# FLOAT32 TORCH RESTATEMENT OF THE SAME FORMULAS (not torch.optim.Adam in float32: its (1 - beta2) is float32(0.001), 1.30e-5 away
# from 1 - float32(0.999)) against the float64 run, over the case lists below, which both tiers share (rerun: yardsticks()).
# Ratios: adam.m / adam.v / adam.upd per segment and step, max|err| / max(max|ref| on the segment, 1e-2 max|ref| on the buffer),
# upd = p_after - p_before formed in float64; adam.norm relative; head.* relative to the float64 sum of the absolute contributions
# the scalar is built from; head.coef relative; head.g per element relative to max|ref|; colsum per column relative to
# sum_r |x[r, c]|; emission per (b, t) by parity_cases._per_step_ratio; epi.bias per (partial row, channel) and per channel over
# all rows, relative to the sum of |g| over the same elements.
# Largest ratios the implementations reach against the same float64 runs, host twin | emulated kernels | gfx950:
#   adam.m 2.5e-07 | 2.5e-07 | 2.5e-07   adam.v 2.7e-07 | 2.7e-07 | 2.7e-07   adam.upd 4.1e-06 | 4.1e-06 | 4.1e-06
#   adam.norm 5.3e-08 | 6.5e-08 | 6.5e-08   head.recon 6.3e-08 | 7.5e-08 | 7.5e-08   head.reg 9.3e-08 | 1.0e-08 | 1.4e-08
#   head.vae 5.8e-08 | 7.9e-08 | 8.3e-08   head.tot 7.1e-08 | 7.0e-08 | 1.1e-07   head.coef 6.5e-08 | 6.5e-08 | 6.5e-08
#   head.g 8.1e-08 | 8.1e-08 | 8.1e-08   colsum 1.7e-07 | 1.4e-07 | 1.4e-07   emission 5.9e-07 | 4.0e-07 | 5.9e-07
#   epi.bias 1.2e-07 | 9.2e-08 | 9.2e-08
# Less than a factor 2 under the bar: none on gfx950 (smallest head.tot 2.55 x, head.vae 2.79 x); on the host twin head.reg, 1.95 x
# (the twin sums the frames in one sequential float32 loop).  DESIGN section 2.
YARDSTICK = {   # float32 torch restatement against the float64 reference, largest ratio over every case list
    "adam.m": 2.49e-7, "adam.v": 2.69e-7, "adam.upd": 4.13e-6, "adam.norm": 6.73e-8,
    "head.recon": 6.33e-8, "head.reg": 4.53e-8, "head.vae": 5.81e-8, "head.tot": 7.09e-8, "head.coef": 6.50e-8, "head.g": 8.09e-8,
    "colsum": 1.39e-7, "emission": 5.09e-7, "epi.bias": 8.04e-8,
}
TOL = {k: 4.0 * v for k, v in YARDSTICK.items()}


def F32(x):
    """A Python float rounded through float32: what ctypes.c_float hands the kernel."""
    return float(np.float32(x))


def _sync(DEV):
    if DEV != "cpu":
        torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _note(worst, key, ratio):
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), ratio)


class Guarded:
    """`n` elements on DEV that start `off` elements past a 16-byte boundary, inside a larger buffer filled with SENTINEL."""

    def __init__(self, DEV, n, off=0, init=None, dtype=torch.float32, pad=16):
        self.buf = torch.full((n + 2 * pad + 8,), SENTINEL, device=DEV, dtype=dtype)
        self.o = ((16 - self.buf.data_ptr() % 16) % 16) // 4 + pad + off
        self.n = n
        self.t = self.buf[self.o:self.o + n]
        if init is not None:
            self.t.copy_(init.reshape(-1))
        assert self.t.data_ptr() % 16 == 4 * off

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def cpu(self):
        return self.t.cpu().clone()

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:self.o] == SENTINEL).all()) and bool((b[self.o + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf.cpu() == SENTINEL).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------------
# 1. kvae_clip_adam
# ---------------------------------------------------------------------------------------------------------------------------
ADAM_SCALARS = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, clip=0.5, div=None)
ADAM_SPEC = dict(seg=True, state="zero", steps0=None, active=(None,), gscale=None, off=0, lr_dev=False, norm_out=True, seed=0,
                 **ADAM_SCALARS)


def adam_restated(p, m, v, steps, g, seg_of, active, sc, dtype):
    """One step of clip_grad_norm_ + torch.optim.Adam (L2 weight decay, no amsgrad) on flat buffers, every operation in `dtype`.
    A segment with active False is a parameter whose grad is None: no norm contribution, no moment, step or value update.
    sc: the scalars as Python floats already rounded through float32; div: the divisor of the multi-rank path (clamped to 1).
    Returns (p, m, v, steps, norm) in `dtype`."""
    t = lambda x: torch.tensor(x, dtype=dtype)
    P, G, M, V = (x.to(dtype) for x in (p, g, m, v))
    one = t(1.0)
    inv = one / torch.clamp(t(sc["div"]), min=1.0) if sc["div"] is not None else one
    on = active[seg_of]
    gs = torch.where(on, G * inv, t(0.0))
    norm = (gs * gs).sum().sqrt()
    scale = inv * (torch.clamp(t(sc["clip"]) / (norm + t(F32(1e-6))), max=1.0) if sc["clip"] > 0 else one)
    steps2 = steps.to(dtype) + active.to(dtype)
    b1, b2, lr, eps, wd = (t(sc[k]) for k in ("beta1", "beta2", "lr", "eps", "wd"))
    live = torch.where(active, steps2, one)                    # a frozen segment may still stand at step 0: no 1 / 0 for it
    step_size = (lr / (one - torch.pow(b1, live)))[seg_of]
    bc2s = (one - torch.pow(b2, live)).sqrt()[seg_of]
    gi = G * scale + wd * P if sc["wd"] != 0 else G * scale
    M2 = M + (gi - M) * (one - b1)
    V2 = b2 * V + (one - b2) * gi * gi
    P2 = P - step_size * M2 / (V2.sqrt() / bc2s + eps)
    return torch.where(on, P2, P), torch.where(on, M2, M), torch.where(on, V2, V), steps2, norm


def _seg_ratio(got, ref, seg_of, n_seg, on, active):
    """Largest per-segment ratio max|err| / max(max|ref| on the segment, 1e-2 max|ref| on the buffer) over the active segments,
    and the segment where it occurs."""
    zero = torch.zeros((), dtype=torch.float64)
    err = torch.where(on, (got.double() - ref).abs(), zero)
    mag = torch.where(on, ref.abs(), zero)
    fold = lambda x: torch.zeros(n_seg, dtype=torch.float64).scatter_reduce(0, seg_of, x, "amax", include_self=True)
    r = fold(err) / fold(mag).clamp_min(1e-2 * float(mag.max())).clamp_min(1e-300)
    r = torch.where(active, r, zero)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()), int(r.argmax())


def _adam_scalars(spec):
    sc = {k: F32(spec[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "clip")}
    sc["div"] = None if spec["div"] is None else F32(spec["div"])
    return sc


class AdamBuffers:
    """The operands of one kvae_clip_adam call on DEV, every one the call may write inside a guarded buffer."""

    def __init__(self, DEV, spec, p0, m0, v0, steps0, seg_of):
        n, n_seg, off = p0.numel(), steps0.numel(), spec["off"]
        self.DEV, self.n, self.n_seg, self.spec = DEV, n, n_seg, spec
        self.p, self.m, self.v = (Guarded(DEV, n, off, init=x) for x in (p0, m0, v0))
        self.g = Guarded(DEV, n, off)
        self.steps = Guarded(DEV, n_seg, init=steps0)
        self.norm = Guarded(DEV, 1)
        self.parts = min((n + 1023) // 1024, 512)
        self.ws = Guarded(DEV, self.parts)
        self.seg_of = seg_of.to(torch.int32).to(DEV) if spec["seg"] else None
        sc = _adam_scalars(spec)
        self.lr_dev = torch.tensor([sc["lr"]], device=DEV) if spec["lr_dev"] else None
        self.div_dev = torch.tensor([sc["div"]], device=DEV) if sc["div"] is not None else None
        self.sc = sc

    def call(self, lib, grad, active, n_seg=None, seg_of="own"):
        sc = self.sc
        self.g.t.copy_(grad)
        self.active = None if active is None else active.to(torch.float32).to(self.DEV)
        rc = lib.dll.kvae_clip_adam(
            self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n, _p(self.seg_of) if seg_of == "own" else seg_of,
            self.n_seg if n_seg is None else n_seg, _p(self.active), self.steps.ptr, _p(self.lr_dev),
            123.0 if self.lr_dev is not None else sc["lr"], sc["beta1"], sc["beta2"], sc["eps"], sc["wd"], sc["clip"],
            _p(self.div_dev), self.norm.ptr if self.spec["norm_out"] else None, self.ws.ptr, None)
        _sync(self.DEV)
        return rc

    def state(self):
        return self.p.cpu(), self.m.cpu(), self.v.cpu(), self.steps.cpu()

    def assert_guards(self, what):
        for k in ("p", "m", "v", "g", "steps", "norm", "ws"):
            assert getattr(self, k).guards_intact(), (what, k, "written outside the operand")
        if not self.spec["norm_out"]:
            assert self.norm.untouched(), (what, "norm_out was NULL")


def _adam_problem(c):
    spec = {**ADAM_SPEC, **c}
    sizes = list(spec["sizes"])
    n, n_seg = sum(sizes), len(sizes)
    assert spec["seg"] or n_seg == 1
    gen = torch.Generator().manual_seed(spec["seed"])
    seg_of = torch.repeat_interleave(torch.arange(n_seg), torch.tensor(sizes))
    gscale = torch.tensor(spec["gscale"] or [1.0] * n_seg, dtype=torch.float32)[seg_of]
    p0 = torch.randn(n, generator=gen) * 1e-2               # at scale 1 the ulp of p swamps the update
    if spec["state"] == "random":
        m0 = torch.randn(n, generator=gen) * gscale * 0.1
        v0 = (torch.rand(n, generator=gen) * 0.1 + 1e-3) * gscale * gscale
    else:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    steps0 = torch.tensor(spec["steps0"] or [0] * n_seg, dtype=torch.float32)
    return spec, gen, n, n_seg, seg_of, gscale, p0, m0, v0, steps0


def adam_case(lib, DEV, c, impl="kernel", bars=None, worst=None):
    """One case of ADAM_CASES: len(active) steps.  The implementation's own float32 state is carried from call to call and the
    float64 reference restarts each step from the state the implementation held before that call, so one bar serves every step.
    impl: "kernel" (lib on DEV) or "f32" (the float32 restatement: the yardstick)."""
    bars = TOL if bars is None else bars
    spec, gen, n, n_seg, seg_of, gscale, p0, m0, v0, steps0 = _adam_problem(c)
    sc = _adam_scalars(spec)
    if impl == "kernel":
        buf = AdamBuffers(DEV, spec, p0, m0, v0, steps0, seg_of)
    state = (p0, m0, v0, steps0)
    for it, act in enumerate(spec["active"]):
        what = (c["id"], "step", it)
        active = torch.ones(n_seg, dtype=torch.bool) if act is None else torch.tensor(act) != 0
        on = active[seg_of]
        grad = torch.randn(n, generator=gen) * gscale * (1.0 + 0.5 * it)
        grad[~on] = math.nan                                  # the mask, not a zero gradient, must exclude a frozen slot
        ref_p, ref_m, ref_v, ref_steps, ref_norm = adam_restated(*state, grad, seg_of, active, sc, torch.float64)
        if impl == "kernel":
            assert buf.call(lib, grad, None if act is None else torch.tensor(act)) == 0, what
            got = buf.state()
            got_norm = float(buf.norm.cpu()) if spec["norm_out"] else None
            buf.assert_guards(what)
            assert torch.equal(_bits(buf.g.cpu()), _bits(grad)), (what, "the gradient was written")
        else:
            q = adam_restated(*state, grad, seg_of, active, sc, torch.float32)
            got, got_norm = (q[0], q[1], q[2], q[3]), float(q[4])
        assert torch.equal(got[3].double(), ref_steps), (what, "seg_steps", got[3].tolist()[:8], ref_steps.tolist()[:8])
        for name, now, was in zip("pmv", got, state):
            assert torch.equal(_bits(now[~on]), _bits(was[~on])), (what, name, "a frozen element moved")
        upd, ref_upd = got[0].double() - state[0].double(), ref_p - state[0].double()
        for key, g_, r_ in (("adam.m", got[1], ref_m), ("adam.v", got[2], ref_v), ("adam.upd", upd, ref_upd)):
            ratio, sg = _seg_ratio(g_, r_, seg_of, n_seg, on, active)
            _note(worst, key, ratio)
            assert ratio < bars[key], (what, key, "segment", sg, ratio, bars[key])
        if got_norm is not None:
            rn = float(ref_norm)
            ratio = abs(got_norm - rn) / rn if rn > 0 else (0.0 if got_norm == 0.0 else math.inf)
            ratio = math.inf if math.isnan(ratio) else ratio
            _note(worst, "adam.norm", ratio)
            assert ratio < bars["adam.norm"], (what, "adam.norm", got_norm, rn, ratio)
        state = got
    return worst


def _adam_cases():
    out = []
    add = lambda id_, **kw: out.append(dict(id=id_, **kw))
    # size ring: one segment, seg_of NULL; from zero moments at step 0 and from a random state at step 7
    for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049):
        add(f"ring-{n}-zero", sizes=[n], seg=False, seed=n)
        add(f"ring-{n}-state", sizes=[n], seg=False, state="random", steps0=[7], seed=n + 1)
    # grid-stride rounds: 512 partials and 2048 blocks are the caps; 524545 = 2048 * 256 + 257 takes a second round of both loops
    add("stride-524288", sizes=[524288], seg=False, seed=11)
    add("stride-524545", sizes=[524545], seg=False, state="random", steps0=[3], seed=12)
    # segment layout (seg_active NULL with seg_of given); per-segment starting steps differ, so one bias correction for all shows
    cyc = lambda k, mod: [(3 * i) % mod for i in range(k)]
    add("layout-7-300-41", sizes=[7, 300, 41], steps0=[2, 0, 5], seed=21)
    add("layout-block-edges", sizes=[1, 1, 254, 1, 255, 513], steps0=cyc(6, 11), state="random", seed=22)
    add("layout-257-segments", sizes=[i % 5 + 1 for i in range(257)], steps0=cyc(257, 11), seed=23)
    add("layout-1024-segments", sizes=[1] * 1024, steps0=cyc(1024, 13), seed=24)
    # frozen segments over four steps (the frozen slots of g hold NaN)
    add("frozen-middle-thaws", sizes=[7, 300, 41], active=([1, 0, 1], [1, 0, 1], [1, 1, 1], [1, 1, 1]), seed=31)
    add("frozen-first-and-all", sizes=[7, 300, 41], active=([0, 1, 1], [0, 1, 1], [0, 0, 0], [0, 1, 1]), seed=32)
    add("frozen-256th-of-257", sizes=[i % 5 + 1 for i in range(257)], active=([1] * 255 + [0, 1],), steps0=cyc(257, 7), seed=33)
    add("frozen-257th-of-257", sizes=[i % 5 + 1 for i in range(257)], active=([1] * 256 + [0],), steps0=cyc(257, 7), seed=36)
    add("single-segment-active-mask", sizes=[300], seg=False, active=([1],), seed=34)
    add("single-segment-frozen", sizes=[300], seg=False, active=([0],), state="random", steps0=[4], seed=35)
    # per-segment step counts: the bias corrections from 1 - beta up to 1
    add("step-counts", sizes=[5, 300, 41, 257, 9], steps0=[0, 1, 9, 999, 99999], state="random", seed=41)
    # scalars
    base = dict(sizes=[7, 300, 41], state="random", steps0=[3, 0, 12])
    add("lr-dev", **base, lr_dev=True, seed=51)
    for d in (0.0, 1.0, 37.0):
        add(f"div-{d:g}", **base, div=d, seed=52)
    add("clip-off", **base, clip=0.0, seed=53)
    add("clip-inactive", **base, clip=1e9, seed=54)
    add("weight-decay", **base, wd=1e-2, seed=55)
    add("weight-decay-clip-off-div", **base, wd=1e-2, clip=0.0, div=37.0, lr_dev=True, seed=56)
    add("no-norm-out", **base, norm_out=False, seed=57)
    # magnitudes: gradients of scale 1e-7 .. 1e3 in one buffer, the clip active (scale ~ 0.1): in the 1e-7 segment sqrt(v_hat) is
    # of the order of eps, so eps inside the bias correction moves its update by tens of percent
    add("magnitudes", sizes=[300, 41, 7, 2], gscale=[1e-7, 1e-3, 1.0, 1e3], clip=150.0, seed=61)
    # all four buffers one float past a 16-byte boundary
    add("offset-by-one-float", sizes=[7, 300, 41], steps0=[1, 4, 0], state="random", off=1, seed=71)
    return out


ADAM_CASES = _adam_cases()
ADAM_IDS = [c["id"] for c in ADAM_CASES]


def adam_case_by_id(id_):
    return ADAM_CASES[ADAM_IDS.index(id_)]


def adam_rejects(lib, DEV):
    """n_seg above CA_MAX_SEG, and seg_of NULL with more than one segment: KVAE_ERR_ARG, no byte written."""
    spec, gen, n, n_seg, seg_of, gscale, p0, m0, v0, steps0 = _adam_problem(dict(sizes=[7, 300, 41], state="random", seed=81))
    wide = torch.zeros(1025)
    for kw in (dict(n_seg=1025), dict(n_seg=2, seg_of=None)):
        buf = AdamBuffers(DEV, spec, p0, m0, v0, wide, seg_of)
        assert buf.call(lib, torch.randn(n, generator=gen), torch.ones(1025), **kw) == KVAE_ERR_ARG, kw
        for got, was in zip(buf.state(), (p0, m0, v0, wide)):
            assert torch.equal(_bits(got), _bits(was)), kw
        buf.assert_guards(kw)
        assert buf.norm.untouched() and buf.ws.untouched(), kw


def adam_repeatable(lib, DEV, id_):
    """The same call from the same state twice: p, m, v and norm_out equal bit for bit (k_clip_adam: every block folds the same
    partials in the same order).  id_: a case id, or a case of the caller's own."""
    spec, gen, n, n_seg, seg_of, gscale, p0, m0, v0, steps0 = _adam_problem(adam_case_by_id(id_) if isinstance(id_, str) else id_)
    grad = torch.randn(n, generator=gen) * gscale
    runs = []
    for _ in range(2):
        buf = AdamBuffers(DEV, spec, p0, m0, v0, steps0, seg_of)
        assert buf.call(lib, grad, None) == 0
        runs.append(buf.state() + (buf.norm.cpu(),))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


def adam_nan_gradient(lib, DEV):
    """One NaN in an active segment: norm_out is not finite and the frozen segment stays bit-identical.  (What happens to the other
    active elements is the kernel's own and differs from torch: DESIGN section 2.)  Returns how many elements of p are finite."""
    spec, gen, n, n_seg, seg_of, gscale, p0, m0, v0, steps0 = _adam_problem(
        dict(sizes=[7, 300, 41], state="random", steps0=[2, 5, 1], seed=91))
    grad = torch.randn(n, generator=gen)
    grad[320] = math.nan
    buf = AdamBuffers(DEV, spec, p0, m0, v0, steps0, seg_of)
    assert buf.call(lib, grad, torch.tensor([1.0, 0.0, 1.0])) == 0
    p, m, v, steps = buf.state()
    assert not math.isfinite(float(buf.norm.cpu()))
    for got, was in ((p, p0), (m, m0), (v, v0)):
        assert torch.equal(_bits(got[7:307]), _bits(was[7:307]))
    assert steps.tolist() == [3.0, 5.0, 2.0]
    buf.assert_guards("nan")
    return int(torch.isfinite(p).sum())


def adam_anchor():
    """The restatement against torch itself, float64 against float64: clip_grad_norm_ + torch.optim.Adam on float64 parameters with
    the float32-rounded betas, three segments, four steps, the middle one frozen for the first two, weight decay on.  Returns the
    largest relative difference over p, exp_avg, exp_avg_sq, the norms and the step counts."""
    gen = torch.Generator().manual_seed(8)
    sizes = [7, 300, 41]
    sc = _adam_scalars(dict(ADAM_SCALARS, lr=2e-3, wd=1e-2, clip=1.5))
    refs = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64) * 1e-2) for s in sizes]
    opt = torch.optim.Adam(refs, lr=sc["lr"], betas=(sc["beta1"], sc["beta2"]), eps=sc["eps"], weight_decay=sc["wd"])
    seg_of = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    n = sum(sizes)
    state = (torch.cat([r.detach().clone() for r in refs]), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
             torch.zeros(3, dtype=torch.float64))
    worst = 0.0
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    for it in range(4):
        active = torch.tensor([True, it >= 2, True])
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 3 for s in sizes]
        for r, gr, a in zip(refs, grads, active):
            r.grad = gr.clone() if a else None
        total = torch.nn.utils.clip_grad_norm_(refs, sc["clip"])
        opt.step()
        state = adam_restated(*state[:4], torch.cat(grads), seg_of, active, sc, torch.float64)
        worst = max(worst, abs(float(state[4]) - float(total)) / float(total))
        live = [r for r, a in zip(refs, [True, it >= 2, True]) if a]
        worst = max(worst, rel(state[0], torch.cat([r.detach() for r in refs])))
        for k, mine in (("exp_avg", state[1]), ("exp_avg_sq", state[2])):
            theirs = torch.cat([opt.state[r][k] if r in opt.state and k in opt.state[r] else torch.zeros_like(r) for r in refs])
            worst = max(worst, rel(mine, theirs))
        assert [float(opt.state[r]["step"]) for r in live] == [float(s) for s, a in zip(state[3], active) if a]
    assert state[3].tolist() == [4.0, 2.0, 4.0]
    return worst


def beta2_constant_gap():
    """exp_avg_sq after one step of torch.optim.Adam in float32 against a float64 Adam with the float32-rounded beta2: the relative
    difference (1.30e-5) is the constant (1 - beta2), float32(0.001) in torch and 1 - float32(0.999) in the kernel."""
    gen = torch.Generator().manual_seed(2)
    p = torch.nn.Parameter(torch.randn(5000, generator=gen) * 1e-2)
    p.grad = torch.randn(5000, generator=gen)
    opt = torch.optim.Adam([p], lr=1e-3)
    opt.step()
    want = (1.0 - F32(0.999)) * p.grad.double() ** 2
    return float(((opt.state[p]["exp_avg_sq"].double() - want).abs() / want).max())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. kvae_loss_head_fwd / bwd
# ---------------------------------------------------------------------------------------------------------------------------
HEAD_W = dict(beta=0.7, scale=0.3, vae_w=1.5, kf_w=0.8)
HEAD_KEYS = ("head.recon", "head.reg", "head.vae", "head.tot", "head.coef", "head.g")


def head_inputs(n, mask, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    lpx, regf, kf = torch.randn(n, generator=gen) * 50, torch.randn(n, generator=gen), torch.randn((), generator=gen)
    mk = {None: None, "random": (torch.rand(n, generator=gen) < 0.7).float(), "ones": torch.ones(n), "zeros": torch.zeros(n)}[mask]
    return lpx, regf, kf, mk


def head_restated(lpx, regf, kf, mk, g_loss, dtype, beta=HEAD_W["beta"], scale=HEAD_W["scale"], vae_w=HEAD_W["vae_w"], kf_w=HEAD_W["kf_w"]):
    """The scalar head (parity_cases.py:1030-1036) and its gradients in `dtype`, every weight rounded through float32 first."""
    t = lambda x: torch.tensor(F32(x), dtype=dtype)
    L, R, K = lpx.to(dtype), regf.to(dtype), kf.to(dtype)
    m = torch.ones_like(L) if mk is None else mk.to(dtype)
    denom = m.sum().clamp(min=1.0)
    recon, reg = (L * m).sum() / denom, (R * m).sum() / denom
    vae = t(scale) * recon + t(beta) * reg
    tot = t(vae_w) * vae + t(kf_w) * K
    coef = torch.stack([-t(vae_w) * t(scale) / denom, -t(vae_w) * t(beta) / denom, t(kf_w)])
    g = t(g_loss)
    return dict(out=torch.stack([-tot, tot, K, vae, recon, reg]), coef=coef, g_lpx=g * coef[0] * m, g_regf=g * coef[1] * m,
                g_kf=-coef[2] * g)


def head_scales(lpx, regf, kf, mk, beta=HEAD_W["beta"], scale=HEAD_W["scale"], vae_w=HEAD_W["vae_w"], kf_w=HEAD_W["kf_w"]):
    """What each scalar's error is taken relative to: the float64 sum of the absolute contributions it is built from."""
    L, R = lpx.double(), regf.double()
    m = torch.ones_like(L) if mk is None else mk.double()
    denom = float(m.sum().clamp(min=1.0))
    recon, reg = float((L * m).abs().sum()) / denom, float((R * m).abs().sum()) / denom
    vae = abs(F32(scale)) * recon + abs(F32(beta)) * reg
    return {"head.recon": recon, "head.reg": reg, "head.vae": vae, "head.tot": abs(F32(vae_w)) * vae + abs(F32(kf_w) * float(kf))}


def _head_compare(what, got, ref, scales, bars, worst):
    """got / ref: dicts of head_restated's keys (got in float32).  kf passes through exactly."""
    o, r = got["out"].double(), ref["out"]
    assert float(got["out"][2]) == float(ref["out"][2]), (what, "elbo_kf")
    assert float(o[0]) == -float(o[1]), (what, "loss != -elbo_total")
    rat = lambda e, s: 0.0 if e == 0.0 else e / max(s, 1e-300)
    found = {"head.tot": rat(abs(float(o[1] - r[1])), scales["head.tot"]), "head.vae": rat(abs(float(o[3] - r[3])), scales["head.vae"]),
             "head.recon": rat(abs(float(o[4] - r[4])), scales["head.recon"]), "head.reg": rat(abs(float(o[5] - r[5])), scales["head.reg"]),
             "head.coef": float(((got["coef"].double() - ref["coef"]).abs() / ref["coef"].abs()).max())}
    worst_g = 0.0
    for k in ("g_lpx", "g_regf", "g_kf"):
        if got.get(k) is None:
            continue
        err, top = float((got[k].double() - ref[k]).abs().max()), float(ref[k].abs().max())
        worst_g = max(worst_g, rat(err, top))
    found["head.g"] = worst_g
    for k, v in found.items():
        v = math.inf if math.isnan(v) else v
        _note(worst, k, v)
        assert v < bars[k], (what, k, v, bars[k])


def head_case(lib, DEV, c, impl="kernel", bars=None, worst=None):
    """One case of HEAD_CASES through the C ABI: forward, then the backward fed with the forward's own coef."""
    bars = TOL if bars is None else bars
    n, mask, g_loss = c["n"], c.get("mask"), c.get("g_loss", 2.5)
    lpx, regf, kf, mk = head_inputs(n, mask, c.get("seed", n))
    ref = head_restated(lpx, regf, kf, mk, g_loss, torch.float64)
    scales = head_scales(lpx, regf, kf, mk)
    if impl == "f32":
        got = {k: v.float() for k, v in head_restated(lpx, regf, kf, mk, g_loss, torch.float32).items()}
        return _head_compare(c["id"], got, ref, scales, bars, worst)
    L, R = Guarded(DEV, n, c.get("off_lpx", 0), init=lpx), Guarded(DEV, n, c.get("off_regf", 0), init=regf)
    M = Guarded(DEV, n, c.get("off_mask", 0), init=mk) if mk is not None else None
    out, coef, g_kf = Guarded(DEV, 6), Guarded(DEV, 3), Guarded(DEV, 1)
    g_lpx, g_regf = Guarded(DEV, n), Guarded(DEV, n)
    dev = lambda x: torch.tensor([F32(v) for v in x], device=DEV)
    kf_d, beta_d, g_d = kf.reshape(1).to(DEV), dev([HEAD_W["beta"]]), dev([g_loss])
    w_dev = dev([HEAD_W["vae_w"], HEAD_W["kf_w"]]) if c.get("w_dev") else None
    by_value = (1e30, -7.0) if w_dev is not None else (F32(HEAD_W["vae_w"]), F32(HEAD_W["kf_w"]))   # garbage when w_dev is given
    rc = lib.dll.kvae_loss_head_fwd(L.ptr, R.ptr, M.ptr if M else None, _p(kf_d), _p(beta_d), F32(HEAD_W["scale"]), *by_value,
                                    _p(w_dev), out.ptr, coef.ptr, n, None)
    assert rc == 0, c["id"]
    rc = lib.dll.kvae_loss_head_bwd(_p(g_d), coef.ptr, M.ptr if M else None, g_lpx.ptr, g_regf.ptr, g_kf.ptr, n, None)
    assert rc == 0, c["id"]
    _sync(DEV)
    for k, b in (("out", out), ("coef", coef), ("g_kf", g_kf), ("g_lpx", g_lpx), ("g_regf", g_regf), ("lpx", L), ("regf", R)):
        assert b.guards_intact(), (c["id"], k, "written outside the operand")
    got = dict(out=out.cpu(), coef=coef.cpu(), g_lpx=g_lpx.cpu(), g_regf=g_regf.cpu(), g_kf=g_kf.cpu().reshape(()))
    if mask == "zeros":      # denom = 1, both means 0, every gradient 0
        assert float(got["out"][4]) == 0.0 and float(got["out"][5]) == 0.0 and float(got["out"][3]) == 0.0
        assert float(got["g_lpx"].abs().max()) == 0.0 and float(got["g_regf"].abs().max()) == 0.0
    return _head_compare(c["id"], got, ref, scales, bars, worst)


def _head_cases():
    out = []
    # 4096 = one float4 per thread, 4100 a second round of the vector loop, an odd n the scalar loop only
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4092, 4096, 4100, 4097, 12800):
        for mask in (None, "random", "ones", "zeros"):
            out.append(dict(id=f"n{n}-{mask}", n=n, mask=mask, g_loss=1.0 if mask == "ones" else 2.5))
    # misaligned inputs at a multiple of four: the scalar path, every frame still summed
    out.append(dict(id="n4096-lpx-offset", n=4096, mask="random", off_lpx=1))
    out.append(dict(id="n4096-regf-offset", n=4096, mask=None, off_regf=1))
    out.append(dict(id="n4096-mask-offset", n=4096, mask="random", off_mask=1))
    # device weights: the by-value pair is garbage and must be ignored
    out.append(dict(id="n4096-w-dev", n=4096, mask="random", w_dev=True))
    out.append(dict(id="n1025-w-dev", n=1025, mask=None, w_dev=True))
    return out


HEAD_CASES = _head_cases()
HEAD_IDS = [c["id"] for c in HEAD_CASES]
HEAD_BWD_N = 256 * 32 * 256 + 3   # past epi_grid's 8192 blocks: the grid-stride round of k_loss_head_bwd


def head_bwd_large(lib, DEV, impl="kernel", bars=None, worst=None, n=HEAD_BWD_N):
    """The backward alone at n = 2097155 with a coef of the test's own: every element, the last three included.  (n: the emulated
    tier lowers epi_grid's cap and runs the same rounds at a few thousand elements.)"""
    bars = TOL if bars is None else bars
    gen = torch.Generator().manual_seed(77)
    mk = (torch.rand(n, generator=gen) < 0.7).float()
    coef, g = torch.tensor([-3.25e-4, -7.5e-3, 0.8]), torch.tensor([2.5])
    ref = {k: g.double()[0] * coef.double()[i] * mk.double() for i, k in enumerate(("g_lpx", "g_regf"))}
    ref["g_kf"] = -coef.double()[2] * g.double()[0]
    if impl == "f32":
        got = dict(g_lpx=g[0] * coef[0] * mk, g_regf=g[0] * coef[1] * mk, g_kf=-coef[2] * g[0])
    else:
        M, g_lpx, g_regf, g_kf = Guarded(DEV, n, init=mk), Guarded(DEV, n), Guarded(DEV, n), Guarded(DEV, 1)
        g_d, coef_d = g.to(DEV), coef.to(DEV)
        rc = lib.dll.kvae_loss_head_bwd(_p(g_d), _p(coef_d), M.ptr, g_lpx.ptr, g_regf.ptr, g_kf.ptr, n, None)
        _sync(DEV)
        assert rc == 0
        assert g_lpx.guards_intact() and g_regf.guards_intact() and g_kf.guards_intact() and M.guards_intact()
        got = dict(g_lpx=g_lpx.cpu(), g_regf=g_regf.cpu(), g_kf=g_kf.cpu().reshape(()))
    for k in ref:
        err = (got[k].double() - ref[k]).abs()
        ratio = float(err.max() / ref[k].abs().max())
        _note(worst, "head.g", ratio)
        assert ratio < bars["head.g"], (k, ratio, int(err.argmax()) if err.dim() else 0)


def head_apply(DEV, transposed, beta_tensor, masked, weights_dev=False, impl="kernel", bars=None, worst=None):
    """LossHead.apply (its .contiguous(), its beta handling, its backward) against float64 autograd of the formula, upstream 2.0."""
    from kvae.vae.fused import LossHead
    bars = TOL if bars is None else bars
    B, T = 5, 13
    lpx, regf, kf, mk = head_inputs(B * T, "random" if masked else None, seed=B * T + transposed)
    shape = lambda x: x.view(T, B).t() if transposed else x.view(B, T)       # [B, T]; transposed: strides (1, B)
    mk2 = None if mk is None else shape(mk)
    ref_in = [shape(lpx).double().requires_grad_(True), shape(regf).double().requires_grad_(True), kf.double().requires_grad_(True)]
    m = torch.ones(B, T, dtype=torch.float64) if mk2 is None else mk2.double()
    w = {k: F32(v) for k, v in HEAD_W.items()}
    denom = m.sum().clamp(min=1.0)
    recon, reg = (ref_in[0] * m).sum() / denom, (ref_in[1] * m).sum() / denom
    vae = w["scale"] * recon + w["beta"] * reg
    tot = w["vae_w"] * vae + w["kf_w"] * ref_in[2]
    (-tot * 2.0).backward()
    ref = dict(out=torch.stack([-tot, tot, ref_in[2], vae, recon, reg]).detach(), g_lpx=ref_in[0].grad, g_regf=ref_in[1].grad,
               g_kf=ref_in[2].grad,
               coef=torch.stack([-w["vae_w"] * w["scale"] / denom, -w["vae_w"] * w["beta"] / denom, torch.tensor(w["kf_w"], dtype=torch.float64)]))
    scales = head_scales(lpx, regf, kf, mk)
    if impl == "f32":
        got = {k: v.float() for k, v in head_restated(lpx, regf, kf, mk, 2.0, torch.float32).items()}
        got["g_lpx"], got["g_regf"] = shape(got["g_lpx"]), shape(got["g_regf"])
        return _head_compare(("apply", transposed, masked), got, ref, scales, bars, worst)
    on_dev = lambda x: (x.view(T, B).to(DEV).t() if transposed else x.view(B, T).to(DEV)).requires_grad_(True)
    dev_in = [on_dev(lpx), on_dev(regf), kf.clone().to(DEV).requires_grad_(True)]
    assert dev_in[0].is_contiguous() != transposed
    beta = torch.tensor(w["beta"]).to(DEV) if beta_tensor else w["beta"]
    weights = (0.0, 0.0, torch.tensor([w["vae_w"], w["kf_w"]]).to(DEV)) if weights_dev else (w["vae_w"], w["kf_w"])
    out = LossHead.apply(dev_in[0], dev_in[1], dev_in[2], None if mk2 is None else on_dev(mk).detach(), beta, w["scale"], *weights)
    (out[0] * 2.0).backward()
    got = dict(out=torch.stack([o.detach() for o in out]).cpu(), g_lpx=dev_in[0].grad.cpu(), g_regf=dev_in[1].grad.cpu(),
               g_kf=dev_in[2].grad.cpu(), coef=ref["coef"].float())   # coef stays inside the Function: its use shows in the gradients
    assert got["g_lpx"].shape == (B, T)
    return _head_compare(("apply", transposed, beta_tensor, masked), got, ref, scales, bars, worst)


HEAD_APPLY_CASES = [(True, True, True), (True, False, False), (False, False, True), (False, True, False)]   # transposed, beta tensor, masked


# ---------------------------------------------------------------------------------------------------------------------------
# 3. column sums
# ---------------------------------------------------------------------------------------------------------------------------
# the eight waves' row strides and the 4-in-flight loop of colsum_v4_body (k_colsum: 4 row lanes, 2 in flight) at every remainder
COLSUM_ROWS = list(range(1, 10)) + [24, 25, 26, 31, 32, 33, 40, 57, 64, 100]
COLSUM_COLS = [1, 3, 4, 8, 63, 64, 65, 252, 256, 260, 1028]
COLSUM_PLACES = {"aligned": (0, 0), "input-offset": (1, 0), "output-offset": (0, 1)}   # floats past a 16-byte boundary: (input, output)
COLSUM2_CASES = [(33, 260, 7, 4), (9, 4, 57, 1028), (33, 260, 7, 3), (5, 63, 26, 8)]    # the last two: cols % 4 != 0, two launches
NATIVE_COLSUM_SHAPES = [(r, c) for r in (1023, 1024, 1030, 1031, 1088, 2048) for c in (3, 4, 36)] + [(1024, 4096)]
# equal tall heights | unequal tall heights | tall, no multiple of 64 | one tall and one short
NATIVE_PAIR_SHAPES = [(2048, 36, 2048, 4), (2048, 36, 1024, 4), (1030, 36, 1030, 4), (2048, 36, 100, 4), (100, 36, 100, 4)]
_POOL = {}


def _randn(rows, cols, seed=0):
    """[rows, cols] standard normal entries, a slice of one pool per seed (the reference inputs are drawn once)."""
    if seed not in _POOL:
        _POOL[seed] = torch.randn(2048 * 2048 + 64, generator=torch.Generator().manual_seed(4000 + seed))
    return _POOL[seed][:rows * cols].view(rows, cols)


def colsum_ratio(got, x):
    """Largest per-column error against x.double().sum(0), relative to sum_r |x[r, c]|."""
    x64 = x.double().reshape(x.shape[0], -1)
    r = (got.double().reshape(-1) - x64.sum(0)).abs() / x64.abs().sum(0)
    return float(r.max()), int(r.argmax())


def _colsum_check(what, got, x, bars, worst):
    ratio, col = colsum_ratio(got, x)
    ratio = math.inf if math.isnan(ratio) else ratio
    _note(worst, "colsum", ratio)
    assert ratio < bars["colsum"], (what, "column", col, ratio, bars["colsum"])


def colsum_abi(lib, DEV, cols, impl="kernel", bars=None, worst=None):
    """kvae_colsum at every row count of COLSUM_ROWS for one column count: 16-byte aligned (k_colsum_v4 when cols % 4 == 0) and
    with the input or the output one float further (k_colsum)."""
    bars = TOL if bars is None else bars
    for rows in COLSUM_ROWS:
        x = _randn(rows, cols, seed=cols % 7)
        if impl == "f32":
            _colsum_check((rows, cols), x.sum(0), x, bars, worst)
            continue
        for place, (oi, oo) in COLSUM_PLACES.items():
            X, out = Guarded(DEV, rows * cols, oi, init=x), Guarded(DEV, cols, oo)
            assert lib.dll.kvae_colsum(X.ptr, out.ptr, rows, cols, None) == 0
            _sync(DEV)
            assert out.guards_intact() and X.guards_intact(), (rows, cols, place, "written outside the output")
            _colsum_check((rows, cols, place), out.cpu(), x, bars, worst)


def colsum2_abi(lib, DEV, impl="kernel", bars=None, worst=None):
    """kvae_colsum2: both jobs aligned with unequal block counts (one launch), a job with cols % 4 != 0 (two launches), a
    misaligned operand (two launches), a NULL operand (KVAE_ERR_NULL, nothing written)."""
    bars = TOL if bars is None else bars
    for ra, ca, rb, cb in COLSUM2_CASES:
        for off in ((0, 0) if impl == "f32" else (0, 1)):
            a, b = _randn(ra, ca, seed=1), _randn(rb, cb, seed=2)
            if impl == "f32":
                _colsum_check((ra, ca), a.sum(0), a, bars, worst), _colsum_check((rb, cb), b.sum(0), b, bars, worst)
                break
            A, Bx, oa, ob = Guarded(DEV, ra * ca, init=a), Guarded(DEV, rb * cb, init=b), Guarded(DEV, ca), Guarded(DEV, cb, off)
            assert lib.dll.kvae_colsum2(A.ptr, oa.ptr, ra, ca, Bx.ptr, ob.ptr, rb, cb, None) == 0
            _sync(DEV)
            assert oa.guards_intact() and ob.guards_intact(), ((ra, ca, rb, cb), "written outside the outputs")
            _colsum_check((ra, ca, "a"), oa.cpu(), a, bars, worst), _colsum_check((rb, cb, "b"), ob.cpu(), b, bars, worst)
    if impl == "f32":
        return
    a, b = _randn(9, 4, seed=1), _randn(7, 8, seed=2)
    for missing in range(4):
        A, Bx, oa, ob = Guarded(DEV, 36, init=a), Guarded(DEV, 56, init=b), Guarded(DEV, 4), Guarded(DEV, 8)
        ptrs = [A.ptr, oa.ptr, Bx.ptr, ob.ptr]
        ptrs[missing] = None
        assert lib.dll.kvae_colsum2(ptrs[0], ptrs[1], 9, 4, ptrs[2], ptrs[3], 7, 8, None) == KVAE_ERR_NULL, missing
        _sync(DEV)
        assert oa.untouched() and ob.untouched(), (missing, "a refused call wrote")


def native_colsum(DEV, rows, cols, impl="kernel", bars=None, worst=None):
    """_native.colsum: the two-pass folding [r1, rows / r1 * cols] -> [rows / r1, cols] of tall inputs (r1 = 2 at 1030, none at the
    prime 1031, none for a wide input)."""
    from kvae import _native
    bars = TOL if bars is None else bars
    x = _randn(rows, cols, seed=3)
    got = x.sum(0) if impl == "f32" else _native.colsum(x.to(DEV)).cpu()
    assert got.shape == (cols,)
    _colsum_check((rows, cols), got, x, bars, worst)


def native_colsum_pair(DEV, ra, ca, rb, cb, impl="kernel", bars=None, worst=None):
    from kvae import _native
    bars = TOL if bars is None else bars
    a, b = _randn(ra, ca, seed=5), _randn(rb, cb, seed=6).view(rb, 2, cb // 2)
    sa, sb = (a.sum(0), b.sum(0)) if impl == "f32" else (t.cpu() for t in _native.colsum_pair(a.to(DEV), b.to(DEV)))
    assert sa.shape == a.shape[1:] and sb.shape == b.shape[1:]
    _colsum_check((ra, ca, "a"), sa, a, bars, worst), _colsum_check((rb, cb, "b"), sb, b, bars, worst)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. kvae_lgssm_emission_means
# ---------------------------------------------------------------------------------------------------------------------------
EMISSION_SHAPES = [(1, 1, 1, 1), (3, 7, 4, 2), (2, 5, 16, 2), (5, 13, 16, 16), (2, 3, 7, 3), (43, 3, 4, 2)]   # 43 * 3 * 2 = 258: a second block
EMISSION_LAYOUTS = ("shared", "per_step", "packed")


def emission_inputs(B, T, n, p, layout, seed=0):
    """(mus_smooth, mus_filt [B,T,n], C [B,T,p,n] as float32 values, and how the layout stores C: (C_view, packed, c_off))."""
    gen = torch.Generator().manual_seed(7000 + seed + 13 * B + T)
    ms, mf = torch.randn(B, T, n, generator=gen), torch.randn(B, T, n, generator=gen)
    if layout == "shared":
        Cm = torch.randn(p, n, generator=gen)
        return ms, mf, Cm.expand(B, T, p, n), (Cm, None, None)
    if layout == "per_step":
        Cm = torch.randn(B, T, p, n, generator=gen)
        return ms, mf, Cm, (Cm, None, None)
    E, off = p * n + 11, 5                                   # a packed step record with its own row stride; C starts at float 5
    packed = torch.randn(B, T, E, generator=gen)
    Cm = packed[..., off:off + p * n].reshape(B, T, p, n)
    return ms, mf, Cm, (Cm, packed, off)


def _emission_check(what, got_s, got_f, ms, mf, Cm, bars, worst):
    for name, got, mu in (("smooth", got_s, ms), ("filt", got_f, mf)):
        if got is None:
            continue
        ref = (Cm.double() @ mu.double().unsqueeze(-1)).squeeze(-1)
        ratio, where = _per_step_ratio(got, ref)
        ratio = math.inf if math.isnan(ratio) else ratio
        _note(worst, "emission", ratio)
        assert ratio < bars["emission"], (what, name, where, ratio, bars["emission"])


def emission_ops(DEV, B, T, n, p, layout, impl="kernel", bars=None, worst=None):
    """lgssm_ops.emission_means over the three layouts of the emission stack."""
    from kvae.kalman import lgssm_ops
    bars = TOL if bars is None else bars
    ms, mf, Cm, (view, packed, off) = emission_inputs(B, T, n, p, layout)
    if impl == "f32":
        a_s, a_f = torch.einsum("btpn,btn->btp", Cm, ms), torch.einsum("btpn,btn->btp", Cm, mf)
    else:
        packed_d = None if packed is None else packed.to(DEV)
        view_d = view.to(DEV) if packed is None else packed_d[..., off:off + p * n].reshape(B, T, p, n)
        a_s, a_f = lgssm_ops.emission_means(ms.unsqueeze(-1).to(DEV), mf.unsqueeze(-1).to(DEV), view_d, packed_d, off)
        assert a_s.shape == (B, T, p) and a_f.shape == (B, T, p)
        a_s, a_f = a_s.cpu(), a_f.cpu()
    _emission_check((B, T, n, p, layout), a_s, a_f, ms, mf, Cm, bars, worst)


def emission_abi(lib, DEV, B, T, n, p, bars=None, worst=None):
    """The C ABI with guarded outputs: both means, smoothed only, filtered only (the other output stays untouched)."""
    from kvae import _native as N
    bars = TOL if bars is None else bars
    ms, mf, Cm, _ = emission_inputs(B, T, n, p, "per_step", seed=1)
    Cd, msd, mfd = Cm.contiguous().to(DEV), ms.to(DEV), mf.to(DEV)
    prob = N.Problem()
    prob.B, prob.T, prob.n, prob.m, prob.p = B, T, n, n, p
    prob.C = N.Stack(Cd.data_ptr(), T * p * n, p * n)
    for want_s, want_f in ((True, True), (True, False), (False, True)):
        a_s, a_f = Guarded(DEV, B * T * p), Guarded(DEV, B * T * p)
        rc = lib.dll.kvae_lgssm_emission_means(C.byref(prob), _p(msd) if want_s else None, _p(mfd) if want_f else None,
                                               a_s.ptr if want_s else None, a_f.ptr if want_f else None, None)
        _sync(DEV)
        assert rc == 0, (want_s, want_f)
        assert a_s.guards_intact() and a_f.guards_intact(), "written outside the outputs"
        assert want_s or a_s.untouched()
        assert want_f or a_f.untouched()
        _emission_check((B, T, n, p, want_s, want_f), a_s.cpu().view(B, T, p) if want_s else None,
                        a_f.cpu().view(B, T, p) if want_f else None, ms, mf, Cm, bars, worst)


def emission_rejects(lib, DEV):
    """A mean without its output (or the reverse, or neither): KVAE_ERR_NULL; n = 17: KVAE_ERR_DIMS; nothing written."""
    from kvae import _native as N
    B, T, n, p = 2, 3, 4, 2
    ms, mf, Cm, _ = emission_inputs(B, T, 17, p, "per_step")
    Cd, msd, mfd = Cm.contiguous().to(DEV), ms.to(DEV), mf.to(DEV)
    a_s, a_f = Guarded(DEV, B * T * p), Guarded(DEV, B * T * p)
    prob = N.Problem()
    prob.B, prob.T, prob.n, prob.m, prob.p = B, T, n, n, p
    prob.C = N.Stack(Cd.data_ptr(), T * p * 17, p * 17)
    call = lambda s, f, os, of: lib.dll.kvae_lgssm_emission_means(C.byref(prob), s, f, os, of, None)
    assert call(_p(msd), _p(mfd), a_s.ptr, a_f.ptr) == 0
    a_s, a_f = Guarded(DEV, B * T * p), Guarded(DEV, B * T * p)
    assert call(_p(msd), _p(mfd), a_s.ptr, None) == KVAE_ERR_NULL
    assert call(_p(msd), None, a_s.ptr, a_f.ptr) == KVAE_ERR_NULL
    assert call(None, _p(mfd), a_s.ptr, a_f.ptr) == KVAE_ERR_NULL
    assert call(None, None, None, None) == KVAE_ERR_NULL
    prob.n = 17
    assert call(_p(msd), _p(mfd), a_s.ptr, a_f.ptr) == KVAE_ERR_DIMS
    prob.n, prob.p = n, 17
    assert call(_p(msd), _p(mfd), a_s.ptr, a_f.ptr) == KVAE_ERR_DIMS
    _sync(DEV)
    assert a_s.untouched() and a_f.untouched()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. kvae_bias_shuffle_act_fwd / bwd (csrc/vae_epilogue.h), per element through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
# Forward: one float32 add, a permutation and a select - `out` equals float32 torch on the CPU bit for bit.  Backward: g_in is a
# select and a permutation (bit for bit, and bit-repeatable); bias_partials [kvae_bias_partial_rows(N), C r^2] is zeroed by the call
# and summed with float atomics whose order is free, so it is compared, per row and summed over the rows, against float64 sums of
# the same elements relative to the sum of |g| (key epi.bias), with no repeatability assertion.
# (N, C, H, W, r), floats `in` / `out` sit past a 16-byte boundary, the kernel the gate of csrc/vae_epilogue.h picks
EPI_FWD_CASES = [
    ((3, 5, 3, 4, 1), 0, 0, "epi.fwd_v4<1>"),
    ((2, 3, 3, 2, 2), 0, 0, "epi.fwd_v4<2>"),      # W / 2 = 1: one quad per output row
    ((2, 3, 3, 6, 2), 0, 0, "epi.fwd_v4<2>"),      # three quads per output row
    ((2, 3, 3, 5, 1), 0, 0, "epi.fwd"),            # scalar by shape: W % 4 != 0
    ((2, 3, 3, 3, 2), 0, 0, "epi.fwd"),            # odd W at r = 2
    ((2, 3, 5, 7, 3), 0, 0, "epi.fwd"),            # r = 3
    ((3, 5, 3, 4, 1), 1, 0, "epi.fwd"),            # scalar by pointer: `in` 4 bytes past a 16-byte boundary
    ((2, 3, 3, 6, 2), 0, 1, "epi.fwd"),            # ... and `out`
    ((2, 65, 1, 2, 2), 0, 0, "epi.fwd_v4<2>"),     # 260 input channels
]
# total / 4 (v4) and total (scalar) just above epi_grid's 8192 x 256 with a ragged remainder: a second grid-stride round of 4 quads
# and of 28 elements.  With the cap lowered to 3 blocks (CPU tier): two full rounds of 768 and a third of 264.
EPI_STRIDE_CARD = [((174763, 2, 1, 6, 2), "epi.fwd_v4<2>"), ((233020, 1, 1, 1, 3), "epi.fwd")]
EPI_STRIDE_EMU = [((150, 2, 1, 6, 2), "epi.fwd_v4<2>"), ((200, 1, 1, 1, 3), "epi.fwd")]
# (N, C, H, W, r), relu, bias partials wanted, floats g_in sits past a 16-byte boundary
EPI_BWD_CASES = (
    [((n, 3, 2, 2, 2), 1, True, 0) for n in (1, 31, 32, 33, 65)]      # the 32-sample chunk: one short row, full rows, 1 + 1, 2 + 1
    + [((2, 3, 5, 7, 2), 1, True, 0),                                 # 420 positions per sample: a ragged second block
       ((2, 65, 1, 2, 2), 1, True, 0),                                # 260 channels: more bins than the 256 threads that zero them
       ((2, 65, 1, 2, 2), 0, True, 0),
       ((33, 3, 2, 2, 2), 0, True, 0),                                # relu = 0: `out` is NULL
       ((3, 5, 3, 4, 1), 1, True, 0), ((2, 3, 5, 7, 3), 1, True, 1),   # r = 1, r = 3 (g_in one float past the boundary)
       ((2, 3, 5, 7, 3), 1, False, 0), ((3, 5, 3, 4, 1), 0, False, 0), ((2, 3, 3, 3, 2), 1, False, 1)])   # k_vae_epilogue_bwd
EPI_BWD_STRIDE_CARD, EPI_BWD_STRIDE_EMU = (233020, 1, 1, 1, 3), (200, 1, 1, 1, 3)   # k_vae_epilogue_bwd past epi_grid's cap


def case_id(v):
    """A pytest id without blanks: (2, 3, 3, 6, 2) -> 2x3x3x6x2."""
    return "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


def epi_inputs(shape, seed=0):
    """x [N, C r^2, H, W] and bias [C r^2] of the forward; g and `out` [N, C, H r, W r] of the backward.  x holds three elements
    whose sum with the bias is exactly +0.0; `out` starts with +0.0, -0.0 and a NaN (the mask is out > 0)."""
    N, Cc, H, W, r = shape
    gen = torch.Generator().manual_seed(9000 + seed + 7 * N + W)
    x, b = torch.randn(N, Cc * r * r, H, W, generator=gen), torch.randn(Cc * r * r, generator=gen)
    flat = x.view(N, Cc * r * r, -1)
    for ch in range(min(3, Cc * r * r)):
        flat[N - 1, ch, 0] = -b[ch]
    g, out = torch.randn(N, Cc, H * r, W * r, generator=gen), torch.randn(N, Cc, H * r, W * r, generator=gen)
    o = out.view(-1)
    o[0], o[1], o[2] = 0.0, -0.0, math.nan
    return x, b, g, out


def epi_fwd_case(lib, DEV, shape, off_in=0, off_out=0):
    """Both values of relu: `out` bit for bit against torch (pixel_shuffle(x + b), then relu), the sentinels around it intact, the
    input untouched."""
    N, Cc, H, W, r = shape
    x, b, _, _ = epi_inputs(shape)
    pre = torch.nn.functional.pixel_shuffle(x + b.view(1, -1, 1, 1), r)
    b_d = b.to(DEV)
    X = Guarded(DEV, x.numel(), off_in, init=x)
    for relu in (0, 1):
        ref = torch.relu(pre) if relu else pre
        out = Guarded(DEV, x.numel(), off_out)
        rc = lib.dll.kvae_bias_shuffle_act_fwd(X.ptr, _p(b_d), out.ptr, N, Cc, H, W, r, relu, None)
        _sync(DEV)
        assert rc == 0, (shape, relu)
        assert out.guards_intact() and X.guards_intact(), (shape, relu, "written outside the output")
        got = out.cpu()
        same = _bits(got) == _bits(ref.reshape(-1))
        assert bool(same.all()), (shape, relu, off_in, off_out, "first differing element", int((~same).int().argmax()),
                                  int((~same).sum()))
        assert torch.equal(_bits(X.cpu()), _bits(x.reshape(-1))), (shape, "the input was written")


def _epi_bias_ratios(rows, ref_in, per_chunk):
    """Largest |err| / sum |g| per (partial row, channel) and per channel over all rows; rows: [R, Cin] (float32 or float64 sums),
    ref_in: the float32 values of g_in [N, Cin, H, W]."""
    N = ref_in.shape[0]
    g64 = ref_in.double()
    worst = 0.0
    tot_ref, tot_abs = g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3))
    parts = [(rows.double().sum(0), tot_ref, tot_abs)]
    for k in range(rows.shape[0]):
        chunk = g64[k * per_chunk:min((k + 1) * per_chunk, N)]
        parts.append((rows[k].double(), chunk.sum((0, 2, 3)), chunk.abs().sum((0, 2, 3))))
    for got, ref, mag in parts:
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / mag.clamp_min(1e-300))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        worst = max(worst, float(ratio.max()))
    return worst


def epi_bwd_case(lib, DEV, shape, relu, want_bias, off=0, per_chunk=32, impl="kernel", bars=None, worst=None):
    """g_in bit for bit against torch (pixel_unshuffle of g where out > 0) and bit-repeatable over two calls; bias_partials of exactly
    kvae_bias_partial_rows(N) x C r^2 floats, pre-filled with the sentinel (the call zeroes it), under the epi.bias bar; the guards
    around both intact.  impl "f32": the float32 torch sums of the same elements (the yardstick)."""
    bars = TOL if bars is None else bars
    N, Cc, H, W, r = shape
    Cin = Cc * r * r
    _, _, g, out = epi_inputs(shape, seed=1)
    masked = torch.where(out > 0, g, torch.zeros(())) if relu else g
    ref_in = torch.nn.functional.pixel_unshuffle(masked, r)
    assert ref_in.shape == (N, Cin, H, W)
    rows = (N + per_chunk - 1) // per_chunk
    if impl == "f32":
        if want_bias:
            f32 = torch.stack([ref_in[k * per_chunk:(k + 1) * per_chunk].sum((0, 2, 3)) for k in range(rows)])
            _note(worst, "epi.bias", _epi_bias_ratios(f32, ref_in, per_chunk))
        return
    assert lib.dll.kvae_bias_partial_rows(N) == rows, (N, per_chunk)
    g_d, out_d = g.to(DEV), (out.to(DEV) if relu else None)
    runs = []
    for _ in range(2):
        G = Guarded(DEV, g.numel(), off)
        BP = Guarded(DEV, rows * Cin) if want_bias else None
        rc = lib.dll.kvae_bias_shuffle_act_bwd(_p(g_d), _p(out_d), G.ptr, BP.ptr if BP else None, N, Cc, H, W, r, relu, None)
        _sync(DEV)
        assert rc == 0, (shape, relu, want_bias)
        assert G.guards_intact(), (shape, relu, want_bias, "written outside g_in")
        got = G.cpu()
        same = _bits(got) == _bits(ref_in.reshape(-1))
        assert bool(same.all()), (shape, relu, want_bias, "g_in: first differing element", int((~same).int().argmax()), int((~same).sum()))
        if want_bias:
            assert BP.guards_intact(), (shape, relu, "written outside bias_partials")
            ratio = _epi_bias_ratios(BP.cpu().view(rows, Cin), ref_in, per_chunk)
            _note(worst, "epi.bias", ratio)
            assert ratio < bars["epi.bias"], (shape, relu, "epi.bias", ratio, bars["epi.bias"])
        runs.append(got)
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), (shape, "g_in is not repeatable")
    assert torch.equal(_bits(g_d.cpu()), _bits(g)), (shape, "g_out was written")


def epi_rejects(lib, DEV):
    """NULL operands (KVAE_ERR_NULL; for the backward `out` only with relu), any extent below 1 (KVAE_ERR_ARG): nothing written."""
    shape = (2, 3, 3, 2, 2)
    N, Cc, H, W, r = shape
    x, b, g, out = epi_inputs(shape)
    n, Cin = x.numel(), Cc * r * r
    x_d, b_d, g_d, out_d = x.to(DEV), b.to(DEV), g.to(DEV), out.to(DEV)
    O, G, BP = Guarded(DEV, n), Guarded(DEV, n), Guarded(DEV, Cin)
    fwd, bwd = lib.dll.kvae_bias_shuffle_act_fwd, lib.dll.kvae_bias_shuffle_act_bwd
    assert fwd(None, _p(b_d), O.ptr, N, Cc, H, W, r, 1, None) == KVAE_ERR_NULL
    assert fwd(_p(x_d), None, O.ptr, N, Cc, H, W, r, 1, None) == KVAE_ERR_NULL
    assert fwd(_p(x_d), _p(b_d), None, N, Cc, H, W, r, 1, None) == KVAE_ERR_NULL
    assert bwd(None, _p(out_d), G.ptr, BP.ptr, N, Cc, H, W, r, 1, None) == KVAE_ERR_NULL
    assert bwd(_p(g_d), _p(out_d), None, BP.ptr, N, Cc, H, W, r, 1, None) == KVAE_ERR_NULL
    assert bwd(_p(g_d), None, G.ptr, BP.ptr, N, Cc, H, W, r, 1, None) == KVAE_ERR_NULL      # relu needs `out`
    for k in range(5):
        for bad in (0, -1):
            ext = [N, Cc, H, W, r]
            ext[k] = bad
            assert fwd(_p(x_d), _p(b_d), O.ptr, *ext, 1, None) == KVAE_ERR_ARG, ext
            assert bwd(_p(g_d), _p(out_d), G.ptr, BP.ptr, *ext, 1, None) == KVAE_ERR_ARG, ext
    _sync(DEV)
    assert O.untouched() and G.untouched() and BP.untouched(), "a refused call wrote"
    assert bwd(_p(g_d), None, G.ptr, BP.ptr, N, Cc, H, W, r, 0, None) == 0                  # ... and only with relu
    _sync(DEV)
    assert G.guards_intact() and BP.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------
def yardsticks():
    """The float32 torch restatements against the float64 references over every case list: the numbers YARDSTICK holds."""
    worst = {}
    free = {k: math.inf for k in YARDSTICK}
    for c in ADAM_CASES:
        adam_case(None, "cpu", c, impl="f32", bars=free, worst=worst)
    for c in HEAD_CASES:
        head_case(None, "cpu", c, impl="f32", bars=free, worst=worst)
    head_bwd_large(None, "cpu", impl="f32", bars=free, worst=worst)
    for tr, bt, mk in HEAD_APPLY_CASES:
        head_apply("cpu", tr, bt, mk, impl="f32", bars=free, worst=worst)
    for cols in COLSUM_COLS:
        colsum_abi(None, "cpu", cols, impl="f32", bars=free, worst=worst)
    colsum2_abi(None, "cpu", impl="f32", bars=free, worst=worst)
    for r, c in NATIVE_COLSUM_SHAPES:
        native_colsum("cpu", r, c, impl="f32", bars=free, worst=worst)
    for s in NATIVE_PAIR_SHAPES:
        native_colsum_pair("cpu", *s, impl="f32", bars=free, worst=worst)
    for B, T, n, p in EMISSION_SHAPES:
        for layout in EMISSION_LAYOUTS:
            emission_ops("cpu", B, T, n, p, layout, impl="f32", bars=free, worst=worst)
    for shape, relu, want_bias, off in EPI_BWD_CASES:
        epi_bwd_case(None, "cpu", shape, relu, want_bias, off, impl="f32", bars=free, worst=worst)
    return worst


if __name__ == "__main__":
    torch.set_num_threads(4)
    print("YARDSTICK =", {k: float(f"{v:.3g}") for k, v in yardsticks().items()})
    print(f"adam_anchor() = {adam_anchor():.3g}   beta2_constant_gap() = {beta2_constant_gap():.3g}")
