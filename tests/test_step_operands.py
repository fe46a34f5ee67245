"""StepOperands (kvae/kalman/operands.py): a record-backed and a plain bundle own their views by identity and hand out the operand
forms lgssm_ops takes; the switching dynamics expose their step record through packed_record() until reset_state()."""
import torch

from hostsim.build import build as build_hostsim
from kvae.kalman.lgssm_ops import Slots, alpha_lstm_slots, slot_view
from kvae.kalman.operands import NO_PASS, StepOperands

n, m, p = 4, 3, 2
R, mu0, Sigma0 = torch.eye(p), torch.zeros(n), torch.eye(n)


def same(got, want):
    return len(got) == len(want) and all(a == b if isinstance(b, Slots) else a is b for a, b in zip(got, want))


def test_record_backed_bundle():
    slots, E = alpha_lstm_slots(n, m, p)
    rec, Q = torch.randn(2, 3, E), torch.eye(n)
    views = (slot_view(rec, slots.A, n, n), slot_view(rec, slots.B, n, m), slot_view(rec, slots.C, p, n))
    ops = StepOperands.packed(rec, slots, list(views), Q=Q)
    assert same(ops.views, views) and ops.owns(*views)
    assert not ops.owns(views[0], views[1], views[2].clone())   # equal values, another tensor
    assert not ops.owns(*(slot_view(rec, o, r, c) for o, r, c in ((slots.A, n, n), (slots.B, n, m), (slots.C, p, n))))
    assert same(ops.emission(), (views[2], rec, Slots(C=slots.C))) and same(ops.emission(views[2]), ops.emission())
    other = views[2].clone()
    assert same(ops.emission(other), (other, None, Slots()))
    assert ops.transition_noise() is Q
    assert same(ops.posterior(), (views[0], views[2], Q, rec, Slots(A=slots.A, C=slots.C)))
    assert same(ops.lgssm(R, mu0, Sigma0), (rec, None, None, None, Q, R, mu0, Sigma0, slots))
    # the switching model's layout: A | B | Q packed, one shared C beside the record
    sw, C = Slots(A=0, B=n * n, Q=n * n + n * m), torch.randn(p, n)
    rec = torch.randn(2, 3, 2 * n * n + n * m)
    views = (slot_view(rec, sw.A, n, n), slot_view(rec, sw.B, n, m), C.expand(2, 3, p, n))
    Q_view = slot_view(rec, sw.Q, n, n)
    ops = StepOperands.packed(rec, sw, views, C=C, Q_view=Q_view)
    assert same(ops.emission(), (C, rec, Slots())) and ops.transition_noise() is Q_view
    assert same(ops.posterior(), (views[0], C, Q_view, rec, Slots(A=sw.A, Q=sw.Q)))
    assert same(ops.lgssm(R, mu0, Sigma0), (rec, None, None, C, None, R, mu0, Sigma0, sw))


def test_plain_bundle():
    A, B, C, Q = torch.eye(n), torch.randn(n, m), torch.randn(p, n), torch.eye(n)
    views = tuple(M.expand(2, 3, -1, -1) for M in (A, B, C))
    ops = StepOperands.plain(A, B, C, Q, views=views)
    assert ops.owns(*views) and not ops.owns(*(M.expand(2, 3, -1, -1) for M in (A, B, C)))
    assert same(ops.emission(), (C, None, Slots())) and ops.transition_noise() is Q
    assert same(ops.posterior(), (views[0], C, Q, None, Slots()))
    assert same(ops.lgssm(R, mu0, Sigma0), (None, A, B, C, Q, R, mu0, Sigma0, Slots()))
    stacks = tuple(v.clone() for v in views)
    ops = StepOperands.plain(*stacks, Q)
    assert same(ops.views, stacks) and ops.owns(*stacks) and not ops.owns(*views)
    assert same(ops.emission(stacks[2]), (stacks[2], None, Slots()))
    assert not NO_PASS.owns(*stacks) and same(NO_PASS.emission(stacks[2]), (stacks[2], None, Slots()))


def test_switching_dynamics_hand_their_record_over():
    from kvae import _native
    from kvae.model.model import KVAE
    from kvae.utils.config import KVAEConfig
    _native._set_test_backend(_native.LgssmLib(build_hostsim()))
    try:
        torch.manual_seed(0)
        kf = KVAE(KVAEConfig(dynamics_model="switching", num_modes=3)).kalman_filter.eval()
        dyn = kf.dyn_params
        assert dyn.packed_record() is None
        with torch.no_grad():
            out = kf.filter(torch.randn(2, 5, kf.p), torch.zeros(2, 5, kf.m))
        rec, slots = dyn.packed_record()
        assert kf._last.record is rec and kf._last.slots == slots and None not in (slots.A, slots.B, slots.Q) and slots.C is None
        assert kf._last.owns(*out[4:]) and kf._last.transition_noise() is dyn.Q_seq
        dyn.reset_state()
        assert dyn.packed_record() is None
    finally:
        _native._set_test_backend(None)
