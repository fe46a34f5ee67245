"""CPU tier: the entry points that apply a ReLU mask where the gradient is made, on the plain-loop twins of tests/hostsim
(csrc/vae_loss.h under KVAE_HOSTSIM), and the plan by which Decoder._decode pairs them (kvae.vae.fused.premask_plan).
Cases: tests/dec_premask_cases.py."""
import pytest
import torch

import dec_premask_cases as P
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)


@pytest.fixture(scope="module", autouse=True)
def hostsim_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    _native._set_test_backend(lib)
    yield lib
    _native._set_test_backend(None)


@pytest.mark.parametrize("loss", (False, True), ids=("plain", "bernoulli"))
@pytest.mark.parametrize("N", P.HEAD_N[:2])
def test_head_masks_its_data_gradient_hostsim(N, loss):
    P.head_case("cpu", N, loss)


@pytest.mark.parametrize("side,N", [(8, n) for n in P.UP8_N[:2]] + [(4, n) for n in P.UP4_N[:2]])
def test_up_takes_a_premasked_gradient_hostsim(side, N):
    P.up_case("cpu", N, side, out_is_unread=False)   # the twin masks by `out` again (no bit changes): it does read it


def test_premask_refusals_hostsim():
    P.refusals("cpu")


def test_plan_pairs_producer_and_consumer(monkeypatch):
    from kvae.vae.fused import premask_plan
    monkeypatch.delenv("KVAE_PREMASK", raising=False)
    assert premask_plan(["up", "up", "head"]) == [(True, False), (True, True), (False, True)]
    assert premask_plan(["block", "up", "head"]) == [(False, False), (True, False), (False, True)]
    assert premask_plan(["up", "block", "head"]) == [(False, False)] * 3      # a neighbour that is not a fused kernel
    assert premask_plan(["up", "up", "block"]) == [(True, False), (False, True), (False, False)]
    assert premask_plan(["head"]) == [(False, False)] and premask_plan([]) == []
    for kinds in (["up", "up", "head"], ["up", "head"], ["up", "up", "up", "head"]):
        plan = premask_plan(kinds)
        assert all(plan[i][0] == plan[i + 1][1] for i in range(len(kinds) - 1)), "both sides of a pair, or neither"
        assert not plan[0][1] and not plan[-1][0]
    monkeypatch.setenv("KVAE_PREMASK", "0")
    assert premask_plan(["up", "up", "head"]) == [(False, False)] * 3
    monkeypatch.setenv("KVAE_PREMASK", "head")
    assert premask_plan(["up", "up", "head"]) == [(False, False), (True, False), (False, True)]


def _decode_calls(monkeypatch, premask, x_frames=True, unsupported_head=False):
    """Run the default decoder forward + backward on the twins; returns (gradients, the non-tensor arguments each Function got)."""
    from kvae.utils.config import KVAEConfig
    from kvae.vae import fused
    from kvae.vae.vae import Decoder
    if premask is None:
        monkeypatch.delenv("KVAE_PREMASK", raising=False)
    else:
        monkeypatch.setenv("KVAE_PREMASK", premask)
    calls = []
    for cls in (fused.DecoderUp, fused.DecoderHead, fused.DecoderHeadBernoulli):
        def spy(*a, _cls=cls, _real=cls.apply):
            calls.append((_cls.__name__, tuple(v for v in a if not torch.is_tensor(v))))
            return _real(*a)
        monkeypatch.setattr(cls, "apply", spy)
    if unsupported_head:
        monkeypatch.setattr(fused.DecoderHead, "supported", staticmethod(lambda h, conv: False))
    torch.manual_seed(5)
    dec = Decoder(KVAEConfig())
    g = torch.Generator().manual_seed(9)
    a = torch.randn(2, 2, generator=g).requires_grad_(True)
    x = (torch.rand(2, 1, 32, 32, generator=g) < 0.2).float()
    if x_frames:
        logits, _, ll = dec.forward_with_frames(a, x, with_recon=False)
        (ll * torch.randn(2, generator=g)).sum().backward()
    else:
        (dec(a) * torch.randn(2, 1, 32, 32, generator=g)).sum().backward()
    grads = {"a": a.grad.clone(), **{k: p.grad.clone() for k, p in dec.named_parameters()}}
    return grads, calls


@pytest.mark.parametrize("x_frames", (True, False), ids=("bernoulli_head", "plain_head"))
def test_decode_hands_the_plan_to_both_sides(monkeypatch, x_frames):
    """Default decoder: up 4 -> up 8 -> head, all fused.  up 4 takes a pre-masked gradient; up 8 takes one and masks its own; the
    head masks its own.  KVAE_PREMASK=0 hands out no flag at all, and the gradients are the same bits."""
    on, calls = _decode_calls(monkeypatch, None, x_frames)
    head = "DecoderHeadBernoulli" if x_frames else "DecoderHead"
    assert [c[0] for c in calls] == ["DecoderUp", "DecoderUp", head]
    assert calls[0][1] == (True, False) and calls[1][1] == (True, True)
    assert calls[2][1] == ((False, True) if x_frames else (True,))        # (with_recon, mask_gh) / (mask_gh,)
    off, calls0 = _decode_calls(monkeypatch, "0", x_frames)
    assert [c[1] for c in calls0] == [(False, False), (False, False), (False, False) if x_frames else (False,)]
    assert set(on) == set(off) and len(on) >= 9
    for k in on:
        assert torch.equal(on[k], off[k]), k


def test_a_neighbour_that_is_not_fused_keeps_the_mask_in_the_producer(monkeypatch):
    """The head falls back to conv_block: up 8 must mask its own gradient again (no G_PREMASKED), the pair below it stays."""
    _, calls = _decode_calls(monkeypatch, None, x_frames=False, unsupported_head=True)
    assert [c for c in calls] == [("DecoderUp", (True, False)), ("DecoderUp", (False, True))]
