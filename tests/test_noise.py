"""kvae.noise.normal / gumbel: the injected tensor of a slot moved, cast and reshaped, else the fresh draw the call sites made."""
import pytest
import torch

from kvae import noise


@pytest.mark.parametrize("fn,slot", [(noise.normal, "gen_z"), (noise.gumbel, "gen_gumbel")])
def test_injected_tensor_is_cast_and_reshaped(fn, slot):
    v = torch.arange(24, dtype=torch.float64)
    with noise.inject(**{slot: v}):
        out = fn(slot, (2, 3, 4), torch.device("cpu"), torch.float32)
        assert out.dtype == torch.float32 and out.shape == (2, 3, 4) and out.device.type == "cpu"
        assert torch.equal(out, v.float().reshape(2, 3, 4))
        assert noise.take(slot) is v   # the slot keeps its tensor for the whole context
        with pytest.raises(RuntimeError):
            fn(slot, (2, 3, 5), torch.device("cpu"), torch.float32)   # 30 elements asked of 24
    assert noise.take(slot) is None


def test_fresh_draws_are_the_torch_calls_they_replace():
    dev = torch.device("cpu")
    torch.manual_seed(5)
    want = (torch.randn(2, 3, 4, device=dev, dtype=torch.float64), torch.randn_like(torch.empty(6, 2)),
            -torch.empty(2, 3, 4, device=dev, dtype=torch.float32).exponential_().log(), torch.randn(1))
    torch.manual_seed(5)
    got = (noise.normal("post_z", (2, 3, 4), dev, torch.float64), noise.normal("eps_a", torch.Size([6, 2]), dev, torch.float32),
           noise.gumbel("gumbel", (2, 3, 4), dev, torch.float32), torch.randn(1))   # the last: the generator is where it was
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(want, got))
