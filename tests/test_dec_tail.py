"""CPU tier: the decoder head with the Bernoulli term folded in, on the plain-loop twins of tests/hostsim (csrc/vae_loss.h under
KVAE_HOSTSIM) - the C ABI, the autograd Function and the routing of KVAE.forward / compute_loss.  Cases: tests/dec_tail_cases.py."""
import pytest
import torch

import dec_tail_cases as D
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)


@pytest.fixture(scope="module", autouse=True)
def hostsim_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    _native._set_test_backend(lib)
    yield lib
    _native._set_test_backend(None)


@pytest.mark.parametrize("N", D.TAIL_N)
def test_dec_tail_random_hostsim(N):
    print(D.tail_random("cpu", N))


@pytest.mark.parametrize("N", D.TAIL_N[:3])
def test_dec_tail_optional_outputs_hostsim(N):
    print(D.tail_optional_outputs("cpu", N))


@pytest.mark.parametrize("N", D.TAIL_N[:3])
def test_dec_tail_general_backward_hostsim(N):
    print(D.tail_general("cpu", N))


@pytest.mark.parametrize("kind,frame,pos", [(k, f, p) for k, P in (("x", D.PROBE_X), ("h", D.PROBE_H)) for f in D.PROBE_FRAMES for p in P])
def test_dec_tail_probe_hostsim(kind, frame, pos):
    print(D.tail_probe("cpu", kind, frame, pos))


def test_dec_tail_refusals_hostsim():
    D.tail_refusals("cpu")


def test_compute_loss_with_another_tensor_takes_the_fallback_hostsim():
    res = D.model_other_tensor("cpu")
    print(res)
    # smoke()'s bars for a whole float32 model against the oracle: 1e-4 on values, 1e-3 on gradients
    assert res["loss"] < 1e-4 and res["loss_same"] < 1e-4 and res["recon"] < 1e-4 and res["grad_head"] < 1e-3 and res["grad_enc"] < 1e-3
