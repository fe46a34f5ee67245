"""GPU tier (-m gpu): the decoder head with the Bernoulli term folded in - k_dec_head_fwd<true> and the persistent k_dec_head_bwd of
csrc/vae_conv_edge.h on the device, through the C ABI (guarded buffers), the autograd Function, KVAE.forward / compute_loss and a
captured training step.  Cases, reference and bars: tests/dec_tail_cases.py.

Largest ratios on gfx950 (bar): ll 1.13e-07 (6.64e-07), recon 7.34e-07 (1.64e-06), dx 5.60e-07 (2.27e-06), dw 1.62e-06 (7.80e-05),
db 2.69e-07 (5.24e-05); recon has the least head-room, 2.2 x."""
import pytest
import torch

import dec_tail_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("N", D.TAIL_N)
def test_dec_tail_random_gpu(N):
    print(D.tail_random(DEV, N))


@pytest.mark.parametrize("N", D.TAIL_N)
def test_dec_tail_optional_outputs_gpu(N):
    print(D.tail_optional_outputs(DEV, N))


@pytest.mark.parametrize("N", D.TAIL_N)
def test_dec_tail_general_backward_gpu(N):
    print(D.tail_general(DEV, N))


@pytest.mark.parametrize("kind,frame,pos", [(k, f, p) for k, P in (("x", D.PROBE_X), ("h", D.PROBE_H)) for f in D.PROBE_FRAMES for p in P])
def test_dec_tail_probe_gpu(kind, frame, pos):
    print(D.tail_probe(DEV, kind, frame, pos))


def test_dec_tail_refusals_gpu():
    D.tail_refusals(DEV)


def test_compute_loss_with_another_tensor_takes_the_fallback_gpu():
    res = D.model_other_tensor(DEV)
    print(res)
    # smoke()'s bars for a whole float32 model against the oracle: 1e-4 on values, 1e-3 on gradients
    assert res["loss"] < 1e-4 and res["loss_same"] < 1e-4 and res["recon"] < 1e-4 and res["grad_head"] < 1e-3 and res["grad_enc"] < 1e-3


def test_captured_step_reproduces_the_eager_step_gpu():
    """The captured step launches the same kernels on the same inputs in the same order as the eager one, and the head has no
    atomics: loss and x_recon of each of two steps agree to float32 rounding of what the step before left (1e-5: relative for the
    loss, absolute for x_recon in [0, 1]), and after two Adam steps of lr = 1e-3 no parameter is further than 2e-4 apart - a tenth
    of what two steps move a parameter, the bar of test_lr_and_tau_schedules_reach_the_captured_graph.  Measured: 0, 6e-8, 7e-8."""
    res = D.trainer_graph_vs_eager(DEV)
    print(res)
    assert res["loss"] < 1e-5 and res["x_recon"] < 1e-5 and res["params"] < 2e-4
