"""GPU tier of kvae_lgssm_switching_smoother / lgssm_ops.switching_smoother / KalmanFilter.smooth_regimes / KVAE.smooth_regimes on
the gfx950 library: the cases of tests/sws_cases.py (the CPU tier runs the same ones on the host simulation), under the same bars."""
import pytest
import torch

import sws_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(case):
    cases.per_step(DEV, case)


def test_hard_prior_on_the_kernel():
    cases.hard_prior_on_kernel(DEV)


@pytest.mark.parametrize("K", [1, 3])
def test_identical_regimes_are_the_existing_smoother(K):
    cases.vs_existing_smoother(DEV, K)


def test_single_step_is_the_filter():
    cases.single_step(DEV)


def test_partial_outputs_and_repeatability():
    cases.partial_outputs(DEV, (3, 5, 3, 4, 2, True))


def test_carried_state():
    cases.carried_state(DEV)


def test_routing():
    cases.routing(DEV)


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_model_level_and_graph_capture():
    """The model-level case; then the whole call captured into a hipGraph - nothing in it synchronises, allocates on the host side
    or copies back - and the replay gives the bits of the eager call."""
    model, x, mask, u = cases.model_level(DEV)
    mask = mask.to(DEV)
    call = lambda: model.smooth_regimes(x, u=u, mask=mask)
    eager = call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = call()
    graph.replay()
    torch.cuda.synchronize()
    for k in cases.SMOOTH + ("regimes", "a_smooth", "regime_filt", "log_lik_seq"):
        assert torch.equal(captured[k], eager[k]), k


def test_model_errors():
    cases.model_errors(DEV)


def test_regime_smoother_scores():
    cases.smoother_scores(DEV)
