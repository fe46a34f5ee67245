"""GPU tier of kvae_lgssm_switching_filter / lgssm_ops.switching_filter / KalmanFilter.filter_regimes / KVAE.filter_regimes on the
gfx950 library: the cases of tests/swf_cases.py (the CPU tier runs the same ones on the host simulation), under the same bars."""
import pytest
import torch

import swf_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(case):
    cases.per_step(DEV, case)


def test_identity_prior_on_the_kernel():
    cases.identity_prior_on_kernel(DEV)


@pytest.mark.parametrize("K", [1, 3])
def test_identical_regimes_are_the_existing_filter(K):
    cases.vs_existing_filter(DEV, K)


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[5] and c[1] >= 8], ids=str)
def test_streaming_is_bit_identical(case):
    cases.streaming(DEV, case)


def test_partial_outputs_and_repeatability():
    cases.partial_outputs(DEV, (3, 5, 3, 4, 2, True))


def test_routing():
    cases.routing(DEV)


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_no_host_synchronisation():
    """The whole call can be captured into a hipGraph: nothing in it synchronises, allocates on the host side or copies back."""
    args, mask, _ = cases.reference((3, 12, 7, 4, 2, True))
    args, mask = tuple(a.to(DEV) for a in args), mask.to(DEV)
    eager = cases.run(DEV, args, mask)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cases.run(DEV, args, mask)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = cases.run(DEV, args, mask)
    graph.replay()
    torch.cuda.synchronize()
    for k in cases.OUTPUTS + ("levels",):
        assert torch.equal(captured[k], eager[k]), k
    for k in cases.STATE:
        assert torch.equal(captured["state"][k], eager["state"][k]), k


def test_model_level():
    cases.model_level(DEV)


def test_model_errors():
    cases.model_errors(DEV)


def test_regime_filter_scores():
    cases.filter_scores(DEV)
