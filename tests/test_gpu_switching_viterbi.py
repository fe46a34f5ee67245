"""GPU tier of kvae_lgssm_switching_viterbi / lgssm_ops.switching_viterbi / KalmanFilter.viterbi_regimes / KVAE.viterbi_regimes
on the gfx950 library: the cases of tests/swv_cases.py (the CPU tier runs the same ones on the host simulation), under the same
bars."""
import pytest
import torch

import swv_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(case):
    cases.per_step(DEV, case)


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_score_and_beliefs_vs_the_pinned_filter(case):
    cases.score_is_exact_on_kernel(DEV, case)


@pytest.mark.parametrize("K,T", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_true_map_when_short(K, T):
    cases.true_map_when_short(DEV, K, T)


@pytest.mark.parametrize("K,T", [(2, 6), (3, 5)])
def test_bounded_by_the_enumerated_map(K, T):
    cases.bounded_by_the_map(DEV, K, T)


def test_identity_prior():
    cases.identity_prior(DEV)


def test_shared_dynamics_take_regime_zero():
    cases.shared_dynamics(DEV)


def test_single_regime_is_the_existing_filter():
    cases.single_regime(DEV)


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


def test_model_level():
    cases.model_level(DEV)


def test_model_errors():
    cases.model_errors(DEV)


def test_viterbi_scores():
    cases.viterbi_scores(DEV)


def test_model_call_captures_into_a_graph():
    """The whole of KVAE.viterbi_regimes - encoder, the one launch, the pinned smoother, the decoded frames - can be captured into
    a hipGraph once: nothing in it synchronises or copies back (the process keeps the project's default queue count)."""
    model, x, mask, u, _ = cases.swf_cases._model_case(DEV)
    model.eval()
    mask = mask.to(DEV)
    call = lambda: model.viterbi_regimes(x, u=u, mask=mask, decode=True)
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
    for k in cases.FLOATS + ("path", "backptr", "levels", "regimes", "a_vae", "mus_smooth", "x_imputed"):
        assert torch.equal(captured[k], eager[k]), k
