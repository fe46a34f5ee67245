"""GPU tier of kvae_lgssm_predictive / KalmanFilter.predictive / KVAE.score / KVAE.log_likelihood on the gfx950 library: the
cases of tests/pred_cases.py (the CPU tier runs the same ones on the host simulation), under the same bars."""
import pytest
import torch

import pred_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("cmode,masked", [("shared", True), ("packed", True), ("shared", False)])
@pytest.mark.parametrize("B,T,n", cases.SHAPES + cases.SEQ_SHAPES)
def test_per_item_vs_float64(B, T, n, cmode, masked):
    cases.check(DEV, B, T, n, cmode, masked)


@pytest.mark.parametrize("B,T,n", [(3, 37, 4), (5, 13, 16)])
def test_unaligned_operands(B, T, n):
    cases.check(DEV, B, T, n, "shared", True, unaligned=True)
    cases.check(DEV, B, T, n, "packed", True, pad=3)


@pytest.mark.parametrize("B,T,n", [(2, 5, 4), (2, 4, 16)])
def test_joint_gaussian(B, T, n):
    cases.joint_gaussian(DEV, B, T, n)


@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_partial_outputs_and_repeatability(B, T, n):
    cases.partial_outputs(DEV, B, T, n)


@pytest.mark.parametrize("n", [4, 16, 5])
def test_ladder_level_per_item(n):
    cases.ladder(DEV, n)
    cases.ladder(DEV, n, impl="torch")


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_unsupported_shapes_take_torch():
    cases.unsupported_takes_torch(DEV)


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_score(kind, K):
    cases.model_score(DEV, kind, K)


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_log_likelihood(kind, K):
    cases.model_log_likelihood(DEV, kind, K)


def test_prediction_scores():
    cases.model_prediction_scores(DEV)
    cases.model_prediction_scores(DEV, "switching", 3)


def test_model_errors():
    cases.model_errors(DEV)


def test_calibration():
    cases.calibration(DEV)


@pytest.mark.parametrize("kind,K,masked", [("lstm", 3, True), ("lstm", 3, False), ("switching", 3, True)])
def test_score_captures_into_a_graph(kind, K, masked):
    """The whole of KVAE.score can be captured into a hipGraph: nothing in it synchronises or copies back."""
    model = cases.small_model(kind, K).to(DEV).eval()
    d = cases.model_inputs(model, K)
    x, u = d["x"].to(DEV), d["u"].to(DEV)
    mask = d["mask"].to(DEV) if masked else None
    eager = model.score(x, u=u, mask=mask)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.score(x, u=u, mask=mask)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = model.score(x, u=u, mask=mask)
    graph.replay()
    torch.cuda.synchronize()
    for k in cases.SCORE_KEYS + ("levels", "a_vae"):
        assert torch.equal(captured[k], eager[k]), k
