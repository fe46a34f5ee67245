"""GPU tier of kvae_lgssm_switching_forecast / lgssm_ops.switching_forecast / KalmanFilter.forecast_regimes /
KVAE.forecast_regimes on the gfx950 library: the cases of tests/swh_cases.py (the CPU tier runs the same ones on the host
simulation), under the same bars."""
import pytest
import torch

import swh_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(case):
    cases.per_step(DEV, case)


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_horizon_one_is_the_filters_next_step(case):
    print("bit-equal:", cases.horizon_one_is_the_next_step(DEV, case))


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[1] <= 12], ids=str)
def test_every_horizon_is_a_masked_filter(case):
    print("bit-equal:", cases.every_horizon_is_a_masked_filter(DEV, case))


@pytest.mark.parametrize("K,H", [(2, 6), (3, 4)])
def test_exact_from_origin_zero(K, H):
    cases.exact_from_origin_zero(DEV, K, H)


@pytest.mark.parametrize("case", cases.CASES, ids=str)
def test_regime_forecast_is_the_chain(case):
    cases.regime_forecast_is_the_chain(DEV, case)


@pytest.mark.parametrize("what", ["identity", "shared", "single"])
def test_exact_with_fixed_regimes(what):
    cases.exact_fixed_regimes(DEV, what)


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[5] and c[1] >= 8], ids=str)
def test_streaming_is_bit_identical(case):
    cases.streaming(DEV, case)


@pytest.mark.parametrize("case", [cases.CASES[2], cases.CASES[6]], ids=str)
def test_last_origin(case):
    cases.last_origin(DEV, case)


def test_partial_outputs_and_repeatability():
    cases.partial_outputs(DEV, (3, 5, 3, 4, 2, True, 4))


def test_routing():
    cases.routing(DEV)


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_model_level():
    cases.model_level(DEV)


def test_model_errors():
    cases.model_errors(DEV)


def test_forecast_scores():
    cases.forecast_scores(DEV)


def test_model_call_captures_into_a_graph():
    """The whole of KVAE.forecast_regimes - encoder, the three launches, regimes_fore, valid, the decoded last origin - can be
    captured into a hipGraph: nothing in it synchronises or copies back (the process keeps the project's default queue count)."""
    model, x, mask, u_all, _ = cases._model_case(DEV)
    model.eval()
    mask = mask.to(DEV)
    call = lambda: model.forecast_regimes(x, cases.MODEL_H, u=u_all, mask=mask, decode=True)
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
    for k in cases.FORE + ("levels_fore", "regimes_fore", "valid", "regime_filt", "log_lik", "a_vae", "x_fore"):
        assert torch.equal(captured[k], eager[k]), k
