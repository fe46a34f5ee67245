"""GPU tier of kvae_lgssm_switching_pf / lgssm_ops.switching_pf / KalmanFilter.particle_filter_regimes /
KVAE.particle_filter_regimes on the gfx950 library: the cases of tests/spf_cases.py (the CPU tier runs the same ones on the host
simulation), under the same bars; the unbiasedness check with the 512 replicates it is specified with."""
import pytest
import torch

import spf_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_step_vs_float64(case):
    cases.per_step(DEV, case)


def test_every_ladder_level_on_the_kernel():
    cases.ladder_levels(DEV)


def test_identity_prior_on_the_kernel():
    cases.identity_prior(DEV)


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("K", [1, 3])
def test_identical_regimes_are_the_existing_filter(K, thr):
    cases.vs_existing_filter(DEV, K, thr)


@pytest.mark.parametrize("thr", [0.5, 1.0])
@pytest.mark.parametrize("K,T", [(2, 10), (3, 8)])
def test_unbiased_on_the_kernel(K, T, thr):
    cases.unbiased(DEV, K, T, thr, G=512, impl="hip")


def test_lineages():
    cases.lineage_rules(DEV)


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[6] and c[2] >= 8], ids=str)
def test_streaming_is_bit_identical(case):
    cases.streaming(DEV, case)


def test_partial_outputs_and_repeatability():
    cases.partial_outputs(DEV, (3, 3, 5, 3, 4, 2, False, 64, 0.5))


def test_routing():
    cases.routing(DEV)


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_no_host_synchronisation():
    """The whole call can be captured into a hipGraph: nothing in it synchronises, allocates on the host side or copies back
    (the process keeps the project's default queue count)."""
    case = (2, 4, 12, 7, 4, 2, True, 64, 1.0)
    args, mask, th, ph, _ = cases.reference(case)
    args, mask, th, ph = tuple(a.to(DEV) for a in args), mask.to(DEV), th.to(DEV), ph.to(DEV)
    eager = cases.run(DEV, args, th, ph, mask, case[-1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cases.run(DEV, args, th, ph, mask, case[-1])   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = cases.run(DEV, args, th, ph, mask, case[-1])
    graph.replay()
    torch.cuda.synchronize()
    for k in cases.PER_STEP + ("log_lik_seq", "paths", "path_log_w"):
        assert torch.equal(captured[k], eager[k]), k
    for k in cases.STATE + ("regime",):
        assert torch.equal(captured["state"][k], eager["state"][k]), k


def test_model_call_captures_into_a_graph():
    """The whole of KVAE.particle_filter_regimes - encoder, the draws, the three launches, the combination over the replicates -
    can be captured into a hipGraph: nothing in it synchronises or copies back."""
    from kvae import noise
    model, x, mask, u, _ = cases._model_case(DEV)
    model.eval()
    mask = mask.to(DEV)
    th, ph = cases._model_draws(x.shape[0], x.shape[1], DEV)
    keys = cases.PER_STEP + ("log_lik_seq", "paths", "log_lik_seq_mean", "regime_filt_mean", "regimes_map", "a_filt", "a_vae")
    with noise.inject(pf_regime=th, pf_resample=ph):
        eager = model.particle_filter_regimes(x, u=u, mask=mask, **cases.MODEL_PF)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.particle_filter_regimes(x, u=u, mask=mask, **cases.MODEL_PF)   # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            captured = model.particle_filter_regimes(x, u=u, mask=mask, **cases.MODEL_PF)
    graph.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(captured[k], eager[k]), k


def test_model_level():
    cases.model_level(DEV)


def test_model_errors():
    cases.model_errors(DEV)


def test_particle_filter_scores():
    cases.pf_scores(DEV)
