"""GPU tier of kvae_regime_decode / lgssm_ops.regime_decode / KVAE.decode_regimes on the gfx950 library: the cases of
tests/regime_decode_cases.py (the CPU tier runs the same ones on the host simulation), under the same bars."""
import pytest
import torch

import regime_decode_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("B,T,K", cases.SHAPES + cases.LONG_SHAPES)
def test_per_step_vs_float64(B, T, K):
    cases.per_step(DEV, B, T, K)


@pytest.mark.parametrize("K,T", [(3, 5), (2, 8)])
def test_brute_force(K, T):
    cases.brute_force(DEV, K, T)


@pytest.mark.parametrize("T,K,seed", [(12, 3, 1), (9, 7, 2)])
def test_vs_sampled_chain(T, K, seed):
    cases.vs_sampled_chain(DEV, T, K, seed)


@pytest.mark.parametrize("K", [4, 7, 16])
def test_ties_take_the_lowest_index(K):
    cases.ties(DEV, K)


@pytest.mark.parametrize("B,T,K", [(2, 9, 5), (2, 6, 10)])
def test_prior_clamp(B, T, K):
    cases.clamp(DEV, B, T, K)


@pytest.mark.parametrize("B,T,K", [(3, 7, 6), (2, 5, 11)])
def test_partial_outputs(B, T, K):
    cases.partial_outputs(DEV, B, T, K)


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_k17_takes_torch():
    cases.k17_takes_torch(DEV)


def test_no_host_synchronisation():
    """The whole call can be captured into a hipGraph: nothing in it synchronises, allocates on the host side or copies back."""
    from kvae.kalman import lgssm_ops
    logits, init, P = (t.to(DEV) for t in cases.inputs(3, 9, 7))
    eager = lgssm_ops.regime_decode(logits, init, P)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lgssm_ops.regime_decode(logits, init, P)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = lgssm_ops.regime_decode(logits, init, P)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("marginals", "path", "path_logq", "kl"):
        assert torch.equal(captured[k], eager[k]), k


@pytest.mark.parametrize("K", [3, 7])
def test_model_level(K):
    cases.model_level(DEV, K)


def test_forward_unchanged_by_pinned():
    cases.forward_unchanged_by_pinned(DEV)


def test_model_errors():
    cases.model_errors(DEV)
