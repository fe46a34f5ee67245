"""GPU tier of kvae_lgssm_predictive_bwd / lgssm_ops.PredictiveLogLik / KalmanFilter.log_marginal / the "marginal" objective on
the gfx950 library: the cases of tests/pred_grad_cases.py (the CPU tier runs the same ones on the host simulation), under the same
bars; plus the Trainer's eager and captured step with kf_objective="marginal"."""
import pytest
import torch

import pred_grad_cases as cases
from golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from kvae import _native
    return _native.hip_lib()


_WORST = {}


@pytest.mark.parametrize("cmode,masked", [("shared", True), ("packed", True), ("shared", False), ("packed", False)])
@pytest.mark.parametrize("B,T,n", cases.SHAPES)
def test_per_item_vs_float64(lib, B, T, n, cmode, masked):
    cases.check(lib, DEV, B, T, n, cmode, masked, worst=_WORST)
    print("worst so far", {k: float(f"{v:.3g}") for k, v in _WORST.items()})


@pytest.mark.parametrize("B,T,n", [(3, 37, 4), (5, 13, 16)])
def test_unaligned_operands(lib, B, T, n):
    cases.check(lib, DEV, B, T, n, "shared", True, unaligned=True)
    cases.check(lib, DEV, B, T, n, "packed", True, pad=3)


@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_upstream_variants(lib, B, T, n):
    cases.upstream_variants(lib, DEV, B, T, n)


@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_partial_outputs_and_repeatability(lib, B, T, n):
    cases.partial_outputs(lib, DEV, B, T, n)


@pytest.mark.parametrize("cmode", cases.CMODES)
@pytest.mark.parametrize("B,T,n", [(3, 5, 4), (2, 3, 16), (3, 5, 7)])
def test_autograd_function(lib, B, T, n, cmode):
    cases.function_matches_raw(lib, DEV, B, T, n, cmode)


@pytest.mark.parametrize("n", [4, 16, 5])
def test_ladder_levels_3_and_5(lib, n):
    cases.ladder(lib, DEV, n)


@pytest.mark.parametrize("B,T,n", [(2, 5, 4), (2, 4, 16)])
def test_joint_gaussian_gradient(B, T, n):
    cases.joint_gaussian_grad(DEV, B, T, n)


def test_c_abi(lib):
    cases.c_abi(lib, DEV)


def test_unsupported_shapes_take_torch():
    cases.unsupported_takes_torch(DEV)


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_kalman_filter_log_marginal(kind, K):
    cases.model_log_marginal(DEV, kind, K)


@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_compute_loss_marginal(kind, K):
    cases.model_compute_loss(DEV, kind, K)


def test_errors():
    cases.model_errors(DEV)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,K", cases.MODELS)
def test_trainer_marginal_step_eager_vs_captured(kind, K, masked):
    """One eager step and one captured-graph step with kf_objective="marginal" from the same start, the same draws: the loss
    <= 1e-4 and the post-Adam parameters <= 1e-3 apart (the bars of tests/test_gpu_phases.py); a second step replays the graph
    (captures stays 1); the model's own kf_objective is untouched outside the step."""
    from kvae import noise
    from kvae.train.train import Trainer
    d = None
    runs = {}
    for use_graph in (False, True):
        model = cases.pc.small_model(kind, K).to(DEV)
        model.train()
        d = d or cases.pc.model_inputs(model, K)
        x = d["x"].to(DEV)
        mask = d["mask"].to(DEV) if masked else None
        nz = dict(eps_a=d["eps_a"].to(DEV), gumbel=d["gumbel"].to(DEV))
        tr = Trainer(model, lr=1e-3, use_graph=use_graph, kf_objective="marginal")
        with noise.inject(**nz):
            out = tr.step(x, mask=mask)
        torch.cuda.synchronize()
        runs[use_graph] = (out["loss"].detach().cpu().clone(), out["elbo_kf"].detach().cpu().clone(),
                           {k: p.detach().cpu().clone() for k, p in model.named_parameters()})
        assert "kf_objective" not in model.__dict__ and model.kf_objective == "elbo"
        if use_graph:
            assert tr.captures == 1
            with noise.inject(**nz):
                tr.step(x, mask=mask)
            torch.cuda.synchronize()
            assert tr.captures == 1
    (l0, e0, p0), (l1, e1, p1) = runs[False], runs[True]
    assert bool(torch.isfinite(l0)) and rel_err(l1, l0) < 1e-4 and rel_err(e1, e0) < 1e-4, (float(l0), float(l1))
    for k in p0:
        assert rel_err(p1[k], p0[k]) < 1e-3, k
