"""GPU tier (-m gpu) of kvae_lgssm_switching_marginal / kvae_lgssm_switching_marginal_bwd / lgssm_ops.switching_log_marginal /
KalmanFilter.regime_log_marginal / the "regime_marginal" objective on the gfx950 library: the cases of tests/swm_cases.py that
tests/test_switching_marginal.py runs on the host simulation, and the Trainer under the objective (eager against captured)."""
import pytest
import torch

import swm_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES, ids=str)
def test_gradients_vs_float64_autograd(case):
    cases.gradients(DEV, case)


def test_upstreams():
    cases.upstreams(DEV)


def test_partial_outputs_and_repeatability():
    cases.bits(DEV)


def test_hard_prior():
    cases.hard_prior(DEV)


@pytest.mark.parametrize("r11,level", [(-2e-6, 1), (-2e-5, 2)])
def test_ladder(r11, level):
    cases.ladder(DEV, r11, level)


@pytest.mark.parametrize("K", [1, 3])
def test_identical_regimes_are_the_existing_marginal(K):
    cases.vs_log_marginal(DEV, K)


def test_routing():
    cases.routing(DEV)
    cases.host_tensors_take_the_restatement()


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_model_level():
    cases.model_level(DEV)


def test_model_compute_loss():
    cases.model_compute_loss(DEV)


def test_trainer_eager_and_captured_agree():
    """One eager and one captured step under kf_objective="regime_marginal" agree on the loss (<= 1e-4) and on the post-Adam
    parameters (<= 1e-3: the bars of tests/test_gpu_phases.py); a second step replays the one capture; the regime posterior
    network takes no gradient, so its parameters keep their bits."""
    from golden_util import rel_err
    from kvae import noise
    from kvae.train.synthetic import bouncing_ball
    from kvae.train.train import Trainer
    from test_gpu_training_features import _model, _noise
    x = bouncing_ball(4, 10, 5).float().to(DEV)
    nz = _noise(4, 10, seed=4)

    def run(use_graph):
        model = _model("switching", seed=2)
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        tr = Trainer(model, lr=2e-3, use_graph=use_graph, kf_objective="regime_marginal")
        with noise.inject(**nz):
            out = tr.step(x)
            loss = out["loss"].detach().clone()
            first = tr.captures
            tr.step(x)
        torch.cuda.synchronize()
        assert type(model).kf_objective == "elbo" and "kf_objective" not in model.__dict__   # carried inside the step only
        return loss.cpu(), before, {k: p.detach().clone() for k, p in model.named_parameters()}, (first, tr.captures)

    lg, before, pg, caps = run(True)
    le, _, pe, _ = run(False)
    assert caps == (1, 1)
    assert bool(torch.isfinite(lg).all()) and rel_err(lg, le) <= 1e-4, (float(lg), float(le))
    moved = 0
    for k in pg:
        if "posterior" in k:
            assert torch.equal(pg[k], before[k]) and torch.equal(pe[k], before[k]), k
        else:
            assert rel_err(pg[k].cpu(), pe[k].cpu()) <= 1e-3, k
            moved += int(not torch.equal(pg[k], before[k]))
    assert moved >= 10 and any("posterior" in k for k in pg)
    dyn = [k for k in pg if k.endswith("dyn_params.A") or k.endswith("dyn_params.Q")]
    assert dyn and all(not torch.equal(pg[k], before[k]) for k in dyn)   # the likelihood moves the dynamics
