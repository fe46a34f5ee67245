"""GPU tier (-m gpu) of kvae_lgssm_switching_em / lgssm_ops.switching_em_statistics / KalmanFilter.em_statistics / em_step /
kvae.train.em.fit_dynamics_em on the gfx950 library: the cases of tests/em_cases.py that tests/test_switching_em.py runs on the host
simulation, and em_statistics captured into a hipGraph."""
import pytest
import torch

import em_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", cases.CASES + [cases.LONG_CASE], ids=str)
def test_per_sequence_vs_float64(case):
    """The table is in DESIGN.md section 17."""
    cases.per_sequence(DEV, case)


def test_bits():
    cases.bits(DEV)


@pytest.mark.parametrize("name", list(cases.MSTEP_CASES))
def test_em_step_on_the_kernel(name):
    cases.mstep_on_kernel(DEV, name)


def test_skipped_regimes():
    cases.skipped_regimes(DEV)


def test_routing():
    cases.routing(DEV)
    cases.host_tensors_take_the_restatement()


def test_c_abi():
    from kvae import _native
    cases.c_abi(_native.hip_lib(), DEV)


def test_model_level():
    cases.model_level(DEV)


def test_model_without_controls():
    cases.no_controls_model(DEV)


def test_model_errors():
    cases.model_errors(DEV)


def test_statistics_capture_into_a_graph():
    """em_statistics has no host synchronisation: captured into a hipGraph, the replay gives the bits of the eager call."""
    args, mask = cases.inputs(3, 12, 3, masked=True, seed=5)
    kf = cases.make_filter(args, DEV)
    Y, U, mk = args[8].to(DEV), args[9].to(DEV), mask.to(DEV)
    eager = kf.em_statistics(Y, U, mk)   # also makes the device copy of P, which a capture may not
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kf.em_statistics(Y, U, mk)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = kf.em_statistics(Y, U, mk)
    for v in out.values():
        if v is not None:
            v.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    for k in cases.SUMS + cases.SMOOTH + ("log_lik_seq",):
        assert torch.equal(out[k], eager[k]), k
