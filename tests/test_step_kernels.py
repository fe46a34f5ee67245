"""CPU tier of tests/step_cases.py on the PLAIN-LOOP TWINS of tests/hostsim/hostsim.cpp (kvae_clip_adam, kvae_loss_head_fwd/bwd,
kvae_colsum, kvae_colsum2, kvae_lgssm_emission_means, kvae_bias_shuffle_act_fwd/bwd with the emulation off) and, through them, the
Python wrappers (LossHead.apply, _native.colsum / colsum_pair, lgssm_ops.emission_means).  The twins are separate
re-implementations: this tier checks the CASES, the float64 REFERENCES, the YARDSTICKS the bars derive from and the wrappers' own
logic, quickly and at the GPU tier's sizes.  The kernels themselves - csrc/clip_adam.h, vae_heads.h, colsum.h, emission_means.h,
vae_epilogue.h - run the same case functions on emulated workgroups in tests/test_wave_emu_step.py, and on the card in
tests/test_gpu_step_kernels.py (DESIGN sections 2, 5 and 8)."""
import pytest
import torch

import step_cases as cases
from hostsim.build import build as build_hostsim

torch.set_num_threads(4)
DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def hostsim_backend():
    from kvae import _native
    lib = _native.LgssmLib(build_hostsim())
    _native._set_test_backend(lib)
    yield lib
    _native._set_test_backend(None)


def test_yardsticks_are_what_float32_torch_gives():
    """The constants the bars derive from: the float32 restatements against the float64 references, remeasured.  Each is the largest
    of a few thousand rounding samples and moves with the host's vector width and libm: within a factor 3 either way."""
    got = cases.yardsticks()
    print({k: float(f"{v:.3g}") for k, v in got.items()})
    assert set(got) == set(cases.YARDSTICK)
    for k, v in got.items():
        assert v / 3 <= cases.YARDSTICK[k] <= v * 3, (k, v, cases.YARDSTICK[k])


def test_restatement_is_torch_adam_in_float64():
    """clip_grad_norm_ + torch.optim.Adam on float64 parameters against adam_restated in float64: 8.1e-16 measured (the bias
    corrections are Python floats in torch, tensors here); the bar is 100 times that."""
    assert cases.adam_anchor() < 8.1e-14


def test_float32_torch_adam_differs_by_the_beta2_constant():
    """Why the yardstick is a restatement and not torch.optim.Adam in float32: its exp_avg_sq sits 1.30e-5 from a float64 Adam
    with the float32-rounded beta2 (float32(0.001) against 1 - float32(0.999)), fifty times the restatement's own rounding."""
    gap = cases.beta2_constant_gap()
    assert 1.2e-5 < gap < 1.4e-5 and gap > 10 * cases.TOL["adam.v"]


@pytest.mark.parametrize("case", cases.ADAM_IDS)
def test_clip_adam_per_element(hostsim_backend, case):
    cases.adam_case(hostsim_backend, DEV, cases.adam_case_by_id(case))


def test_clip_adam_rejects(hostsim_backend):
    cases.adam_rejects(hostsim_backend, DEV)


@pytest.mark.parametrize("case", ["stride-524545", "layout-block-edges"])
def test_clip_adam_repeatable(hostsim_backend, case):
    cases.adam_repeatable(hostsim_backend, DEV, case)


def test_clip_adam_nan_gradient(hostsim_backend):
    cases.adam_nan_gradient(hostsim_backend, DEV)


@pytest.mark.parametrize("case", cases.HEAD_IDS)
def test_loss_head_c_abi(hostsim_backend, case):
    cases.head_case(hostsim_backend, DEV, cases.HEAD_CASES[cases.HEAD_IDS.index(case)])


def test_loss_head_bwd_grid_stride(hostsim_backend):
    cases.head_bwd_large(hostsim_backend, DEV)


@pytest.mark.parametrize("transposed,beta_tensor,masked", cases.HEAD_APPLY_CASES)
def test_loss_head_apply(transposed, beta_tensor, masked):
    cases.head_apply(DEV, transposed, beta_tensor, masked)
    cases.head_apply(DEV, transposed, beta_tensor, masked, weights_dev=True)


@pytest.mark.parametrize("cols", cases.COLSUM_COLS)
def test_colsum_c_abi(hostsim_backend, cols):
    cases.colsum_abi(hostsim_backend, DEV, cols)


def test_colsum2_c_abi(hostsim_backend):
    cases.colsum2_abi(hostsim_backend, DEV)


@pytest.mark.parametrize("rows,cols", cases.NATIVE_COLSUM_SHAPES)
def test_native_colsum(rows, cols):
    cases.native_colsum(DEV, rows, cols)


@pytest.mark.parametrize("ra,ca,rb,cb", cases.NATIVE_PAIR_SHAPES)
def test_native_colsum_pair(ra, ca, rb, cb):
    cases.native_colsum_pair(DEV, ra, ca, rb, cb)


@pytest.mark.parametrize("layout", cases.EMISSION_LAYOUTS)
@pytest.mark.parametrize("B,T,n,p", cases.EMISSION_SHAPES)
def test_emission_means(B, T, n, p, layout):
    cases.emission_ops(DEV, B, T, n, p, layout)


@pytest.mark.parametrize("B,T,n,p", cases.EMISSION_SHAPES)
def test_emission_means_c_abi(hostsim_backend, B, T, n, p):
    cases.emission_abi(hostsim_backend, DEV, B, T, n, p)


def test_emission_means_rejects(hostsim_backend):
    cases.emission_rejects(hostsim_backend, DEV)


@pytest.mark.parametrize("shape,off_in,off_out,kernel", cases.EPI_FWD_CASES, ids=cases.case_id)
def test_epilogue_fwd_per_element(hostsim_backend, shape, off_in, off_out, kernel):
    cases.epi_fwd_case(hostsim_backend, DEV, shape, off_in, off_out)


@pytest.mark.parametrize("shape,relu,want_bias,off", cases.EPI_BWD_CASES, ids=cases.case_id)
def test_epilogue_bwd_per_element(hostsim_backend, shape, relu, want_bias, off):
    cases.epi_bwd_case(hostsim_backend, DEV, shape, relu, want_bias, off)


def test_epilogue_rejects(hostsim_backend):
    cases.epi_rejects(hostsim_backend, DEV)
