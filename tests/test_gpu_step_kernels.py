"""GPU tier of tests/step_cases.py: kvae_clip_adam (k_grad_sumsq + k_clip_adam), kvae_loss_head_fwd/bwd, kvae_colsum / kvae_colsum2
with the folding of _native.colsum / colsum_pair, kvae_lgssm_emission_means and kvae_bias_shuffle_act_fwd/bwd on the gfx950 library,
per element against float64 under bars of 4 x the float32 yardstick (the conv epilogue's permutation and select: bit for bit
against float32 torch).  The CPU tiers run the same cases on the product's kernels on emulated workgroups
(tests/test_wave_emu_step.py) and on the plain-loop twins (tests/test_step_kernels.py)."""
import pytest

import step_cases as cases
from kvae import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"
_WORST = {}


@pytest.fixture(scope="module")
def lib():
    return _native.hip_lib()


@pytest.mark.parametrize("case", cases.ADAM_IDS)
def test_clip_adam_per_element(lib, case):
    cases.adam_case(lib, DEV, cases.adam_case_by_id(case), worst=_WORST)


def test_clip_adam_rejects(lib):
    cases.adam_rejects(lib, DEV)


@pytest.mark.parametrize("case", ["stride-524545", "layout-block-edges"])
def test_clip_adam_repeatable(lib, case):
    cases.adam_repeatable(lib, DEV, case)


def test_clip_adam_nan_gradient(lib):
    """fminf(clip / (NaN + 1e-6), 1) is 1: the other active elements take an UNCLIPPED step (torch's clamp would hand the NaN to
    every gradient); only the element with the NaN turns NaN.  Asserted: the norm is not finite, the frozen segment is untouched."""
    print("finite parameters after a NaN gradient:", cases.adam_nan_gradient(lib, DEV), "of 348")


@pytest.mark.parametrize("case", cases.HEAD_IDS)
def test_loss_head_c_abi(lib, case):
    cases.head_case(lib, DEV, cases.HEAD_CASES[cases.HEAD_IDS.index(case)], worst=_WORST)


def test_loss_head_bwd_grid_stride(lib):
    cases.head_bwd_large(lib, DEV, worst=_WORST)


@pytest.mark.parametrize("transposed,beta_tensor,masked", cases.HEAD_APPLY_CASES)
def test_loss_head_apply(transposed, beta_tensor, masked):
    cases.head_apply(DEV, transposed, beta_tensor, masked, worst=_WORST)
    cases.head_apply(DEV, transposed, beta_tensor, masked, weights_dev=True, worst=_WORST)


@pytest.mark.parametrize("cols", cases.COLSUM_COLS)
def test_colsum_c_abi(lib, cols):
    cases.colsum_abi(lib, DEV, cols, worst=_WORST)


def test_colsum2_c_abi(lib):
    cases.colsum2_abi(lib, DEV, worst=_WORST)


@pytest.mark.parametrize("rows,cols", cases.NATIVE_COLSUM_SHAPES)
def test_native_colsum(rows, cols):
    cases.native_colsum(DEV, rows, cols, worst=_WORST)


@pytest.mark.parametrize("ra,ca,rb,cb", cases.NATIVE_PAIR_SHAPES)
def test_native_colsum_pair(ra, ca, rb, cb):
    cases.native_colsum_pair(DEV, ra, ca, rb, cb, worst=_WORST)


@pytest.mark.parametrize("layout", cases.EMISSION_LAYOUTS)
@pytest.mark.parametrize("B,T,n,p", cases.EMISSION_SHAPES)
def test_emission_means(B, T, n, p, layout):
    cases.emission_ops(DEV, B, T, n, p, layout, worst=_WORST)


@pytest.mark.parametrize("B,T,n,p", cases.EMISSION_SHAPES)
def test_emission_means_c_abi(lib, B, T, n, p):
    cases.emission_abi(lib, DEV, B, T, n, p, worst=_WORST)


def test_emission_means_rejects(lib):
    cases.emission_rejects(lib, DEV)


@pytest.mark.parametrize("shape,off_in,off_out,kernel", cases.EPI_FWD_CASES, ids=cases.case_id)
def test_epilogue_fwd_per_element(lib, shape, off_in, off_out, kernel):
    cases.epi_fwd_case(lib, DEV, shape, off_in, off_out)


@pytest.mark.parametrize("shape,kernel", cases.EPI_STRIDE_CARD, ids=cases.case_id)
def test_epilogue_fwd_grid_stride(lib, shape, kernel):
    """total / 4 (float4 kernel) and total (scalar kernel) just above epi_grid's 8192 x 256: a second, ragged grid-stride round."""
    cases.epi_fwd_case(lib, DEV, shape)


@pytest.mark.parametrize("shape,relu,want_bias,off", cases.EPI_BWD_CASES, ids=cases.case_id)
def test_epilogue_bwd_per_element(lib, shape, relu, want_bias, off):
    cases.epi_bwd_case(lib, DEV, shape, relu, want_bias, off, worst=_WORST)


def test_epilogue_bwd_grid_stride(lib):
    cases.epi_bwd_case(lib, DEV, cases.EPI_BWD_STRIDE_CARD, 1, False)


def test_epilogue_rejects(lib):
    cases.epi_rejects(lib, DEV)


def test_report_largest_ratios():
    """Prints (pytest -s) the largest ratio each quantity reached in this run beside its bar: the table of DESIGN section 2."""
    for k in sorted(_WORST):
        print(f"{k:12s} {_WORST[k]:.3g}  bar {cases.TOL[k]:.3g}  head-room {cases.TOL[k] / max(_WORST[k], 1e-300):.2f} x")
