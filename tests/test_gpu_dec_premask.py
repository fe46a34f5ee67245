"""GPU tier (-m gpu): the decoder backward with each ReLU mask applied once, where the gradient is made - k_dec_head_bwd<., true, true>
and the PREMASKED / MASK_GX forms of the Winograd gradient kernels on the device, through the C ABI (guarded buffers), and the
fused decoder end to end with KVAE_PREMASK 1 against 0.  Every bar is bit equality; cases: tests/dec_premask_cases.py."""
import pytest

import dec_premask_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("loss", (False, True), ids=("plain", "bernoulli"))
@pytest.mark.parametrize("N", P.HEAD_N)
def test_head_masks_its_data_gradient_gpu(N, loss):
    P.head_case(DEV, N, loss)


@pytest.mark.parametrize("N", P.UP8_N)
def test_up8_takes_a_premasked_gradient_and_masks_its_own_gpu(N):
    P.up_case(DEV, N, 8, out_is_unread=True)


@pytest.mark.parametrize("N", P.UP4_N)
def test_up4_takes_a_premasked_gradient_gpu(N):
    P.up_case(DEV, N, 4, out_is_unread=True)


def test_premask_refusals_gpu():
    P.refusals(DEV)


@pytest.mark.parametrize("wino", (1, 0), ids=("winograd", "direct"))
def test_decoder_gradients_do_not_depend_on_where_the_mask_is_applied_gpu(tmp_path, wino):
    """forward_with_frames + backward at N = 3 and 1025, KVAE_PREMASK=1 against 0, one fresh process each: the gradient of a and
    of every decoder parameter is the same bits (also with the direct kernels of KVAE_WINO=0, which mask a second time)."""
    P.decoder_end_to_end(tmp_path, wino)
