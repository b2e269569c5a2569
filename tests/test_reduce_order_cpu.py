"""kpn_mse_psnr, kpn_pix_l1_loss and kpn_train_loss on the wave64 emulator build against the NumPy restatement of the shared
reduction's summation order (tests/reduce_order_cases.py): exact bits.  tests/test_gpu_reduce_order.py repeats them on the device."""
import numpy as np
import pytest

from tests import reduce_order_cases as rc
from tests import simt_harness as sh
from tests import train_loss_cases as tc


@pytest.fixture(scope="module")
def drv():
    return tc.Driver(sh.simt_lib(), to_dev=lambda a: np.array(a), ptr=sh.ptr, to_host=lambda a: a)


def test_order_model_on_a_hand_computed_case():
    """the model itself: 257 elements are two blocks; block 0's tree pairs t with t + 128, then + 64, ...; 0.0 + partials in order"""
    e = np.arange(1.0, 258.0) * (1.0 + 2.0 ** -30)
    red = e[:256].copy()
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        red[:s] = red[:s] + red[s:2 * s]
    assert rc.bits(rc.ordered_sum(e, 2)) == rc.bits((np.float64(0.0) + red[0]) + e[256])
    assert rc.blocks_for(1) == 1 and rc.blocks_for(257) == 2 and rc.blocks_for(524288) == 2048 and rc.blocks_for(524289) == 2048
    # what the checks can see: another grid and another element order give other bits for the L1 sum of wide inputs and for
    # the sums of squares of uniform and of grid inputs
    for kind, elem in (("wide", np.abs), ("uniform", np.square), ("grid", np.square)):
        a, b = rc.pair(1048653, 2, kind)
        e = elem((a - b).astype(np.float64))
        model = rc.bits(rc.ordered_sum(e, 2048))
        assert model != rc.bits(rc.ordered_sum(e, 2047)) and model != rc.bits(rc.ordered_sum(np.roll(e, 1), 2048)), kind


@pytest.mark.parametrize("n", rc.COUNTS)
def test_mse_is_the_order_model_bit_for_bit(drv, n):
    rc.check_mse(drv, n)


@pytest.mark.parametrize("n", rc.COUNTS)
def test_pix_l1_is_the_order_model_bit_for_bit(drv, n):
    rc.check_pix_l1(drv, n)


@pytest.mark.parametrize("n", rc.TRAIN_N)
def test_train_loss_is_the_order_model_bit_for_bit(drv, n):
    rc.check_train_loss(drv, n)
