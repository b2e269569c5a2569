"""kpn_mse_psnr, kpn_pix_l1_loss and kpn_train_loss on the device against the NumPy restatement of the shared reduction's
summation order (tests/reduce_order_cases.py): exact bits, the cases of tests/test_reduce_order_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import reduce_order_cases as rc
from tests import train_loss_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from keypointnerf_amd import lib as kl

    def to_host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return tc.Driver(kl.get_library(), to_dev=lambda a: torch.from_numpy(np.array(a)).cuda(), ptr=lambda t: ctypes.c_void_p(t.data_ptr()),
                     to_host=to_host, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("n", rc.COUNTS)
def test_mse_is_the_order_model_bit_for_bit(drv, n):
    rc.check_mse(drv, n)


@pytest.mark.parametrize("n", rc.COUNTS)
def test_pix_l1_is_the_order_model_bit_for_bit(drv, n):
    rc.check_pix_l1(drv, n)


@pytest.mark.parametrize("n", rc.TRAIN_N)
def test_train_loss_is_the_order_model_bit_for_bit(drv, n):
    rc.check_train_loss(drv, n)
