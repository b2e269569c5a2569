"""The native convolution (kpn_conv2d_forward / kpn_conv2d_backward) on the host SIMT emulator: the very kernel sources, with
numpy buffers through the C ABI.  Cases, reference and bar: tests/conv_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_cases as cc
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = cc.HostArrays()


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_forward_and_gradients_against_fp64(L, name):
    cc.check_case(L, B, name)


def test_packed_copies_hold_the_weight_in_both_orders(L):
    """[chunk][cout_p][16] with k = tap * cin + ci; the second copy is w'[ci][co][k - 1 - ky][k - 1 - kx]"""
    c = cc.CASES["k5_12to36"]
    w = cc.reference("k5_12to36")[0][1].numpy()
    packed = cc.pack(L, B, c, w)
    cin, cout, k = c["cin"], c["cout"], c["k"]
    nk_f, coutp_f = -(-k * k * cin // 16), 64                      # 36 output channels: the 64-wide tile
    fwd = packed[:nk_f * coutp_f * 16].reshape(nk_f, coutp_f, 16).transpose(0, 2, 1).reshape(nk_f * 16, coutp_f)
    assert np.array_equal(fwd[:k * k * cin, :cout], w.transpose(2, 3, 1, 0).reshape(k * k * cin, cout))
    assert not fwd[k * k * cin:].any() and not fwd[:, cout:].any()
    nk_b, coutp_b = -(-k * k * cout // 16), 32                     # 12 "output" channels: the 32-wide tile
    bwd = packed[nk_f * coutp_f * 16:].reshape(nk_b, coutp_b, 16).transpose(0, 2, 1).reshape(nk_b * 16, coutp_b)
    assert packed.size == (nk_f * coutp_f + nk_b * coutp_b) * 16
    assert np.array_equal(bwd[:k * k * cout, :cin], w[:, :, ::-1, ::-1].transpose(2, 3, 0, 1).reshape(k * k * cout, cin))
    assert not bwd[k * k * cout:].any() and not bwd[:, cin:].any()


def test_two_calls_give_equal_bits(L):
    cc.check_two_calls_equal_bits(L, B, "k5_12to36")


def test_null_legs_leave_their_buffers_untouched(L):
    cc.check_null_legs_leave_buffers_alone(L, B, "k3_4to8")


def test_zero_dy_gives_exact_zeros(L):
    cc.check_zero_dy_gives_zeros(L, B, "k3_p0")


def test_bad_descriptors_are_refused_with_a_message(L):
    cc.check_bad_descriptors(L, B)


def test_wgrad_range_counts_follow_the_stated_rule(L):
    cc.check_range_counts(L)


def test_workspace_covers_every_partial_buffer(L):
    """the workspace query is at least the split-K scratch of both k_enc_conv launches, the wgrad ranges and the fp64 bias chunks"""
    c = cc.CASES["ranges3"]
    nb = L.kpn_conv2d_workspace_bytes(ctypes.byref(cc.desc(c)))
    n, _, _ = cc.expected_ranges(c)
    assert nb >= n * c["k"] * c["k"] * c["cin"] * c["cout"] * 4 + 3 * c["cout"] * 8


def test_fake_kernel_gives_the_output_shape_in_channels_last():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w = torch.empty(2, 12, 9, 11, device="cuda"), torch.empty(36, 12, 5, 5, device="cuda")
        y = torch.ops.kpnerf.conv2d(x, w, None, 1)
        assert tuple(y.shape) == (2, 36, 7, 9) and y.is_contiguous(memory_format=torch.channels_last)
        dx, dw, db = torch.ops.kpnerf.conv2d_backward(x, w, y, 1, True, [True, True, False])
        assert dx.shape == x.shape and dw.shape == w.shape and db.numel() == 0
    with pytest.raises((NotImplementedError, RuntimeError)):             # no CPU kernel
        torch.ops.kpnerf.conv2d(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3), None, 1)


def test_install_native_convs_rebinds_only_eligible_layers_and_restores_them():
    from keypointnerf_amd import encoders
    net, twin = cc.stand_in_stack(), cc.stand_in_stack()
    net.add_module("odd", torch.nn.Conv2d(8, 6, 3, padding=1))
    net.add_module("rep", torch.nn.Conv2d(8, 8, 3, padding=1, padding_mode="replicate"))
    net.add_module("stem", torch.nn.Conv2d(4, 8, 7, padding=3))
    net.add_module("up", torch.nn.ConvTranspose2d(8, 8, 3, stride=2, padding=1, output_padding=1))
    keys, bound = list(net.state_dict().keys()), [m.forward.__func__ for m in net]
    served, left = encoders.install_native_convs(net)
    assert served == ["0", "3"]
    assert sorted(left) == ["4", "odd", "rep", "stem"]                   # a ConvTranspose2d is no nn.Conv2d: not even listed
    assert "stride=2" in left["4"] and "channels" in left["odd"] and "padding_mode" in left["rep"] and "kernel_size" in left["stem"]
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == keys
    assert all(("forward" in m.__dict__) == (n in served) for n, m in net.named_children())
    # CPU tensors are none of the native path's business: the rebound forward hands them to the module's own forward
    x = torch.randn(1, 8, 6, 6, generator=torch.Generator().manual_seed(1))
    assert torch.equal(net[:5](x), twin(x))
    assert encoders.install_native_convs(net)[0] == served               # installing twice does not stack
    encoders.uninstall_native_convs(net)
    assert all("forward" not in m.__dict__ and "_kpnerf_conv_saved" not in m.__dict__ for m in net)
    assert [m.forward.__func__ for m in net] == bound
