"""The native stride-2, stem and transposed convolutions (kpn_conv2d_s2_forward / kpn_conv2d_s2_backward) on the host SIMT emulator:
the very kernel sources, with numpy buffers through the C ABI.  Cases, reference and bar: tests/strided_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import simt_harness as sh
from tests import strided_cases as sc


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = sc.HostArrays()


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_forward_and_gradients_against_fp64(L, name):
    sc.check_case(L, B, name)


@pytest.mark.parametrize("name", sc.ONE_PER_KIND)
def test_two_calls_give_equal_bits(L, name):
    sc.check_two_calls_equal_bits(L, B, name)


@pytest.mark.parametrize("name", ("s2_4to8", "stem_3to64", "up_8to4"))
def test_null_legs_leave_their_buffers_untouched(L, name):
    sc.check_null_legs_leave_buffers_alone(L, B, name)


@pytest.mark.parametrize("name", sc.ONE_PER_KIND)
def test_zero_dy_gives_exact_zeros(L, name):
    sc.check_zero_dy_gives_zeros(L, B, name)


def test_wgrad_range_counts_follow_the_stated_rule(L):
    sc.check_range_counts(L)


def test_the_padded_stem_channel_is_never_read(L):
    sc.check_padded_stem_channel(L, B)


def test_bad_calls_are_refused_with_a_message_and_launch_nothing(L):
    sc.check_refusals(L, B)


def test_the_stem_packs_four_channel_taps_and_zeros_the_padded_one(L):
    """[chunk][cout_p][16] with k = tap * 4 + ci: the fourth channel of every tap, and everything behind tap 48, is zero"""
    c = sc.CASES["stem_3to64"]
    w = sc.reference("stem_3to64")[0][1].numpy()
    packed = sc.pack(L, B, c, w)
    nk = -(-49 * 4 // 16)
    assert packed.size == nk * 64 * 16                                   # no input-gradient copy
    rows = packed.reshape(nk, 64, 16).transpose(0, 2, 1).reshape(nk * 16, 64)[:196].reshape(49, 4, 64)
    assert np.array_equal(rows[:, :3], w.transpose(2, 3, 1, 0).reshape(49, 3, 64)) and not rows[:, 3].any()
    assert not packed.reshape(nk, 64, 16).transpose(0, 2, 1).reshape(nk * 16, 64)[196:].any()


def test_workspace_covers_the_range_partials(L):
    for name in ("s2_ranges", "stem_ranges", "up_ranges"):
        c = sc.CASES[name]
        n = sc.expected_ranges(c)[0]
        assert L.kpn_conv2d_s2_workspace_bytes(ctypes.byref(sc.desc(c))) >= n * int(np.prod(sc.w_shape(c))) * 4


def test_fake_kernels_give_channels_last_shapes():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 12, 8, 10, device="cuda").contiguous(memory_format=torch.channels_last)
        w = torch.empty(36, 12, 3, 3, device="cuda")
        y = torch.ops.kpnerf.conv2d_down2(x, w, None)
        assert tuple(y.shape) == (2, 36, 4, 5) and y.is_contiguous(memory_format=torch.channels_last)
        dx, dw, db = torch.ops.kpnerf.conv2d_s2_backward(x, w, y, 0, False, [True, True, False])
        assert dx.shape == x.shape and dw.shape == w.shape and db.numel() == 0
        im, ws = torch.empty(1, 3, 9, 7, device="cuda"), torch.empty(8, 3, 7, 7, device="cuda")
        ys = torch.ops.kpnerf.conv2d_down2(im, ws, None)
        assert tuple(ys.shape) == (1, 8, 5, 4) and ys.is_contiguous(memory_format=torch.channels_last)
        wt = torch.empty(12, 4, 3, 3, device="cuda")
        yt = torch.ops.kpnerf.conv_transpose2d_up2(x, wt, None)
        assert tuple(yt.shape) == (2, 4, 16, 20) and yt.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises((NotImplementedError, RuntimeError)):             # no CPU kernel
        torch.ops.kpnerf.conv2d_down2(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3), None)


def _stack():
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(3, 8, 7, stride=2, padding=3), nn.Conv2d(8, 16, 3, stride=2, padding=1),
                         nn.ConvTranspose2d(16, 8, 3, stride=2, padding=1, output_padding=1), nn.Conv2d(8, 8, 3, stride=2, padding=0))


def test_install_native_strided_rebinds_only_eligible_layers_and_restores_them():
    from keypointnerf_amd import encoders
    net, twin = _stack(), _stack()
    twin.load_state_dict(net.state_dict())
    net.add_module("s1", torch.nn.Conv2d(8, 8, 3, padding=1))                                    # install_native_convs' layer: not listed
    net.add_module("rep", torch.nn.Conv2d(8, 8, 3, stride=2, padding=1, padding_mode="replicate"))
    net.add_module("odd", torch.nn.Conv2d(6, 8, 3, stride=2, padding=1))
    net.add_module("up4", torch.nn.ConvTranspose2d(8, 8, 4, stride=2, padding=1))
    keys, bound = list(net.state_dict().keys()), [m.forward.__func__ for m in net]
    served, left = encoders.install_native_strided(net)
    assert served == ["0", "1", "2"] and sorted(left) == ["3", "odd", "rep", "up4"]
    assert "padding" in left["3"] and "padding_mode" in left["rep"] and "channels" in left["odd"] and "kernel_size" in left["up4"]
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == keys
    assert all(("forward" in m.__dict__) == (n in served) for n, m in net.named_children())
    assert encoders.install_native_convs(net)[0] == ["s1"]                                       # the two installers share no layer
    encoders.uninstall_native_convs(net)
    x = torch.randn(1, 3, 12, 12, generator=torch.Generator().manual_seed(1))
    assert torch.equal(net[:4](x), twin(x))                                                      # CPU input: the module's own forward
    assert encoders.install_native_strided(net)[0] == served                                     # installing twice does not stack
    encoders.uninstall_native_strided(net)
    assert all("forward" not in m.__dict__ and not any(k.startswith("_kpnerf") for k in m.__dict__) for m in net)
    assert [m.forward.__func__ for m in net] == bound
