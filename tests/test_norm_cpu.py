"""The native GroupNorm / InstanceNorm [+ ReLU] (kpn_group_norm_forward / kpn_group_norm_backward) on the host SIMT emulator: the
very kernel sources, with numpy buffers through the C ABI; and what of torch.ops.kpnerf.group_norm, install_native_norms and
install_native_blocks needs no GPU.  Cases, reference and bar: tests/norm_cases.py."""
import pytest
import torch

from tests import conv_cases as cc
from tests import norm_cases as nc
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = nc.HostArrays()


@pytest.mark.parametrize("relu", nc.RELU)
@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_forward_and_gradients_against_fp64(L, name, relu):
    nc.check_case(L, B, name, relu)


@pytest.mark.parametrize("name", ["chunks3", "in16", "offset", "gn4x8_ragged"])
def test_stats_buffer_holds_what_the_header_says(L, name):
    nc.check_stats_buffer(L, B, name)


def test_two_calls_give_equal_bits(L):
    nc.check_two_calls_equal_bits(L, B, "chunks3")


def test_null_legs_leave_their_buffers_untouched(L):
    nc.check_null_legs_leave_buffers_alone(L, B, "gn4x8_ragged")


def test_zero_dy_gives_exact_zeros(L):
    nc.check_zero_dy_gives_zeros(L, B, "offset")
    nc.check_zero_dy_gives_zeros(L, B, "in16", relu=0)


def test_bad_descriptors_are_refused_with_a_message(L):
    nc.check_bad_descriptors(L, B)


def test_workspace_covers_the_partial_and_coefficient_buffers(L):
    nc.check_workspace_covers_partials(L)


def test_fake_kernels_give_shapes_in_channels_last_and_there_is_no_cpu_kernel():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w, b = torch.empty(2, 64, 9, 11, device="cuda"), torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
        y = torch.ops.kpnerf.group_norm(x, w, b, 32, 1e-5, True)
        assert tuple(y.shape) == (2, 64, 9, 11) and y.is_contiguous(memory_format=torch.channels_last)
        y, stats = torch.ops.kpnerf.group_norm_cl(x.contiguous(memory_format=torch.channels_last), None, None, 64, 1e-5, False)
        assert y.is_contiguous(memory_format=torch.channels_last) and tuple(stats.shape) == (2 * 2 * 64 + 2 * 2 * 64,)
        dx, dw, db = torch.ops.kpnerf.group_norm_backward(x, w, stats, y, 32, 1e-5, True, [True, True, False])
        assert dx.shape == x.shape and tuple(dw.shape) == (64,) and db.numel() == 0
        dx, dw, db = torch.ops.kpnerf.group_norm_backward(x, None, stats, y, 64, 1e-5, False, [False, True, True])
        assert dx.numel() == 0 and dw.numel() == 0 and db.numel() == 0           # no parameters: no parameter gradients
    with pytest.raises((NotImplementedError, RuntimeError)):                     # no CPU kernel
        torch.ops.kpnerf.group_norm(torch.zeros(1, 8, 4, 4), None, None, 4, 1e-5, False)


def _norm_stack():
    nn = torch.nn
    net = cc.stand_in_stack()
    net.add_module("inorm", nn.InstanceNorm2d(8))
    net.add_module("odd", nn.GroupNorm(3, 12))
    net.add_module("in_affine", nn.InstanceNorm2d(8, affine=True))
    net.add_module("in_running", nn.InstanceNorm2d(8, track_running_stats=True))
    net.add_module("bn", nn.BatchNorm2d(8))
    return net


def test_install_native_norms_rebinds_only_eligible_layers_and_restores_them():
    from keypointnerf_amd import encoders
    net = _norm_stack()
    keys, bound = list(net.state_dict().keys()), [m.forward.__func__ for m in net]
    served, left = encoders.install_native_norms(net)
    assert served == ["1", "inorm"]
    assert sorted(left) == ["in_affine", "in_running", "odd"]                    # a BatchNorm2d is neither: not even listed
    assert "channels 12" in left["odd"] and "affine" in left["in_affine"] and "running" in left["in_running"]
    assert list(net.state_dict().keys()) == keys
    assert all(("forward" in m.__dict__) == (n in served) for n, m in net.named_children())
    # CPU tensors are none of the native path's business: the rebound forward hands them to the module's own forward
    x = torch.randn(1, 8, 6, 6, generator=torch.Generator().manual_seed(1))
    calls = encoders.NativeTraining.norm_calls
    twin = cc.stand_in_stack()
    assert torch.equal(net[:5](x), twin(x)) and torch.equal(net.inorm(x), torch.nn.InstanceNorm2d(8)(x))
    assert encoders.NativeTraining.norm_calls == calls
    assert encoders.install_native_norms(net)[0] == served                       # installing twice does not stack
    encoders.uninstall_native_norms(net)
    assert all("forward" not in m.__dict__ and "_kpnerf_norm_saved" not in m.__dict__ for m in net)
    assert [m.forward.__func__ for m in net] == bound


def _block_net(seed=3):
    from tests.encoder_golden import ConvBlock
    net = torch.nn.ModuleDict({"block": ConvBlock(16, 32), "plain": cc.stand_in_stack(), "odd": ConvBlock(24, 48)})
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * seed + i)) * (0.3 if p.dim() > 1 else 1.0))
    return net


def test_install_native_blocks_rebinds_only_conv_blocks_and_restores_them():
    from keypointnerf_amd import encoders
    net, twin = _block_net(), _block_net()
    keys = list(net.state_dict().keys())
    bound = {n: m.forward.__func__ for n, m in net.named_modules()}
    served, left = encoders.install_native_blocks(net)
    assert served == ["block"] and list(left) == ["odd"] and "powers of two" in left["odd"]      # the plain stack: not even listed
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == [n for n, _ in twin.named_parameters()]
    assert [n for n, m in net.named_modules() if "forward" in m.__dict__] == ["block"]
    # a ConvBlock whose structure is not the reference's is left alone with the refusal's text
    broken = _block_net()
    broken["block"].conv2 = torch.nn.Conv2d(16, 8, 3, padding=1, bias=True)
    assert "block.conv2" in encoders.install_native_blocks(broken)[1]["block"]
    x = torch.randn(1, 16, 6, 6, generator=torch.Generator().manual_seed(1))
    calls = encoders.NativeTraining.block_calls
    assert torch.equal(net["block"](x), twin["block"](x))                        # CPU input: the original forward
    assert encoders.NativeTraining.block_calls == calls
    assert encoders.install_native_blocks(net)[0] == served                      # installing twice does not stack
    # the three installers rebind different modules: any order of installing and uninstalling restores everything
    encoders.install_native_convs(net)
    encoders.install_native_norms(net)
    assert torch.equal(net["block"](x), twin["block"](x)) and torch.equal(net["plain"](x[:, :8]), twin["plain"](x[:, :8]))
    encoders.uninstall_native_blocks(net)
    assert "forward" not in net["block"].__dict__ and "forward" in net["block"].bn1.__dict__ and "forward" in net["block"].conv1.__dict__
    encoders.uninstall_native_convs(net)
    encoders.uninstall_native_norms(net)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)
    assert {n: m.forward.__func__ for n, m in net.named_modules()} == bound
