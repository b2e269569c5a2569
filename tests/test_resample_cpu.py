"""The native resampling steps of an HourGlass (kpn_avg_pool2_* / kpn_upsample2x_add_*) on the host SIMT emulator: the very kernel
sources, with numpy buffers through the C ABI; and what of torch.ops.kpnerf.avg_pool2 / upsample2x_add and install_native_hourglass
needs no GPU.  Cases, reference and bar: tests/resample_cases.py."""
import pytest
import torch

from tests import resample_cases as rc
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = rc.HostArrays()


def test_the_library_reports_abi_10(L):
    assert L.kpn_abi_version() == 10


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_forward_and_gradients_against_fp64(L, name):
    rc.check_case(L, B, name)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_pool_backward_is_exact(L, name):
    rc.check_pool_backward_is_exact(L, B, name)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_skip_forms_agree(L, name):
    rc.check_skip_forms_agree(L, B, name)


def test_two_calls_give_equal_bits(L):
    rc.check_two_calls_equal_bits(L, B, "interior")
    rc.check_two_calls_equal_bits(L, B, "hg")


def test_an_image_does_not_depend_on_its_batch(L):
    rc.check_an_image_does_not_depend_on_its_batch(L, B)


@pytest.mark.parametrize("name", ["one", "clamp", "interior"])
def test_zero_dy_gives_exact_zeros(L, name):
    rc.check_zero_dy_gives_zeros(L, B, name)


def test_bad_calls_are_refused_with_a_message(L):
    rc.check_refusals(L, B)


def test_fake_kernels_give_shapes_in_channels_last_and_there_is_no_cpu_kernel():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    cl = torch.channels_last
    with FakeTensorMode():
        x = torch.empty(2, 8, 6, 10, device="cuda")
        y = torch.ops.kpnerf.avg_pool2(x)
        assert tuple(y.shape) == (2, 8, 3, 5) and y.is_contiguous(memory_format=cl)
        y = torch.ops.kpnerf.avg_pool2_cl(x.contiguous(memory_format=cl))
        assert tuple(y.shape) == (2, 8, 3, 5) and y.is_contiguous(memory_format=cl)
        for skip in (x, None):
            z = torch.ops.kpnerf.upsample2x_add(y, skip)
            assert tuple(z.shape) == (2, 8, 6, 10) and z.is_contiguous(memory_format=cl)
        z = torch.ops.kpnerf.upsample2x_add_cl(y, x.contiguous(memory_format=cl))
        assert tuple(z.shape) == (2, 8, 6, 10) and z.is_contiguous(memory_format=cl)
        dx = torch.ops.kpnerf.avg_pool2_backward(y)
        assert tuple(dx.shape) == (2, 8, 6, 10) and dx.is_contiguous(memory_format=cl)
        d_low = torch.ops.kpnerf.upsample2x_add_backward(z)
        assert tuple(d_low.shape) == (2, 8, 3, 5) and d_low.is_contiguous(memory_format=cl)
    for call in (lambda: torch.ops.kpnerf.avg_pool2(torch.zeros(1, 4, 2, 2)),
                 lambda: torch.ops.kpnerf.upsample2x_add(torch.zeros(1, 4, 1, 1), torch.zeros(1, 4, 2, 2)),
                 lambda: torch.ops.kpnerf.avg_pool2_backward(torch.zeros(1, 4, 1, 1)),
                 lambda: torch.ops.kpnerf.upsample2x_add_backward(torch.zeros(1, 4, 2, 2))):
        with pytest.raises((NotImplementedError, RuntimeError)):                 # no CPU kernel
            call()


def _hourglass_net(seed=3):
    from tests.encoder_golden import ConvBlock, HourGlass
    nn = torch.nn
    net = nn.ModuleDict({
        "hg": HourGlass(2, 16),                                                  # the real structure
        "wired": rc.HourGlass(1, 8),                                             # the same recursion around 1x1 convolutions
        "odd": rc.HourGlass(1, 6),                                               # features no multiple of 4
        "shallow": rc.HourGlass(1, 8),                                           # depth says 2, the children are those of depth 1
        "nodepth": rc.HourGlass(1, 8),
        "block": ConvBlock(16, 16),                                              # no HourGlass: not even listed
    })
    net["shallow"].depth = 2
    net["nodepth"].depth = None
    return rc.seed_parameters(net, seed)


def test_install_native_hourglass_rebinds_only_eligible_hourglasses_and_restores_them():
    from keypointnerf_amd import encoders
    net, twin = _hourglass_net(), _hourglass_net()
    keys = list(net.state_dict().keys())
    bound = {n: m.forward.__func__ for n, m in net.named_modules()}
    served, left = encoders.install_native_hourglass(net)
    assert served == ["hg", "wired"] and sorted(left) == ["nodepth", "odd", "shallow"]
    assert "features=6" in left["odd"] and "depth=None" in left["nodepth"]
    assert "missing children" in left["shallow"] and "b1_2" in left["shallow"] and "b3_2" in left["shallow"]
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == [n for n, _ in twin.named_parameters()]
    assert [n for n, m in net.named_modules() if "forward" in m.__dict__] == ["hg", "wired"]
    # CPU tensors are none of the native path's business: the rebound forward hands them to the module's own forward
    gen = torch.Generator().manual_seed(1)
    x16, x8 = torch.randn(1, 16, 8, 8, generator=gen), torch.randn(2, 8, 4, 6, generator=gen)
    calls = encoders.NativeTraining.hourglass_calls
    assert torch.equal(net["hg"](x16), twin["hg"](x16)) and torch.equal(net["wired"](x8), twin["wired"](x8))
    assert encoders.NativeTraining.hourglass_calls == calls
    assert encoders.install_native_hourglass(net)[0] == served                   # installing twice does not stack
    assert net["hg"].__dict__["_kpnerf_hourglass_saved"] is None
    encoders.uninstall_native_hourglass(net)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)
    assert {n: m.forward.__func__ for n, m in net.named_modules()} == bound


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1), (1, 3, 0, 2)])
def test_the_four_installers_restore_every_forward_in_any_order(order):
    from keypointnerf_amd import encoders
    pairs = [(encoders.install_native_hourglass, encoders.uninstall_native_hourglass),
             (encoders.install_native_blocks, encoders.uninstall_native_blocks),
             (encoders.install_native_norms, encoders.uninstall_native_norms),
             (encoders.install_native_convs, encoders.uninstall_native_convs)]
    net, twin = _hourglass_net(), _hourglass_net()
    bound = {n: m.forward.__func__ for n, m in net.named_modules()}
    for i in order:
        pairs[i][0](net)
    assert "forward" in net["hg"].__dict__ and "forward" in net["hg"].b1_2.__dict__ and "forward" in net["hg"].b1_2.bn1.__dict__
    x = torch.randn(1, 16, 8, 8, generator=torch.Generator().manual_seed(1))
    assert torch.equal(net["hg"](x), twin["hg"](x))                              # CPU input: every layer's original forward
    for i in sorted(order, key=lambda i: (order.index(i) * 3 + 1) % 4):          # uninstall in another order than installed
        pairs[i][1](net)
        assert ("forward" in net["hg"].__dict__) == ("_kpnerf_hourglass_saved" in net["hg"].__dict__)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)
    assert {n: m.forward.__func__ for n, m in net.named_modules()} == bound
