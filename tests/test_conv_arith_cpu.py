"""The arithmetic selector of the native convolution and of the fused ConvBlock (kpn_conv2d_ex_*, kpn_conv_block_ex_*) on the host SIMT
emulator: the very kernel sources (csrc/encoder_split_kernels.hip for KPN_CONV_BF16X3), with numpy buffers through the C ABI.  Cases,
rules and driver: tests/conv_arith_cases.py; reference and bar: tests/conv_cases.py, tests/block_cases.py."""
import pytest

from tests import block_cases as bc
from tests import conv_arith_cases as ca
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


@pytest.fixture(scope="module")
def L3(L):
    return ca.ArithLib(L, ca.B3)


B = ca.HostArrays()


@pytest.mark.parametrize("name", sorted(ca.CASES))
def test_bf16x3_forward_and_gradients_against_fp64(L3, name):
    ca.check_case(L3, B, name)


def test_the_own_cases_sit_where_their_rules_put_them(L3):
    ca.check_own_rules(L3)


@pytest.mark.parametrize("name", ["k5_12to36", "ranges3"])
def test_f32_through_ex_has_the_bits_of_the_plain_entry_points(L, name):
    ca.check_f32_through_ex_has_the_bits_of_the_plain_entry_points(L, B, name)


def test_two_calls_give_equal_bits(L3):
    ca.check_two_calls_equal_bits(L3, B, "k5_12to36")


def test_an_image_does_not_depend_on_its_batch(L3):
    ca.check_image_does_not_depend_on_batch(L3, B, "ranges3")


@pytest.mark.parametrize("name", ["k3_p2", "acc_empty"])
def test_results_scale_exactly_with_powers_of_two(L3, name):
    ca.check_exponent_range(L3, B, name)


def test_zero_dy_gives_exact_zeros(L3):
    ca.cc.check_zero_dy_gives_zeros(L3, B, "k3_p0")


def test_null_legs_leave_their_buffers_untouched(L3):
    ca.cc.check_null_legs_leave_buffers_alone(L3, B, "k3_4to8")


def test_packed_copies_hold_three_pieces_and_zero_padding(L3):
    ca.check_packed_pieces(L3, B, "k5_12to36")       # cin 12 / cout 36: padded channels in both copies, K = 300 / 900: padded taps


def test_packs_of_the_two_arithmetics_differ_in_size(L):
    ca.check_packs_of_the_two_arithmetics_differ_in_size(L)


def test_a_bad_arith_is_refused_and_launches_nothing(L):
    ca.check_bad_arith(L, B)


def test_the_descriptor_refusals_hold_for_bf16x3(L3):
    ca.cc.check_bad_descriptors(L3, B)


@pytest.mark.parametrize("name", ca.BLOCKS)
def test_block_forward_state_and_gradients_against_fp64(L3, name):
    bc.check_case(L3, B, name)


@pytest.mark.parametrize("name", ca.BLOCKS)
def test_block_has_the_bits_of_the_block_computed_leg_by_leg(L3, name):
    ca.check_block_has_the_bits_of_its_legs(L3, B, name)


def test_block_housekeeping(L3):
    bc.check_two_calls_equal_bits(L3, B, "d4to16")
    bc.check_zero_dy_gives_zeros(L3, B, "i32")
    bc.check_null_legs_leave_buffers_alone(L3, B, "d4to16")


# ---- what of the Python layers needs no GPU ----
def test_fake_kernels_give_shapes_and_there_is_no_cpu_kernel():
    import torch
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w = torch.empty(2, 12, 9, 11, device="cuda"), torch.empty(36, 12, 5, 5, device="cuda")
        y = torch.ops.kpnerf.conv2d_arith(x, w, None, 1, 1)
        assert tuple(y.shape) == (2, 36, 7, 9) and y.is_contiguous(memory_format=torch.channels_last)
        c = bc.CASES["i32"]
        win, wout, ks = bc.widths(c)
        tensors = [torch.empty(s, device="cuda") for i in range(bc.legs_of(c)) for s in ((win[i],), (win[i],), (wout[i], win[i], ks[i], ks[i]))]
        yb = torch.ops.kpnerf.conv_block_arith(torch.empty(c["N"], c["cin"], c["H"], c["W"], device="cuda"), tensors, 1e-5, 1)
        assert tuple(yb.shape) == (c["N"], c["cout"], c["H"], c["W"]) and yb.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises((NotImplementedError, RuntimeError)):             # no CPU kernel
        torch.ops.kpnerf.conv2d_arith(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3), None, 1, 1)


def test_installers_take_the_arith_keyword_and_restore_as_before():
    import torch
    from keypointnerf_amd import encoders
    net, twin = ca.cc.stand_in_stack(), ca.cc.stand_in_stack()
    bound = [m.forward.__func__ for m in net]
    for fn in (encoders.install_native_convs, encoders.install_native_blocks, encoders.install_native_geo):
        with pytest.raises(ValueError, match="arith must"):
            fn(net, arith="f16x2")
    assert all("forward" not in m.__dict__ for m in net)                 # a refused keyword rebinds nothing
    served, left = encoders.install_native_convs(net, arith="bf16x3")
    assert served == ["0", "3"] and list(left) == ["4"] and "stride=2" in left["4"]          # the same layers as the default serves
    x = torch.randn(1, 8, 6, 6, generator=torch.Generator().manual_seed(1))
    assert torch.equal(net(x), twin(x))                                  # CPU input: the module's own forward
    assert encoders.install_native_convs(net)[0] == served               # switching the arithmetic does not stack
    encoders.uninstall_native_convs(net)
    assert all("forward" not in m.__dict__ and "_kpnerf_conv_saved" not in m.__dict__ for m in net)
    assert [m.forward.__func__ for m in net] == bound
    blocks = torch.nn.ModuleDict({"block": bc.block(16, 32), "same": bc.block(16, 16)})
    for fused in (False, True):
        assert encoders.install_native_blocks(blocks, fused=fused, arith="bf16x3") == (["block", "same"], {})
    encoders.uninstall_native_blocks(blocks)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in blocks.modules() for k in m.__dict__)
