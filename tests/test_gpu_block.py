"""The single-operator ConvBlock on the MI355X: the C ABI on device memory (the same checks as tests/test_block_cpu.py runs on the
emulator), torch.ops.kpnerf.conv_block under autograd, encoders.install_native_blocks(fused=True) and
encoders.install_native_geo(fused_blocks=True).  Cases, reference and bar: tests/block_cases.py - every comparison against a
reference is against the CPU fp64 module, |native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor."""
import copy

import numpy as np
import pytest
import torch

from tests import block_cases as bc
from tests.parity import Spy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return bc.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_abi_forward_state_and_gradients_against_fp64(L, B, name):
    bc.check_case(L, B, name)


def test_abi_two_calls_give_equal_bits(L, B):
    bc.check_two_calls_equal_bits(L, B, "i16_ranges3")
    bc.check_two_calls_equal_bits(L, B, "d64to128")


def test_abi_null_legs_leave_their_buffers_untouched(L, B):
    bc.check_null_legs_leave_buffers_alone(L, B, "d4to16")
    bc.check_null_legs_leave_buffers_alone(L, B, "i32")


def test_abi_zero_dy_gives_exact_zeros(L, B):
    bc.check_zero_dy_gives_zeros(L, B, "d16to32")
    bc.check_zero_dy_gives_zeros(L, B, "i32")


def test_abi_bad_descriptors_are_refused_with_a_message(L, B):
    bc.check_bad_descriptors(L, B)


def test_abi_an_image_does_not_depend_on_its_batch(L, B):
    bc.check_image_does_not_depend_on_batch(L, B, "d16to32")
    bc.check_image_does_not_depend_on_batch(L, B, "i16_ranges3")


# ---- torch.ops.kpnerf.conv_block ----
def _tensors(net):
    return [t for bn, conv in bc.leg_modules(net) for t in (bn.weight, bn.bias, conv.weight)]


def _case_on_device(name):
    net, x, g, _, _ = bc.reference(name)
    dev = copy.deepcopy(net).cuda()
    return dev, x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True), g.cuda().contiguous(memory_format=torch.channels_last)


bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)  # noqa: E731


@pytest.mark.parametrize("name", ["d16to32", "i16_ranges3"])
def test_op_autograd_gives_the_abi_bits(L, B, name):
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = bc.CASES[name]
    y_abi, _, out = bc.run(L, B, name)
    dev, x, g = _case_on_device(name)
    tensors = _tensors(dev)
    y = torch.ops.kpnerf.conv_block(x, tensors, bc.EPS)
    grads = torch.autograd.grad(y, [x] + tensors, g)
    assert y.is_contiguous(memory_format=torch.channels_last) and grads[0].is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bits(y), bits(bc.nchw(y_abi))) and np.array_equal(bits(grads[0]), bits(bc.nchw(out["dx"])))
    keys = [(i, k) for i in range(bc.legs_of(c)) for k in ("dgamma", "dbeta", "dw")]
    for key, got in zip(keys, grads[1:]):
        assert np.array_equal(bits(got), bits(out[key])), key


def test_op_nchw_input_and_partial_gradients():
    """a contiguous NCHW x gives the channels_last bits, and asking for two gradients only gives those two, unchanged"""
    import keypointnerf_amd.torch_ops  # noqa: F401
    dev, x, g = _case_on_device("d16to32")
    tensors = _tensors(dev)
    full = torch.autograd.grad(torch.ops.kpnerf.conv_block(x, tensors, bc.EPS), [x] + tensors, g)
    xn = x.detach().contiguous().requires_grad_(True)
    yn = torch.ops.kpnerf.conv_block(xn, tensors, bc.EPS)
    assert yn.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(torch.autograd.grad(yn, [xn], g)[0], full[0])
    for p in dev.parameters():
        p.requires_grad_(False)
    dev.conv2.weight.requires_grad_(True)
    dev.bn4.bias.requires_grad_(True)
    y = torch.ops.kpnerf.conv_block(x.detach(), tensors, bc.EPS)
    got = torch.autograd.grad(y, [dev.conv2.weight, dev.bn4.bias], g)
    assert torch.equal(got[0], full[1 + 5]) and torch.equal(got[1], full[1 + 10])


def test_op_fake_kernels_agree_with_the_real_ones():
    import keypointnerf_amd.torch_ops  # noqa: F401
    for name in ("d16to32", "i32"):
        dev, x, g = _case_on_device(name)
        tensors = [t.detach() for t in _tensors(dev)]
        x = x.detach()
        checks = ("test_schema", "test_faketensor")
        torch.library.opcheck(torch.ops.kpnerf.conv_block_cl.default, (x, tensors, bc.EPS), test_utils=checks)
        _, state = torch.ops.kpnerf.conv_block_cl(x, tensors, bc.EPS)
        mask = [True] + [i % 2 == 0 for i in range(len(tensors))]
        torch.library.opcheck(torch.ops.kpnerf.conv_block_backward.default, (x, tensors, state, g, bc.EPS, mask), test_utils=checks)


# ---- install_native_blocks(fused=True) ----
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_fused_forward_has_the_bits_of_the_unfused_native_path(name):
    """Same kernels, same launch geometry, one commutative fp32 add for the residual: y of the fused operator equals y of the same
    block under install_native_blocks(fused=False), bit for bit"""
    from keypointnerf_amd import encoders
    dev, x, _ = _case_on_device(name)
    with torch.no_grad():
        assert encoders.install_native_blocks(dev)[0] == [""]
        plain = dev(x)
        assert encoders.install_native_blocks(dev, fused=True)[0] == [""]
        fused = dev(x)
    encoders.uninstall_native_blocks(dev)
    assert torch.equal(plain, fused)


INSIDE_A_BLOCK = ("aten::cat", "aten::add", "aten::convolution", "aten::native_group_norm", "aten::relu", "aten::threshold_backward",
                  "aten::_convolution", "aten::miopen_convolution", "aten::cudnn_convolution")


@pytest.mark.parametrize("name", ["d16to32", "i32"])
def test_a_fused_block_is_one_operator_forward_and_one_backward(name):
    from keypointnerf_amd import encoders
    dev, x, g = _case_on_device(name)
    assert encoders.install_native_blocks(dev, fused=True) == ([""], {})
    calls = encoders.NativeTraining.fused_block_calls, encoders.NativeTraining.block_calls
    with Spy() as spy:
        y = dev(x)
        torch.autograd.grad(y, [x] + _tensors(dev), g)
    assert (encoders.NativeTraining.fused_block_calls, encoders.NativeTraining.block_calls) == (calls[0] + 1, calls[1])
    bad = sorted({n for n in spy.names if n.startswith(INSIDE_A_BLOCK)})
    assert not bad, (bad, spy.names)
    assert sum(n.startswith("kpnerf::conv_block_cl") for n in spy.names) == 1
    assert sum(n.startswith("kpnerf::conv_block_backward") for n in spy.names) == 1
    assert not any(n.startswith(("kpnerf::conv2d", "kpnerf::group_norm")) for n in spy.names)
    encoders.uninstall_native_blocks(dev)
    assert "forward" not in dev.__dict__ and "_kpnerf_block_saved" not in dev.__dict__


def _saved_floats(net, x, least):
    """floats of the tensors that a forward of net(x) saves for its backward with numel >= least, one count per storage"""
    seen = {}

    def pack(t):
        if t.numel() >= least:
            seen[t.untyped_storage().data_ptr()] = max(seen.get(t.untyped_storage().data_ptr(), 0), t.numel())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = net(x)
    del y
    return sum(seen.values())


def test_a_fused_block_saves_at_most_its_input_and_three_quarters_of_its_output():
    """The bound is a condition, not a measurement: the fused operator saves x (cin P floats), `state` (3 cout / 4 P floats and the
    statistics) and the parameters, so the saved tensors of at least P = N H W elements total at most (cin + cout) P floats.  The shape
    keeps every parameter below P elements (the largest, conv1.weight, has 1152).  The unfused native path saves x, n1, o1, n2, o2 and
    n3: 3.5 C P floats for cin == cout == C; printed, not asserted."""
    from keypointnerf_amd import encoders
    C, N, H, W = 16, 2, 32, 32
    P = N * H * W
    dev = bc.block(C, C).cuda()
    assert max(p.numel() for p in dev.parameters()) < P
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(5)).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    encoders.install_native_blocks(dev)
    unfused = _saved_floats(dev, x, P)
    encoders.install_native_blocks(dev, fused=True)
    fused = _saved_floats(dev, x, P)
    encoders.uninstall_native_blocks(dev)
    print(f"[block saved activations] fused {fused} floats = {fused / (C * P):.3f} C P; unfused {unfused} floats = {unfused / (C * P):.3f} C P; "
          f"bound {(C + C) * P}")
    assert 0 < fused <= (C + C) * P


def test_install_native_blocks_fused_serves_and_restores_and_the_default_stays_unfused():
    from keypointnerf_amd import encoders, ops
    from tests.encoder_golden import ConvBlock
    net, x, g, r64, e_ref = bc.reference("d16to32")
    dev = copy.deepcopy(net).cuda()
    keys = list(dev.state_dict().keys())
    odd = ConvBlock(24, 48).cuda()
    served, left = encoders.install_native_blocks(odd, fused=True)
    assert served == [] and list(left) == [""] and "powers of two" in left[""] and "forward" not in odd.__dict__
    assert encoders.install_native_blocks(dev, fused=True) == ([""], {}) and list(dev.state_dict().keys()) == keys
    N_ = encoders.NativeTraining
    calls = N_.fused_block_calls
    got, _ = bc.block_run(dev, x.cuda(), g.cuda())
    assert N_.fused_block_calls == calls + 1
    for n, f64 in r64.items():
        if n not in ("o1", "o2"):
            bc.check(f"installed d16to32 {n}", got[n].cpu().numpy(), f64, e_ref[n])
    encoders.uninstall_native_blocks(dev)
    assert "forward" not in dev.__dict__ and "_kpnerf_block_saved" not in dev.__dict__
    # the default is what it was: one group_norm and one conv2d per leg
    assert encoders.install_native_blocks(dev) == ([""], {})
    seen = {"norm": 0, "conv": 0}
    real_n, real_c = ops.group_norm_forward, ops.conv2d_forward
    ops.group_norm_forward = lambda *a, **kw: (seen.__setitem__("norm", seen["norm"] + 1), real_n(*a, **kw))[1]
    ops.conv2d_forward = lambda *a, **kw: (seen.__setitem__("conv", seen["conv"] + 1), real_c(*a, **kw))[1]
    calls = N_.block_calls, N_.fused_block_calls
    try:
        with torch.no_grad():
            dev(x.cuda())
    finally:
        ops.group_norm_forward, ops.conv2d_forward = real_n, real_c
    assert (N_.block_calls, N_.fused_block_calls) == (calls[0] + 1, calls[1]) and seen == {"norm": 4, "conv": 4}
    encoders.uninstall_native_blocks(dev)
    assert "forward" not in dev.__dict__


# ---- install_native_geo(fused_blocks=True) ----
def test_a_narrow_hgfilter_trains_with_fused_blocks():
    """The narrow HGFilterV2 of tests/test_gpu_strided.py under install_native_geo(fused_blocks=True), held to that test's bar: both
    outputs and every parameter gradient against the CPU fp64 module, e_ref the larger deviation of two CPU fp32 runs; the ReLU-margin
    condition on the reference alone.  No torch.cat is left (every one the network has sits in a ConvBlock), and every block is one
    kpnerf::conv_block_cl with one kpnerf::conv_block_backward."""
    from keypointnerf_amd import encoders
    from tests import layer_op_checks as loc
    from tests import strided_cases as sc
    from tests import test_gpu_strided as tgs
    net, x, gs = tgs.narrow_case()
    margin, e_pre = loc.narrow_margin(net, x, loc.group_norms, tgs.NARROW_NORMS)
    assert margin > 8.0 * e_pre, (margin, e_pre)
    r64 = tgs._param_grads(copy.deepcopy(net).double(), x.double(), [g.double() for g in gs])
    runs32 = [tgs._param_grads(copy.deepcopy(net), x.contiguous(memory_format=mf), gs) for mf in (torch.contiguous_format, torch.channels_last)]
    dev = copy.deepcopy(net).cuda()
    keys = list(dev.state_dict().keys())
    report = encoders.install_native_geo(dev, fused_blocks=True)
    assert report["geo"] == ([""], {}) and all(not left for _, left in report.values()), report
    n_blocks = sum(type(m).__name__ == "ConvBlock" for m in dev.modules())
    assert len(report["blocks"][0]) == n_blocks == 8 and list(dev.state_dict().keys()) == keys
    N_ = encoders.NativeTraining
    calls = N_.geo_calls, N_.fused_block_calls, N_.block_calls
    with Spy() as spy:
        got = tgs._param_grads(dev, x.cuda(), [g.cuda() for g in gs])
    assert (N_.geo_calls, N_.fused_block_calls, N_.block_calls) == (calls[0] + 1, calls[1] + n_blocks, calls[2])
    bad = sorted({n for n in spy.names if n.startswith(tgs.FORBIDDEN + ("aten::cat",))})
    assert not bad, bad
    assert sum(n.startswith("kpnerf::conv_block_cl") for n in spy.names) == n_blocks
    assert sum(n.startswith("kpnerf::conv_block_backward") for n in spy.names) == n_blocks
    for n, f64 in r64.items():
        if f64 is None:                                                 # the unused bn4 of the blocks that keep their width
            assert ".bn4." in n and got[n] is None
            continue
        e_ref = max(float((r[n].double() - f64).abs().max()) for r in runs32)
        sc.check(f"narrow fused {n}", got[n].cpu().numpy(), f64.numpy(), e_ref)
    encoders.uninstall_native_geo(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
