"""The native GroupNorm / InstanceNorm [+ ReLU] on the MI355X: the C ABI on device memory (the same checks as tests/test_norm_cpu.py
runs on the emulator), torch.ops.kpnerf.group_norm under autograd, and encoders.install_native_norms / install_native_blocks.
Cases, reference and bar: tests/norm_cases.py - every comparison is against the CPU fp64 result,
|native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor, e_ref the deviation of CPU fp32 torch from the same fp64 result."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cc
from tests import norm_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return nc.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("relu", nc.RELU)
@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_abi_forward_and_gradients_against_fp64(L, B, name, relu):
    nc.check_case(L, B, name, relu)


def test_abi_stats_buffer_holds_what_the_header_says(L, B):
    nc.check_stats_buffer(L, B, "chunks3")
    nc.check_stats_buffer(L, B, "in16")


def test_abi_two_calls_give_equal_bits(L, B):
    nc.check_two_calls_equal_bits(L, B, "chunks3")
    nc.check_two_calls_equal_bits(L, B, "c1024")


def test_abi_null_legs_leave_their_buffers_untouched(L, B):
    nc.check_null_legs_leave_buffers_alone(L, B, "gn4x8_ragged")


def test_abi_zero_dy_gives_exact_zeros(L, B):
    nc.check_zero_dy_gives_zeros(L, B, "offset")


def test_abi_bad_descriptors_are_refused_with_a_message(L, B):
    nc.check_bad_descriptors(L, B)


def test_abi_an_image_does_not_depend_on_its_batch(L, B):
    """image 1 of chunks3 alone and inside the batch of three: y and dx have equal bits"""
    name, relu = "chunks3", 1
    c = nc.CASES[name]
    (x, gamma, beta, g), _, _ = nc.reference(name, relu)
    y3, _, out3 = nc.run(L, B, name, relu)
    c1 = dict(c, N=1)
    x1, g1 = nc.nhwc(x[1:2]), nc.nhwc(g[1:2])
    y1, stats1 = nc.forward(L, B, c1, relu, x1, gamma.numpy(), beta.numpy())
    dx1 = nc.backward(L, B, c1, relu, x1, g1, gamma.numpy(), stats1, legs=("dx",))["dx"]
    assert np.array_equal(y1.view(np.uint32), y3[1:2].view(np.uint32))
    assert np.array_equal(dx1.view(np.uint32), out3["dx"][1:2].view(np.uint32))


# ---- torch.ops.kpnerf.group_norm ----
def _op_run(name, relu, inplace_relu=False):
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = nc.CASES[name]
    (x, gamma, beta, g), _, _ = nc.reference(name, 1 if inplace_relu else relu)
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd, bd = (gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)) if c["affine"] else (None, None)
    y = torch.ops.kpnerf.group_norm(xd, wd, bd, c["G"], nc.EPS, bool(relu))
    if inplace_relu:
        y = F.relu_(y)                                                  # the reference's nl = ReLU(inplace=True)
    (y * g.cuda()).sum().backward()
    return y.detach(), xd, wd, bd


@pytest.mark.parametrize("relu", nc.RELU)
def test_op_autograd_gives_the_abi_bits(L, B, relu):
    name = "gn32x64"
    y_abi, _, out = nc.run(L, B, name, relu)
    y, xd, wd, bd = _op_run(name, relu)
    assert y.is_contiguous(memory_format=torch.channels_last) and xd.grad.is_contiguous(memory_format=torch.channels_last)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(y.cpu().numpy()), bits(nc.nchw(y_abi)))
    assert np.array_equal(bits(xd.grad.cpu().numpy()), bits(nc.nchw(out["dx"])))
    assert np.array_equal(bits(wd.grad.cpu().numpy()), bits(out["dgamma"]))
    assert np.array_equal(bits(bd.grad.cpu().numpy()), bits(out["dbeta"]))


def test_op_survives_an_in_place_relu_on_its_output():
    """norm without ReLU, then relu_ on its result, then backward: y is not what the backward reads.  Held to the relu = 1 reference."""
    name = "gn32x64"
    _, r64, e_ref = nc.reference(name, 1)
    y, xd, wd, bd = _op_run(name, 0, inplace_relu=True)
    nc.check("in-place relu y", y.cpu().numpy(), r64["y"], e_ref["y"])
    nc.check("in-place relu dx", xd.grad.cpu().numpy(), r64["dx"], e_ref["dx"])
    nc.check("in-place relu dgamma", wd.grad.cpu().numpy(), r64["dgamma"], e_ref["dgamma"])
    nc.check("in-place relu dbeta", bd.grad.cpu().numpy(), r64["dbeta"], e_ref["dbeta"])


def test_op_instance_norm_has_no_parameter_gradients():
    _, r64, e_ref = nc.reference("in16", 0)
    y, xd, wd, bd = _op_run("in16", 0)
    assert wd is None and bd is None
    nc.check("op in16 dx", xd.grad.cpu().numpy(), r64["dx"], e_ref["dx"])


# ---- install_native_norms ----
def _grads(net, x, g, memory_format=torch.contiguous_format):
    x = x.clone().contiguous(memory_format=memory_format).requires_grad_(True)
    y = net(x)
    (y * g).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in net.parameters()]


def test_install_native_norms_serves_the_eligible_layers_and_matches_fp64():
    from keypointnerf_amd import encoders
    net = cc.stand_in_stack()
    gen = torch.Generator().manual_seed(11)
    x, g = torch.randn(2, 8, 10, 14, generator=gen), torch.randn(2, 8, 5, 7, generator=gen)
    r64 = _grads(copy.deepcopy(net).double(), x.double(), g.double())
    r32 = _grads(copy.deepcopy(net), x, g)
    dev = copy.deepcopy(net).cuda()
    keys, bound = list(dev.state_dict().keys()), [m.forward.__func__ for m in dev]
    served, left = encoders.install_native_norms(dev)
    assert served == ["1"] and left == {}
    assert list(dev.state_dict().keys()) == keys and [n for n, _ in dev.named_parameters()] == keys
    calls = encoders.NativeTraining.norm_calls
    got = _grads(dev, x.cuda(), g.cuda())
    assert encoders.NativeTraining.norm_calls == calls + 1              # the norm ran natively
    for n, a, f64, f32 in zip(["y", "x"] + keys, got, r64, r32):
        nc.check(f"norm stack {n}", a.cpu().numpy(), f64.numpy(), float((f32.double() - f64).abs().max()))
    encoders.uninstall_native_norms(dev)
    assert all("forward" not in m.__dict__ and "_kpnerf_norm_saved" not in m.__dict__ for m in dev)
    assert [m.forward.__func__ for m in dev] == bound


# ---- install_native_blocks ----
def _block(cin, cout, seed=3):
    from tests.encoder_golden import ConvBlock
    net = ConvBlock(cin, cout)
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * seed + i)) * (0.3 if p.dim() > 1 else 1.0))
    return net


def _block_run(net, x, g, memory_format=torch.contiguous_format):
    """-> ({tensor name: value}, {norm name: its output before the in-place ReLU})"""
    pre, hooks = {}, []
    for n in ("bn1", "bn2", "bn3", "bn4"):
        hooks.append(getattr(net, n).register_forward_hook(lambda m, i, o, n=n: pre.__setitem__(n, o.detach().clone())))
    x = x.clone().contiguous(memory_format=memory_format).requires_grad_(True)
    y = net(x)
    (y * g).sum().backward()
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "dx": x.grad}
    out.update({n: p.grad for n, p in net.named_parameters()})
    return out, pre


@pytest.mark.parametrize("cin,cout,hw", [(16, 32, (8, 8)), (32, 32, (6, 10))])
def test_install_native_blocks_matches_the_block_in_fp64(cin, cout, hw):
    """A ConvBlock is a chain of seven ops: e_ref per tensor is the larger deviation of two CPU fp32 runs from fp64, one contiguous
    and one channels_last (a mere fp32 reordering already reaches 3x the single-run e_ref).  The factor 4 and the ulp term stay."""
    from keypointnerf_amd import encoders, ops
    net = _block(cin, cout)
    gen = torch.Generator().manual_seed(1003)
    x, g = torch.randn(2, cin, *hw, generator=gen), torch.randn(2, cout, *hw, generator=gen)
    r64, pre64 = _block_run(copy.deepcopy(net).double(), x.double(), g.double())
    runs32 = [_block_run(copy.deepcopy(net), x, g, mf) for mf in (torch.contiguous_format, torch.channels_last)]
    dev_err = lambda a, b: float((a.double() - b).abs().max())
    # no rounding can flip a ReLU mask: every norm's pre-activation clears 8 e_ref, on the reference alone
    assert sorted(pre64) == (["bn1", "bn2", "bn3", "bn4"] if cin != cout else ["bn1", "bn2", "bn3"])
    for n, p in pre64.items():
        e_pre, margin = max(dev_err(r[1][n], p) for r in runs32), float(p.abs().min())
        print(f"[block {cin}->{cout}] {n}: min|pre-activation| {margin:.3e} against 8 e_ref = {8 * e_pre:.3e}")
        assert margin > 8.0 * e_pre, (n, margin, e_pre)
    dev = copy.deepcopy(net).cuda()
    keys = list(dev.state_dict().keys())
    served, left = encoders.install_native_blocks(dev)
    assert served == [""] and left == {} and list(dev.state_dict().keys()) == keys
    seen = {"norm": 0, "conv": 0}
    real_n, real_c = ops.group_norm_forward, ops.conv2d_forward
    ops.group_norm_forward = lambda *a, **kw: (seen.__setitem__("norm", seen["norm"] + 1), real_n(*a, **kw))[1]
    ops.conv2d_forward = lambda *a, **kw: (seen.__setitem__("conv", seen["conv"] + 1), real_c(*a, **kw))[1]
    calls = encoders.NativeTraining.block_calls
    try:
        got, _ = _block_run(dev, x.cuda(), g.cuda())
    finally:
        ops.group_norm_forward, ops.conv2d_forward = real_n, real_c
    legs = 4 if cin != cout else 3
    assert encoders.NativeTraining.block_calls == calls + 1 and seen == {"norm": legs, "conv": legs}      # the native ops ran
    for n, f64 in r64.items():
        if f64 is None:                                                 # bn4 of the equal-width block: no gradient on either side
            assert cin == cout and n.startswith("bn4.") and got[n] is None
            continue
        e_ref = max(dev_err(r[0][n], f64) for r in runs32)
        nc.check(f"block {cin}->{cout} {n}", got[n].cpu().numpy(), f64.numpy(), e_ref)
    if cin == cout:
        assert r64["bn4.weight"] is None and r64["bn4.bias"] is None
    encoders.uninstall_native_blocks(dev)
    assert "forward" not in dev.__dict__ and "_kpnerf_block_saved" not in dev.__dict__
