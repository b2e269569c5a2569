"""The native convolution on the MI355X: the C ABI on device memory (the same checks as tests/test_conv_cpu.py runs on the emulator),
torch.ops.kpnerf.conv2d under autograd, and encoders.install_native_convs on a small stack.  Cases, reference and bar:
tests/conv_cases.py - every comparison is against the CPU fp64 result, |native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor,
e_ref the deviation of CPU fp32 torch from the same fp64 result."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cc
from tests import layer_op_checks as loc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return cc.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_abi_forward_and_gradients_against_fp64(L, B, name):
    cc.check_case(L, B, name)


def test_abi_two_calls_give_equal_bits(L, B):
    cc.check_two_calls_equal_bits(L, B, "k5_12to36")
    cc.check_two_calls_equal_bits(L, B, "ranges3")


def test_abi_null_legs_leave_their_buffers_untouched(L, B):
    cc.check_null_legs_leave_buffers_alone(L, B, "k3_4to8")


def test_abi_zero_dy_gives_exact_zeros(L, B):
    cc.check_zero_dy_gives_zeros(L, B, "k3_p0")


def test_abi_bad_descriptors_are_refused_with_a_message(L, B):
    cc.check_bad_descriptors(L, B)


def test_abi_wgrad_range_counts_follow_the_stated_rule(L):
    cc.check_range_counts(L)


# ---- torch.ops.kpnerf.conv2d ----
def _op(c):
    return c, lambda x, w, b: torch.ops.kpnerf.conv2d(x, w, b, c["pad"])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_op_autograd_against_fp64(name):
    _, r64, e_ref = cc.reference(name)
    y, xd, wd, bd = loc.op_run(cc.FAMILY, _op, name)
    assert y.is_contiguous(memory_format=torch.channels_last) and xd.grad.is_contiguous(memory_format=torch.channels_last)
    cc.check(f"op {name} y", y.cpu().numpy(), r64["y"], e_ref["y"])
    cc.check(f"op {name} dx", xd.grad.cpu().numpy(), r64["dx"], e_ref["dx"])
    cc.check(f"op {name} dw", wd.grad.cpu().numpy(), r64["dw"], e_ref["dw"])
    if bd is not None:
        cc.check(f"op {name} db", bd.grad.cpu().numpy(), r64["db"], e_ref["db"])


def test_op_launches_only_the_legs_that_need_a_gradient(monkeypatch):
    loc.check_op_launches_only_needed_legs(monkeypatch, cc.FAMILY, _op, "conv2d_backward", ("k3_4to8",), name_in_label=False)


def test_op_pack_cache_is_reused_and_rebuilt_after_an_in_place_update():
    from keypointnerf_amd import torch_ops
    C = torch_ops._ConvPackCache
    torch_ops.conv2d_cache_clear()
    c = cc.CASES["k3_p0"]
    (x, w, b, g), _, _ = cc.reference("k3_p0")
    xd, wd = x.cuda().contiguous(memory_format=torch.channels_last), w.cuda().requires_grad_(True)
    h0, m0 = C.hits, C.misses
    y1 = torch.ops.kpnerf.conv2d(xd, wd, None, c["pad"])
    y2 = torch.ops.kpnerf.conv2d(xd, wd, None, c["pad"])
    (y2 * g.cuda()).sum().backward()                                    # the backward's dX leg is off (x needs no gradient): no lookup
    assert (C.misses - m0, C.hits - h0) == (1, 1) and torch.equal(y1, y2)
    xg = xd.clone().requires_grad_(True)
    (torch.ops.kpnerf.conv2d(xg, wd, None, c["pad"]) * g.cuda()).sum().backward()
    assert (C.misses - m0, C.hits - h0) == (1, 3)                       # forward and the dX leg of the backward: two hits
    with torch.no_grad():
        wd.mul_(2.0)                                                    # what an optimizer step does
    y3 = torch.ops.kpnerf.conv2d(xd, wd, None, c["pad"])
    assert (C.misses - m0, C.hits - h0) == (2, 3)
    assert torch.equal(y3, 2.0 * y1)                                    # a power of two: exact
    with torch.inference_mode():
        wi = w.cuda()
        n = len(C.entries)
        torch.ops.kpnerf.conv2d(xd.clone(), wi, None, c["pad"])
        torch.ops.kpnerf.conv2d(xd.clone(), wi, None, c["pad"])
    assert len(C.entries) == n and (C.misses - m0, C.hits - h0) == (2, 3)       # inference tensors get no cache
    torch_ops.conv2d_cache_clear()
    assert len(C.entries) == 0


def test_op_nchw_input_gives_the_channels_last_bits():
    loc.check_op_nchw_bits(cc.FAMILY, _op, ("k5_12to36", "k3_p2"))


def test_op_fake_kernel_shapes_and_refusals():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w = torch.empty(2, 12, 9, 11, device="cuda"), torch.empty(36, 12, 5, 5, device="cuda")
        y = torch.ops.kpnerf.conv2d(x, w, None, 1)
        assert tuple(y.shape) == (2, 36, 7, 9) and y.is_contiguous(memory_format=torch.channels_last)
    x = torch.zeros(1, 4, 8, 8, device="cuda")
    with pytest.raises(ValueError, match="k must"):
        torch.ops.kpnerf.conv2d(x, torch.zeros(4, 4, 7, 7, device="cuda"), None, 3)
    with pytest.raises(ValueError, match="cin must"):
        torch.ops.kpnerf.conv2d(torch.zeros(1, 6, 8, 8, device="cuda"), torch.zeros(4, 6, 3, 3, device="cuda"), None, 1)
    with pytest.raises(ValueError, match="pad must"):
        torch.ops.kpnerf.conv2d(x, torch.zeros(4, 4, 3, 3, device="cuda"), None, 3)


def test_ops_calls_of_one_shape_share_one_plan_and_keep_the_bits_of_the_abi(L, B):
    """keypointnerf_amd.ops on the smallest case: two forward and two backward calls build one plan (ops._layer_plan) and give
    equal bits, the layer with one image more builds a second plan and has the bits of the C-ABI driver"""
    loc.check_ops_plan_once_per_shape(cc.FAMILY, L, B, ("k3_p0",))


# ---- install_native_convs ----
_stack = cc.stand_in_stack


def _stack_grads(net, x, g):
    x = x.clone().requires_grad_(True)
    (net(x) * g).sum().backward()
    return [x.grad] + [p.grad for p in net.parameters()]


def test_install_native_convs_serves_the_eligible_layers_and_matches_fp64():
    from keypointnerf_amd import encoders
    net = _stack()
    gen = torch.Generator().manual_seed(11)
    x, g = torch.randn(2, 8, 10, 14, generator=gen), torch.randn(2, 8, 5, 7, generator=gen)
    r64 = _stack_grads(copy.deepcopy(net).double(), x.double(), g.double())
    r32 = _stack_grads(copy.deepcopy(net), x, g)
    dev = copy.deepcopy(net).cuda()
    keys, bound = list(dev.state_dict().keys()), [m.forward.__func__ for m in dev]
    served, left = encoders.install_native_convs(dev)
    assert served == ["0", "3"] and list(left) == ["4"] and "stride=2" in left["4"]
    assert list(dev.state_dict().keys()) == keys and [n for n, _ in dev.named_parameters()] == keys
    calls = []
    from keypointnerf_amd import ops
    real = ops.conv2d_forward
    ops.conv2d_forward = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    try:
        got = _stack_grads(dev, x.cuda(), g.cuda())
    finally:
        ops.conv2d_forward = real
    assert len(calls) == 2                                              # both served layers ran natively
    names = ["x"] + keys
    for n, a, f64, f32 in zip(names, got, r64, r32):
        e_ref = float((f32.double() - f64).abs().max())
        cc.check(f"stack d{n}", a.cpu().numpy(), f64.numpy(), e_ref)
    encoders.uninstall_native_convs(dev)
    assert all("forward" not in m.__dict__ and "_kpnerf_conv_saved" not in m.__dict__ for m in dev)
    assert [m.forward.__func__ for m in dev] == bound


def _train(net, x, target, steps=3):
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, foreach=False)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.mse_loss(net(x), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, [p.detach() for p in net.parameters()]


def test_three_adam_steps_through_the_native_convolutions():
    """N = 3, 32 x 32.  The bar compounds over the steps by the same rule: the drift of fp32 torch from fp64 torch over the same
    three steps is e_ref of each parameter tensor, and the native run may deviate from fp64 by 4 e_ref + 1 ulp."""
    from keypointnerf_amd import encoders
    net = _stack(5)
    gen = torch.Generator().manual_seed(21)
    x, target = torch.randn(3, 8, 32, 32, generator=gen), torch.randn(3, 8, 16, 16, generator=gen)
    _, p64 = _train(copy.deepcopy(net).double(), x.double(), target.double())
    _, p32 = _train(copy.deepcopy(net), x, target)
    dev = copy.deepcopy(net).cuda()
    encoders.install_native_convs(dev)
    losses, pn = _train(dev, x.cuda(), target.cuda())
    assert len(losses) == 3 and all(np.isfinite(losses))
    for (n, _), a, f64, f32 in zip(net.named_parameters(), pn, p64, p32):
        assert not torch.equal(a.cpu(), dict(net.named_parameters())[n].detach()), n     # it moved
        cc.check(f"adam x3 {n}", a.cpu().numpy(), f64.numpy(), float((f32.double() - f64).abs().max()))
