"""The arithmetic selector of the native convolution and of the fused ConvBlock on the MI355X: the C ABI on device memory (the same
checks as tests/test_conv_arith_cpu.py runs on the emulator), torch.ops.kpnerf.conv2d_arith / conv_block_arith under autograd, and the
installers' ``arith`` keyword.  Cases, rules and driver: tests/conv_arith_cases.py; every comparison is against the CPU fp64 result at the
standing bar, |native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor."""
import copy

import numpy as np
import pytest
import torch

from tests import block_cases as bc
from tests import conv_arith_cases as ca
from tests import conv_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def L3(L):
    return ca.ArithLib(L, ca.B3)


@pytest.fixture(scope="module")
def B():
    return ca.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("name", sorted(ca.CASES))
def test_abi_bf16x3_forward_and_gradients_against_fp64(L3, B, name):
    ca.check_case(L3, B, name)


def test_abi_the_own_cases_sit_where_their_rules_put_them(L3):
    ca.check_own_rules(L3)


@pytest.mark.parametrize("name", ["k5_12to36", "ranges3"])
def test_abi_f32_through_ex_has_the_bits_of_the_plain_entry_points(L, B, name):
    ca.check_f32_through_ex_has_the_bits_of_the_plain_entry_points(L, B, name)


def test_abi_two_calls_give_equal_bits(L3, B):
    ca.check_two_calls_equal_bits(L3, B, "k5_12to36")
    ca.check_two_calls_equal_bits(L3, B, "ranges3")


def test_abi_an_image_does_not_depend_on_its_batch(L3, B):
    ca.check_image_does_not_depend_on_batch(L3, B, "ranges3")


@pytest.mark.parametrize("name", ["k3_p2", "acc_empty"])
def test_abi_results_scale_exactly_with_powers_of_two(L3, B, name):
    ca.check_exponent_range(L3, B, name)


def test_abi_housekeeping(L, L3, B):
    cc.check_zero_dy_gives_zeros(L3, B, "k3_p0")
    cc.check_null_legs_leave_buffers_alone(L3, B, "k3_4to8")
    ca.check_packed_pieces(L3, B, "k5_12to36")
    ca.check_packs_of_the_two_arithmetics_differ_in_size(L)
    cc.check_bad_descriptors(L3, B)


def test_abi_a_bad_arith_is_refused_and_launches_nothing(L, B):
    ca.check_bad_arith(L, B)


@pytest.mark.parametrize("name", ca.BLOCKS)
def test_abi_block_against_fp64_and_against_its_legs(L3, B, name):
    bc.check_case(L3, B, name)
    ca.check_block_has_the_bits_of_its_legs(L3, B, name)


def test_abi_block_housekeeping(L3, B):
    bc.check_two_calls_equal_bits(L3, B, "d4to16")
    bc.check_zero_dy_gives_zeros(L3, B, "i32")
    bc.check_null_legs_leave_buffers_alone(L3, B, "d4to16")


# ---- torch.ops.kpnerf.conv2d_arith ----
def _op_run(name, arith, channels_last=True):
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = ca.CASES[name]
    (x, w, b, g), _, _ = ca.reference(name)
    xd = x.cuda().contiguous(memory_format=torch.channels_last) if channels_last else x.cuda().contiguous()
    xd.requires_grad_(True)
    wd = w.cuda().requires_grad_(True)
    bd = None if b is None else b.cuda().requires_grad_(True)
    y = torch.ops.kpnerf.conv2d_arith(xd, wd, bd, c["pad"], arith)
    (y * g.cuda()).sum().backward()
    return y.detach(), xd, wd, bd


@pytest.mark.parametrize("name", ["k3_4to8", "k5_12to36", "ranges3", "acc_empty"])
def test_op_conv2d_arith_autograd_against_fp64(name):
    _, r64, e_ref = ca.reference(name)
    for channels_last in (True, False):
        y, xd, wd, bd = _op_run(name, ca.B3, channels_last)
        assert y.is_contiguous(memory_format=torch.channels_last)
        assert xd.grad.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        cc.check(f"op {name} y", y.cpu().numpy(), r64["y"], e_ref["y"])
        cc.check(f"op {name} dx", xd.grad.cpu().numpy(), r64["dx"], e_ref["dx"])
        cc.check(f"op {name} dw", wd.grad.cpu().numpy(), r64["dw"], e_ref["dw"])
        if bd is not None:
            cc.check(f"op {name} db", bd.grad.cpu().numpy(), r64["db"], e_ref["db"])


def test_op_conv2d_arith_0_has_the_bits_of_conv2d():
    import keypointnerf_amd.torch_ops  # noqa: F401
    name = "k5_12to36"
    c = ca.CASES[name]
    (x, w, b, g), _, _ = ca.reference(name)
    y0, xd, wd, bd = _op_run(name, ca.F32)
    x1, w1, b1 = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y1 = torch.ops.kpnerf.conv2d(x1, w1, b1, c["pad"])
    (y1 * g.cuda()).sum().backward()
    assert torch.equal(y0, y1.detach()) and torch.equal(xd.grad, x1.grad) and torch.equal(wd.grad, w1.grad) and torch.equal(bd.grad, b1.grad)


def test_op_fake_kernels_and_refusals():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, w = torch.empty(2, 12, 9, 11, device="cuda"), torch.empty(36, 12, 5, 5, device="cuda")
        y = torch.ops.kpnerf.conv2d_arith(x, w, None, 1, 1)
        assert tuple(y.shape) == (2, 36, 7, 9) and y.is_contiguous(memory_format=torch.channels_last)
        dx, dw, db = torch.ops.kpnerf.conv2d_arith_backward(x, w, y, 1, 1, True, [True, True, False])
        assert dx.shape == x.shape and dw.shape == w.shape and db.numel() == 0
        c = bc.CASES["d16to32"]
        win, wout, ks = bc.widths(c)
        tensors = [torch.empty(s, device="cuda") for i in range(bc.legs_of(c)) for s in ((win[i],), (win[i],), (wout[i], win[i], ks[i], ks[i]))]
        xb = torch.empty(c["N"], c["cin"], c["H"], c["W"], device="cuda")
        yb = torch.ops.kpnerf.conv_block_arith(xb, tensors, 1e-5, 1)
        assert tuple(yb.shape) == (c["N"], c["cout"], c["H"], c["W"]) and yb.is_contiguous(memory_format=torch.channels_last)
        yb, state = torch.ops.kpnerf.conv_block_arith_cl(xb.contiguous(memory_format=torch.channels_last), tensors, 1e-5, 1)
        assert tuple(state.shape) == (bc.state_floats(c),)
        out = torch.ops.kpnerf.conv_block_arith_backward(xb, tensors, state, yb, 1e-5, 1, [True] * (1 + len(tensors)))
        assert [o.shape for o in out] == [xb.shape] + [t.shape for t in tensors]
    x = torch.zeros(1, 4, 8, 8, device="cuda")
    with pytest.raises(ValueError, match="arith must"):
        torch.ops.kpnerf.conv2d_arith(x, torch.zeros(4, 4, 3, 3, device="cuda"), None, 1, 2)
    with pytest.raises(ValueError, match="k must"):
        torch.ops.kpnerf.conv2d_arith(x, torch.zeros(4, 4, 7, 7, device="cuda"), None, 3, 1)


def test_a_pack_of_the_other_arithmetic_is_refused():
    from keypointnerf_amd import ops
    (x, w, b, g), _, _ = ca.reference("k3_4to8")
    xd, wd = x.cuda().contiguous(memory_format=torch.channels_last), w.cuda()
    p0, p3 = ops.conv2d_pack(wd), ops.conv2d_pack(wd, arith=ca.B3)
    assert p3.numel() > p0.numel()
    for packed, arith in ((p0, ca.B3), (p3, ca.F32)):
        with pytest.raises(ValueError, match="packed does not belong"):
            ops.conv2d_forward(xd, packed, None, 8, 3, 1, arith=arith)
        with pytest.raises(ValueError, match="packed does not belong"):
            ops.conv2d_backward(xd, g.cuda().contiguous(memory_format=torch.channels_last), packed, 4, 3, 1, False, arith=arith)


def test_op_pack_cache_has_the_arithmetic_in_its_key():
    from keypointnerf_amd import torch_ops
    C = torch_ops._ConvPackCache
    torch_ops.conv2d_cache_clear()
    c = ca.CASES["k3_p0"]
    (x, w, b, g), _, _ = ca.reference("k3_p0")
    xd, wd = x.cuda().contiguous(memory_format=torch.channels_last), w.cuda().requires_grad_(True)
    h0, m0 = C.hits, C.misses
    y1 = torch.ops.kpnerf.conv2d_arith(xd, wd, None, c["pad"], ca.B3)
    y2 = torch.ops.kpnerf.conv2d_arith(xd, wd, None, c["pad"], ca.B3)
    assert (C.misses - m0, C.hits - h0) == (1, 1) and torch.equal(y1, y2)
    y0 = torch.ops.kpnerf.conv2d(xd, wd, None, c["pad"])                # the same weight under the other arithmetic: a miss, never the
    assert (C.misses - m0, C.hits - h0) == (2, 1)                       # other's pack
    torch.ops.kpnerf.conv2d_arith(xd, wd, None, c["pad"], ca.F32)       # arith 0 shares the entry of kpnerf::conv2d
    assert (C.misses - m0, C.hits - h0) == (2, 2)
    assert torch.equal(torch.ops.kpnerf.conv2d_arith(xd, wd, None, c["pad"], ca.B3), y1) and (C.misses - m0, C.hits - h0) == (3, 2)
    with torch.no_grad():
        wd.mul_(2.0)                                                    # what an optimizer step does
    y3 = torch.ops.kpnerf.conv2d_arith(xd, wd, None, c["pad"], ca.B3)
    assert (C.misses - m0, C.hits - h0) == (4, 2) and torch.equal(y3, 2.0 * y1)          # a power of two: exact
    assert y0.shape == y1.shape
    torch_ops.conv2d_cache_clear()


# ---- torch.ops.kpnerf.conv_block_arith ----
def _block_op_run(name, arith, channels_last=True):
    import keypointnerf_amd.torch_ops  # noqa: F401
    net, x, g, _, _ = bc.reference(name)
    dev = copy.deepcopy(net).cuda()
    xd = x.cuda().contiguous(memory_format=torch.channels_last) if channels_last else x.cuda().contiguous()
    xd.requires_grad_(True)
    tensors = [t for bn, conv in bc.leg_modules(dev) for t in (bn.weight, bn.bias, conv.weight)]
    y = torch.ops.kpnerf.conv_block_arith(xd, tensors, bc.EPS, arith)
    (y * g.cuda()).sum().backward()
    return y.detach(), xd, dev


def _leg_grads(name, dev):
    """{parameter name: gradient} of the legs' parameters (a block with cin == cout holds a fourth norm that no leg uses)"""
    params = dict(dev.named_parameters())
    return {pname: params[pname].grad for pname in bc.param_names(bc.CASES[name]).values()}


@pytest.mark.parametrize("name", ca.BLOCKS)
def test_op_conv_block_arith_autograd_against_fp64(name):
    _, _, _, r64, e_ref = bc.reference(name)
    runs = []
    for channels_last in (True, False):
        y, xd, dev = _block_op_run(name, ca.B3, channels_last)
        bc.check(f"op {name} y", y.cpu().numpy(), r64["y"], e_ref["y"])
        bc.check(f"op {name} dx", xd.grad.cpu().numpy(), r64["dx"], e_ref["dx"])
        grads = _leg_grads(name, dev)
        for pname, grad in grads.items():
            bc.check(f"op {name} {pname}", grad.cpu().numpy(), r64[pname], e_ref[pname])
        runs.append([y, xd.grad] + list(grads.values()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))                 # an NCHW input gives the channels_last bits
    y0, x0, dev0 = _block_op_run(name, ca.F32)
    net, x, g, _, _ = bc.reference(name)
    dev1 = copy.deepcopy(net).cuda()
    x1 = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y1 = torch.ops.kpnerf.conv_block(x1, [t for bn, conv in bc.leg_modules(dev1) for t in (bn.weight, bn.bias, conv.weight)], bc.EPS)
    (y1 * g.cuda()).sum().backward()
    assert torch.equal(y0, y1.detach()) and torch.equal(x0.grad, x1.grad)
    assert all(torch.equal(a, b) for a, b in zip(_leg_grads(name, dev0).values(), _leg_grads(name, dev1).values()))


# ---- the installers' arith keyword ----
def test_install_native_blocks_bf16x3_fused_has_the_bits_of_the_unfused_path():
    from keypointnerf_amd import encoders
    for name in ca.BLOCKS:
        net, x, g, _, _ = bc.reference(name)
        outs = []
        for fused in (False, True):
            dev = copy.deepcopy(net).cuda()
            served, left = encoders.install_native_blocks(dev, fused=fused, arith="bf16x3")
            assert served == [""] and not left
            N = encoders.NativeTraining
            calls = (N.block_calls, N.fused_block_calls)
            xd = x.cuda().requires_grad_(True)
            y = dev(xd)
            (y * g.cuda()).sum().backward()
            assert (N.block_calls - calls[0], N.fused_block_calls - calls[1]) == ((0, 1) if fused else (1, 0))
            outs.append((y.detach(), xd.grad))
            encoders.uninstall_native_blocks(dev)
            assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
        assert torch.equal(outs[0][0], outs[1][0])
        _, _, _, r64, e_ref = bc.reference(name)
        for y, dx in outs:
            bc.check(f"installed {name} y", y.cpu().numpy(), r64["y"], e_ref["y"])
            bc.check(f"installed {name} dx", dx.cpu().numpy(), r64["dx"], e_ref["dx"])


def _train_geo(net, x, targets, steps=3):
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, foreach=False)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = sum(torch.nn.functional.mse_loss(y, t) for y, t in zip(net(x), targets))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, {n: p.detach() for n, p in net.named_parameters()}


def test_three_adam_steps_through_install_native_geo_bf16x3():
    """The narrow HGFilterV2 of tests/test_gpu_strided.py under install_native_geo(fused_blocks=True, arith="bf16x3"): which layers run on
    which arithmetic as the installer reports it, and three Adam steps against the CPU fp64 module by the compounding rule of
    tests/test_gpu_conv.py::test_three_adam_steps_through_the_native_convolutions - the drift of fp32 torch from fp64 torch over the same
    three steps is e_ref of each parameter tensor, and the native run may deviate from fp64 by 4 e_ref + 1 ulp.  fp32 torch is, as in
    every test on this network (tests/test_gpu_strided.py, tests/test_gpu_block.py), the larger deviation of two CPU fp32 runs, one
    contiguous and one channels_last: the native path runs channels_last, and the two torch runs differ from each other by up to 50x
    on single tensors (conv4.conv1.weight: 1.9e-7 contiguous, 6.3e-6 channels_last after three steps).  Measured on the MI355X with the
    contiguous run alone as e_ref, that tensor is the one over the bar for bf16x3 (6.9e-6, ratio 36) and for the fp32 kernels alike
    (3.3e-6, ratio 17), fused or not: the rule's e_ref, not an arithmetic, is what that shows."""
    from keypointnerf_amd import encoders
    from tests.test_gpu_strided import narrow_case
    net, x, gs = narrow_case()
    targets = [0.5 * g for g in gs]
    _, p64 = _train_geo(copy.deepcopy(net).double(), x.double(), [t.double() for t in targets])
    p32 = [_train_geo(copy.deepcopy(net), x.contiguous(memory_format=mf), targets)[1] for mf in (torch.contiguous_format, torch.channels_last)]
    dev = copy.deepcopy(net).cuda()
    with pytest.raises(ValueError, match="arith must"):
        encoders.install_native_geo(dev, fused_blocks=True, arith="f16x2")
    report = encoders.install_native_geo(dev, fused_blocks=True, arith="bf16x3")
    assert report["geo"] == ([""], {}) and all(not report[k][1] for k in report if k != "arith"), report
    blocks = sorted(n for n, m in dev.named_modules() if type(m).__name__ == "ConvBlock")
    assert len(blocks) == 8 and sorted(report["blocks"][0]) == blocks
    assert report["arith"] == {"bf16x3": sorted(blocks + ["conv_last0", "conv_out", "l0"]), "f32": ["conv1", "unpack1.conv"]}
    assert "arith" not in encoders.install_native_geo(copy.deepcopy(net).cuda(), fused_blocks=True)      # the default report is unchanged
    N = encoders.NativeTraining
    calls = (N.geo_calls, N.fused_block_calls, N.block_calls)
    losses, pn = _train_geo(dev, x.cuda(), [t.cuda() for t in targets])
    assert (N.geo_calls - calls[0], N.fused_block_calls - calls[1], N.block_calls - calls[2]) == (3, 3 * 8, 0)
    assert len(losses) == 3 and all(np.isfinite(losses))
    start = dict(net.named_parameters())
    for n, f64 in p64.items():
        moved = not torch.equal(f64.float(), start[n].detach())
        if ".bn4." in n and not moved:                                      # the unused bn4 of the blocks that keep their width
            assert torch.equal(pn[n].cpu(), start[n].detach())
            continue
        # (a bias in front of a norm has a zero gradient: it stays in fp64 and drifts by rounding noise in fp32 - e_ref says by how much)
        assert not moved or not torch.equal(pn[n].cpu(), start[n].detach()), n
        cc.check(f"adam x3 {n}", pn[n].cpu().numpy(), f64.numpy(), max(float((r[n].double() - f64).abs().max()) for r in p32))
    encoders.uninstall_native_geo(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
