"""The native resampling steps of an HourGlass on the MI355X: the C ABI on device memory (the same checks as
tests/test_resample_cpu.py runs on the emulator, and the case that needs a second grid-stride iteration), torch.ops.kpnerf.avg_pool2 /
upsample2x_add under autograd, and encoders.install_native_hourglass.  Cases, reference and bar: tests/resample_cases.py - every
comparison is against the CPU fp64 result, |native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor, e_ref the deviation of CPU fp32
torch from the same fp64 result."""
import copy

import numpy as np
import pytest
import torch

from tests import layer_op_checks as loc
from tests import resample_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return rc.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("name", sorted(rc.GPU_CASES))
def test_abi_forward_and_gradients_against_fp64(L, B, name):
    rc.check_case(L, B, name)


@pytest.mark.parametrize("name", sorted(rc.GPU_CASES))
def test_abi_pool_backward_is_exact(L, B, name):
    rc.check_pool_backward_is_exact(L, B, name)


@pytest.mark.parametrize("name", sorted(rc.GPU_CASES))
def test_abi_skip_forms_agree(L, B, name):
    rc.check_skip_forms_agree(L, B, name)


@pytest.mark.parametrize("name", ["interior", "hg", "stride"])
def test_abi_two_calls_give_equal_bits(L, B, name):
    rc.check_two_calls_equal_bits(L, B, name)


def test_abi_an_image_does_not_depend_on_its_batch(L, B):
    rc.check_an_image_does_not_depend_on_its_batch(L, B)


@pytest.mark.parametrize("name", ["one", "clamp", "interior"])
def test_abi_zero_dy_gives_exact_zeros(L, B, name):
    rc.check_zero_dy_gives_zeros(L, B, name)


def test_abi_bad_calls_are_refused_with_a_message(L, B):
    rc.check_refusals(L, B)


# ---- torch.ops.kpnerf.avg_pool2 / upsample2x_add ----
def _cl(t, grad=True):
    return t.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def _same_bits(t, nhwc_array):
    return np.array_equal(rc.bits(t.detach().cpu().numpy()), rc.bits(rc.nchw(nhwc_array)))


@pytest.mark.parametrize("name", ["clamp", "hg"])
def test_ops_under_autograd_give_the_abi_bits(L, B, name):
    import keypointnerf_amd.torch_ops  # noqa: F401
    t = rc.reference(name)[0]
    abi = rc.run(L, B, name)
    x, low, skip = _cl(t["x"]), _cl(t["low"]), _cl(t["skip"])
    py = torch.ops.kpnerf.avg_pool2(x)
    uy = torch.ops.kpnerf.upsample2x_add(low, skip)
    (py * t["g_low"].cuda()).sum().backward()
    (uy * t["g_high"].cuda()).sum().backward()
    cl = torch.channels_last
    assert all(v.is_contiguous(memory_format=cl) for v in (py, uy, x.grad, low.grad))
    assert _same_bits(py, abi["pool_y"]) and _same_bits(x.grad, abi["pool_dx"])
    assert _same_bits(uy, abi["up_y"]) and _same_bits(low.grad, abi["up_dlow"])
    assert torch.equal(skip.grad, t["g_high"].cuda())                   # the skip's gradient is dy itself
    # without a skip: the interpolation alone, the same d_low
    low2 = _cl(t["low"])
    alone = torch.ops.kpnerf.upsample2x_add(low2, None)
    (alone * t["g_high"].cuda()).sum().backward()
    assert _same_bits(alone, rc.up_forward(L, B, rc.GPU_CASES[name], rc.nhwc(t["low"]))) and _same_bits(low2.grad, abi["up_dlow"])
    # NCHW-contiguous input is converted once and gives the same values
    x_nchw = t["x"].cuda().requires_grad_(True)
    assert torch.equal(torch.ops.kpnerf.avg_pool2(x_nchw), py)


def test_d_low_is_not_computed_when_low_needs_no_gradient():
    from keypointnerf_amd import ops
    import keypointnerf_amd.torch_ops  # noqa: F401
    t = rc.reference("hg")[0]
    seen = {"up": 0, "pool": 0}
    real_u, real_p = ops.upsample2x_add_backward, ops.avg_pool2_backward
    ops.upsample2x_add_backward = lambda *a: (seen.__setitem__("up", seen["up"] + 1), real_u(*a))[1]
    ops.avg_pool2_backward = lambda *a: (seen.__setitem__("pool", seen["pool"] + 1), real_p(*a))[1]
    try:
        low, skip = _cl(t["low"], grad=False), _cl(t["skip"])
        (torch.ops.kpnerf.upsample2x_add(low, skip) * t["g_high"].cuda()).sum().backward()
        assert seen == {"up": 0, "pool": 0} and low.grad is None and torch.equal(skip.grad, t["g_high"].cuda())
        low, skip = _cl(t["low"]), _cl(t["skip"], grad=False)
        (torch.ops.kpnerf.upsample2x_add(low, skip) * t["g_high"].cuda()).sum().backward()
        assert seen == {"up": 1, "pool": 0} and skip.grad is None and low.grad is not None
        x = _cl(t["x"])
        (torch.ops.kpnerf.avg_pool2(x) * t["g_low"].cuda()).sum().backward()
        assert seen == {"up": 1, "pool": 1}
    finally:
        ops.upsample2x_add_backward, ops.avg_pool2_backward = real_u, real_p


def test_ops_raise_on_what_they_do_not_serve():
    from keypointnerf_amd import ops
    with pytest.raises(RuntimeError):
        ops.avg_pool2_forward(torch.zeros(1, 4, 2, 2))                  # a CPU tensor
    with pytest.raises(ValueError):
        ops.avg_pool2_forward(torch.zeros(1, 4, 3, 2, device="cuda").contiguous(memory_format=torch.channels_last))     # odd height
    with pytest.raises(ValueError):
        ops.upsample2x_add_forward(torch.zeros(1, 6, 2, 2, device="cuda").contiguous(memory_format=torch.channels_last))  # C % 4
    with pytest.raises(ValueError):
        ops.upsample2x_add_forward(torch.zeros(1, 4, 2, 2, device="cuda").contiguous(memory_format=torch.channels_last),
                                   torch.zeros(1, 4, 2, 2, device="cuda").contiguous(memory_format=torch.channels_last))  # the skip's size


# ---- install_native_hourglass ----
def _grads(net, x, g, memory_format=torch.contiguous_format):
    """-> {"y", "dx", parameter name: gradient or None}"""
    x = x.clone().contiguous(memory_format=memory_format).requires_grad_(True)
    y = net(x)
    params = dict(net.named_parameters())
    grads = torch.autograd.grad(y, [x] + list(params.values()), g, allow_unused=True)
    out = {"y": y.detach(), "dx": grads[0]}
    out.update(dict(zip(params, grads[1:])))
    return out


def test_wiring_without_a_relu_to_flip():
    """the recursion around 1x1 convolutions, install_native_hourglass alone: output, input gradient and every parameter gradient
    against the CPU fp64 module"""
    from keypointnerf_amd import encoders
    net = rc.seed_parameters(rc.HourGlass(2, 8), 3)
    gen = torch.Generator().manual_seed(7)
    x, g = torch.randn(2, 8, 8, 12, generator=gen), torch.randn(2, 8, 8, 12, generator=gen)
    r64 = _grads(copy.deepcopy(net).double(), x.double(), g.double())
    r32 = _grads(copy.deepcopy(net), x, g)
    dev = copy.deepcopy(net).cuda()
    keys = list(dev.state_dict().keys())
    served, left = encoders.install_native_hourglass(dev)
    assert served == [""] and left == {} and list(dev.state_dict().keys()) == keys
    calls = encoders.NativeTraining.hourglass_calls
    got = _grads(dev, x.cuda(), g.cuda())
    assert encoders.NativeTraining.hourglass_calls == calls + 1
    assert sorted(got) == sorted(r64) and all(v is not None for v in r64.values())
    for n, f64 in r64.items():
        rc.check(f"wiring {n}", got[n].cpu().numpy(), f64.numpy(), float((r32[n].double() - f64).abs().max()))
    # a size the recursion cannot halve twice goes to the original forward, which fails on it as the untouched module does
    calls = encoders.NativeTraining.hourglass_calls
    with pytest.raises(RuntimeError, match="must match the size"):
        dev(torch.randn(1, 8, 6, 8, generator=gen).cuda())
    assert encoders.NativeTraining.hourglass_calls == calls
    encoders.uninstall_native_hourglass(dev)
    assert "forward" not in dev.__dict__ and "_kpnerf_hourglass_saved" not in dev.__dict__


@pytest.mark.parametrize("depth,shape,seed", [(2, (1, 16, 8, 8), 2), (1, (2, 16, 4, 6), 1)])
def test_the_real_hourglass_trains_on_the_native_kernels(depth, shape, seed):
    """tests/encoder_golden.HourGlass with install_native_hourglass + install_native_blocks against the CPU fp64 module.  e_ref per
    tensor is the larger deviation of two CPU fp32 runs, one contiguous and one channels_last (the rule of
    tests/test_gpu_norm.py::test_install_native_blocks_matches_the_block_in_fp64).  First, on the reference alone: the smallest
    |GroupNorm output| over all norms exceeds 8x the largest fp32 deviation of those outputs - no rounding can flip a ReLU mask."""
    from keypointnerf_amd import encoders
    from tests.encoder_golden import HourGlass
    net = rc.seed_parameters(HourGlass(depth, 16), seed)
    gen = torch.Generator().manual_seed(seed)
    x, g = torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen)
    formats = (torch.contiguous_format, torch.channels_last)
    dev_err = lambda a, b: float((a.double() - b).abs().max())
    pre64 = loc.norm_outputs(copy.deepcopy(net).double(), x.double(), torch.contiguous_format)
    pre32 = [loc.norm_outputs(copy.deepcopy(net), x, mf) for mf in formats]
    assert len(pre64) == 3 * (3 * depth + 1)                            # bn1 .. bn3 of every block; bn4 never runs
    margin = min(float(p.abs().min()) for p in pre64.values())
    e_pre = max(dev_err(r[n], p) for r in pre32 for n, p in pre64.items())
    print(f"[hourglass {depth}] min|GroupNorm output| {margin:.3e} against 8 e_ref = {8 * e_pre:.3e}")
    assert margin > 8.0 * e_pre, (margin, e_pre)
    r64 = _grads(copy.deepcopy(net).double(), x.double(), g.double())
    runs32 = [_grads(copy.deepcopy(net), x, g, mf) for mf in formats]
    dev = copy.deepcopy(net).cuda()
    keys = list(dev.state_dict().keys())
    served, left = encoders.install_native_hourglass(dev)
    assert served == [""] and left == {}
    served, left = encoders.install_native_blocks(dev)
    assert len(served) == 3 * depth + 1 and left == {} and list(dev.state_dict().keys()) == keys
    hg_calls, block_calls = encoders.NativeTraining.hourglass_calls, encoders.NativeTraining.block_calls
    got = _grads(dev, x.cuda(), g.cuda())
    assert encoders.NativeTraining.hourglass_calls == hg_calls + 1
    assert encoders.NativeTraining.block_calls == block_calls + 3 * depth + 1
    for n, f64 in r64.items():
        if f64 is None:                                                 # the unused bn4 of every block: no gradient on either side
            assert ".bn4." in n and got[n] is None
            continue
        e_ref = max(dev_err(r[n], f64) for r in runs32)
        rc.check(f"hourglass {depth} {n}", got[n].cpu().numpy(), f64.numpy(), e_ref)
    assert sum(v is None for v in r64.values()) == 2 * (3 * depth + 1)
    encoders.uninstall_native_blocks(dev)
    encoders.uninstall_native_hourglass(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
