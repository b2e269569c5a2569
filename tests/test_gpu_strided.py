"""The native stride-2, stem and transposed convolutions on the MI355X: the C ABI on device memory (the same checks as
tests/test_strided_cpu.py runs on the emulator), torch.ops.kpnerf.conv2d_down2 / conv_transpose2d_up2 under autograd,
encoders.install_native_strided on a small stack and encoders.install_native_geo on a narrow and on the full-width HGFilterV2.
Cases, reference and bar: tests/strided_cases.py - every comparison is against the CPU fp64 result,
|native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor, e_ref the deviation of CPU fp32 torch from the same fp64 result."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from tests import encoder_golden as eg
from tests import layer_op_checks as loc
from tests import strided_cases as sc
from tests.parity import Spy
from tests.resample_cases import seed_parameters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return sc.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_abi_forward_and_gradients_against_fp64(L, B, name):
    sc.check_case(L, B, name)


@pytest.mark.parametrize("name", sc.ONE_PER_KIND + ("s2_ranges", "stem_ranges", "up_ranges"))
def test_abi_two_calls_give_equal_bits(L, B, name):
    sc.check_two_calls_equal_bits(L, B, name)


@pytest.mark.parametrize("name", ("s2_4to8", "stem_3to64", "up_8to4"))
def test_abi_null_legs_leave_their_buffers_untouched(L, B, name):
    sc.check_null_legs_leave_buffers_alone(L, B, name)


@pytest.mark.parametrize("name", sc.ONE_PER_KIND)
def test_abi_zero_dy_gives_exact_zeros(L, B, name):
    sc.check_zero_dy_gives_zeros(L, B, name)


def test_abi_wgrad_range_counts_follow_the_stated_rule(L):
    sc.check_range_counts(L)


def test_abi_the_padded_stem_channel_is_never_read(L, B):
    sc.check_padded_stem_channel(L, B)


def test_abi_bad_calls_are_refused_with_a_message_and_launch_nothing(L, B):
    sc.check_refusals(L, B)


# ---- torch.ops.kpnerf.conv2d_down2 / conv_transpose2d_up2 ----
def _op(c):
    return c, (torch.ops.kpnerf.conv_transpose2d_up2 if c["kind"] == sc.DECONV3 else torch.ops.kpnerf.conv2d_down2)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_op_autograd_gives_the_bits_of_the_abi(L, B, name):
    """the operators under autograd run the very ABI calls: y, dX, dW, db equal the driver's bits (and so meet the bar against fp64)"""
    c = sc.CASES[name]
    (x, w, b, g), _, _ = sc.reference(name)
    packed = sc.pack(L, B, c, w.numpy())
    y_abi = sc.forward(L, B, c, sc.x_layout(c, x), packed, None if b is None else b.numpy())
    abi = sc.backward(L, B, c, sc.x_layout(c, x), sc.nhwc(g), packed)
    y, xd, wd, bd = loc.op_run(sc.FAMILY, _op, name)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.cpu(), torch.from_numpy(sc.nchw(y_abi)))
    assert torch.equal(wd.grad.cpu(), torch.from_numpy(abi["dw"]))
    if c["kind"] != sc.STEM7:
        assert xd.grad.is_contiguous(memory_format=torch.channels_last) and torch.equal(xd.grad.cpu(), torch.from_numpy(sc.nchw(abi["dx"])))
    if bd is not None:
        assert torch.equal(bd.grad.cpu(), torch.from_numpy(abi["db"]))


def test_op_launches_only_the_legs_that_need_a_gradient(monkeypatch):
    loc.check_op_launches_only_needed_legs(monkeypatch, sc.FAMILY, _op, "conv2d_s2_backward", ("s2_4to8", "up_8to4"), stem_name="stem_3to64")


def test_op_nchw_input_gives_the_channels_last_bits():
    loc.check_op_nchw_bits(sc.FAMILY, _op, ("s2_12to36", "up_36to12", "stem_odd"))


def test_the_stem_op_raises_on_an_input_that_requires_a_gradient():
    import keypointnerf_amd.torch_ops  # noqa: F401
    (x, w, b, g), _, _ = sc.reference("stem_odd")
    with pytest.raises(RuntimeError, match="no input gradient"):
        torch.ops.kpnerf.conv2d_down2(x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), None)
    with pytest.raises(ValueError, match="kernel size"):
        torch.ops.kpnerf.conv2d_down2(x.cuda(), torch.zeros(8, 3, 5, 5, device="cuda"), None)
    with pytest.raises(ValueError, match="H, W must be even"):
        torch.ops.kpnerf.conv2d_down2(torch.zeros(1, 4, 5, 6, device="cuda"), torch.zeros(4, 4, 3, 3, device="cuda"), None)


def test_ops_calls_of_one_shape_share_one_plan_and_keep_the_bits_of_the_abi(L, B):
    """keypointnerf_amd.ops on the smallest case and on a stem: two forward and two backward calls build one plan (ops._layer_plan) and give
    equal bits, the layer with one image more builds a second plan and has the bits of the C-ABI driver; the stem refuses a dx"""
    loc.check_ops_plan_once_per_shape(sc.FAMILY, L, B, ("s2_2x2",), stem_name="stem_odd")


# ---- install_native_strided ----
def _stack(seed=4):
    net = nn.Sequential(nn.Conv2d(3, 8, 7, stride=2, padding=3), nn.Conv2d(8, 16, 3, stride=2, padding=1),
                        nn.ConvTranspose2d(16, 8, 3, stride=2, padding=1, output_padding=1), nn.Conv2d(8, 8, 3, stride=2, padding=0))
    return seed_parameters(net, seed)


_param_grads = functools.partial(loc.param_grads, allow_unused=True)      # the blocks that keep their width never run their bn4


def test_install_native_strided_serves_the_eligible_layers_and_matches_fp64():
    from keypointnerf_amd import encoders
    net = _stack()
    gen = torch.Generator().manual_seed(12)
    x, g = torch.randn(2, 3, 16, 24, generator=gen), torch.randn(2, 8, 3, 5, generator=gen)
    r64 = _param_grads(copy.deepcopy(net).double(), x.double(), [g.double()])
    r32 = _param_grads(copy.deepcopy(net), x, [g])
    dev = copy.deepcopy(net).cuda()
    keys, bound = list(dev.state_dict().keys()), [m.forward.__func__ for m in dev]
    served, left = encoders.install_native_strided(dev)
    assert served == ["0", "1", "2"] and list(left) == ["3"] and "padding" in left["3"]
    assert list(dev.state_dict().keys()) == keys and [n for n, _ in dev.named_parameters()] == keys
    calls = encoders.NativeTraining.strided_calls
    got = _param_grads(dev, x.cuda(), [g.cuda()])
    assert encoders.NativeTraining.strided_calls == calls + 3
    for n, f64 in r64.items():
        sc.check(f"stack {n}", got[n].cpu().numpy(), f64.numpy(), float((r32[n].double() - f64).abs().max()))
    encoders.uninstall_native_strided(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
    assert [m.forward.__func__ for m in dev] == bound


# ---- install_native_geo ----
class HGFilterV2(nn.Module):
    """a narrow HGFilterV2 of the reference's structure (n_stack = 1, hd = False): stem 3 -> 8, blocks 8 -> 16 -> 16 -> 32,
    HourGlass(1, 32).  The class name is what install_native_geo looks for.  Stem 3 -> 16, blocks 16 -> 32 -> 32 -> 64 and
    HourGlass(2, 64) on 32 x 32 were tried first: with 62,000 GroupNorm outputs no seed in 0 .. 9 keeps the smallest of them above
    8x the fp32 deviation (the margin assertion of the test below), so the net was narrowed, the factor kept."""

    def __init__(self):
        super().__init__()
        self.n_stack, self.hd = 1, False
        self.nl = nn.ReLU(True)
        self.unpack1 = eg.DeconvReLUGroup(16, 8)
        self.conv_out = nn.Conv2d(8, 8, 5, padding=2)
        self.conv1 = nn.Conv2d(3, 8, 7, stride=2, padding=3)
        self.bn1 = nn.GroupNorm(8, 8)
        self.conv2, self.conv3, self.conv4 = eg.ConvBlock(8, 16), eg.ConvBlock(16, 16), eg.ConvBlock(16, 32)
        self.m0 = eg.HourGlass(1, 32)
        self.top_m_0 = eg.ConvBlock(32, 32)
        self.conv_last0 = nn.Conv2d(32, 32, 1)
        self.bn_end0 = nn.GroupNorm(32, 32)
        self.l0 = nn.Conv2d(32, 16, 1)

    forward = eg.HGFilterV2.forward


# Chosen on the CPU: of the seeds 0 .. 9 this one leaves the widest margin (3.1e-4 against 8 e_ref = 4.1e-5)
NARROW_SEED = 8
NARROW_NORMS = 3 + 4 * 2 + 3 * 6        # bn1, unpack1.norm, bn_end0; conv2 / conv4 with their bn4; conv3, top_m_0 and the 4 hourglass blocks without


def narrow_case(seed=NARROW_SEED):
    net = seed_parameters(HGFilterV2(), seed)
    gen = torch.Generator().manual_seed(50 + seed)
    return net, torch.randn(1, 3, 16, 16, generator=gen), [torch.randn(1, 16, 4, 4, generator=gen), torch.randn(1, 8, 16, 16, generator=gen)]


FORBIDDEN = ("aten::convolution", "aten::convolution_backward", "aten::native_group_norm", "aten::avg_pool2d", "aten::upsample_bicubic2d",
             "aten::relu", "aten::threshold_backward", "aten::cudnn_convolution", "aten::miopen_convolution", "aten::_convolution")


def test_a_narrow_hgfilter_trains_on_the_native_kernels_alone():
    """install_native_geo on the narrow HGFilterV2 against the CPU fp64 module: both outputs and every parameter gradient.  e_ref per
    tensor is the larger deviation of two CPU fp32 runs, one contiguous and one channels_last (the rule of
    tests/test_gpu_resample.py::test_the_real_hourglass_trains_on_the_native_kernels).  First, on the reference alone: the smallest
    |GroupNorm output| over all norms exceeds 8x the largest fp32 deviation of those outputs - no rounding can flip a ReLU mask.
    Under a dispatch spy over forward and backward no aten convolution, group norm, pool, bicubic upsample or ReLU runs."""
    from keypointnerf_amd import encoders
    net, x, gs = narrow_case()
    margin, e_pre = loc.narrow_margin(net, x, loc.group_norms, NARROW_NORMS)
    print(f"[narrow HGFilterV2] min|GroupNorm output| {margin:.3e} against 8 e_ref = {8 * e_pre:.3e}")
    assert margin > 8.0 * e_pre, (margin, e_pre)
    r64 = _param_grads(copy.deepcopy(net).double(), x.double(), [g.double() for g in gs])
    runs32 = [_param_grads(copy.deepcopy(net), x.contiguous(memory_format=mf), gs) for mf in (torch.contiguous_format, torch.channels_last)]
    dev = copy.deepcopy(net).cuda()
    keys, names = list(dev.state_dict().keys()), [n for n, _ in dev.named_parameters()]
    report = encoders.install_native_geo(dev)
    assert report["geo"] == ([""], {}) and all(not left for _, left in report.values()), report
    assert sorted(report["strided"][0]) == ["conv1", "unpack1.conv"] and len(report["blocks"][0]) == 4 + 4 and report["hourglass"][0] == ["m0"]
    assert sorted(report["convs"][0]) == sorted(n for n, m in dev.named_modules() if type(m) is nn.Conv2d and n != "conv1")
    assert list(dev.state_dict().keys()) == keys and [n for n, _ in dev.named_parameters()] == names
    calls = encoders.NativeTraining.geo_calls
    with Spy() as spy:
        got = _param_grads(dev, x.cuda(), [g.cuda() for g in gs])
    assert encoders.NativeTraining.geo_calls == calls + 1
    bad = sorted({n for n in spy.names if n.startswith(FORBIDDEN)})
    assert not bad, bad
    assert any(n.startswith("kpnerf::conv2d_down2_cl") for n in spy.names) and any(n.startswith("kpnerf::conv2d_s2_backward") for n in spy.names)
    for n, f64 in r64.items():
        if f64 is None:                                                 # the unused bn4 of the blocks that keep their width
            assert ".bn4." in n and got[n] is None
            continue
        e_ref = max(float((r[n].double() - f64).abs().max()) for r in runs32)
        sc.check(f"narrow {n}", got[n].cpu().numpy(), f64.numpy(), e_ref)
    encoders.uninstall_native_geo(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)


def test_the_full_width_hgfilter_runs_and_repeats_on_the_native_kernels():
    """tests/encoder_golden.HGFilterV2 on 1 x 3 x 64 x 64 with install_native_geo: nothing is left on torch, the forward meets the bar
    against the CPU fp64 module (a ReLU is continuous: a flipped mask cannot hurt a forward), every gradient is finite and two runs
    agree bit for bit.  No gradient value is compared at this width: mask flips are unavoidable there."""
    from keypointnerf_amd import encoders
    net = eg.stand_in_geo(3).train()
    gen = torch.Generator().manual_seed(31)
    x = 2.0 * torch.rand(1, 3, 64, 64, generator=gen) - 1.0
    gs = [torch.randn(1, 64, 16, 16, generator=gen), torch.randn(1, 8, 64, 64, generator=gen)]
    with torch.no_grad():
        y64 = copy.deepcopy(net).double()(x.double())
        y32 = [copy.deepcopy(net)(x.contiguous(memory_format=mf)) for mf in (torch.contiguous_format, torch.channels_last)]
    dev = copy.deepcopy(net).cuda()
    report = encoders.install_native_geo(dev)
    assert report["geo"] == ([""], {}) and all(not left for _, left in report.values()), report
    N = encoders.NativeTraining
    before = (N.geo_calls, N.strided_calls, N.block_calls, N.hourglass_calls, N.norm_calls)
    runs = [_param_grads(dev, x.cuda(), [g.cuda() for g in gs]) for _ in range(2)]
    after = (N.geo_calls, N.strided_calls, N.block_calls, N.hourglass_calls, N.norm_calls)
    assert tuple(a - b for a, b in zip(after, before)) == (2, 4, 2 * 17, 2, 0)       # the fused calls bypass the rebound norms
    for i in range(2):
        e_ref = max(float((r[i].double() - y64[i]).abs().max()) for r in y32)
        sc.check(f"full width y{i}", runs[0][f"y{i}"].cpu().numpy(), y64[i].numpy(), e_ref)
    for n, v in runs[0].items():
        if v is None:
            assert ".bn4." in n and runs[1][n] is None
            continue
        assert torch.isfinite(v).all(), n
        assert torch.equal(v, runs[1][n]), n
    encoders.uninstall_native_geo(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
