"""The single-operator ResBlkEncoder on the MI355X: the C ABI on device memory (the same checks as tests/test_res_encoder_cpu.py runs on
the emulator), torch.ops.kpnerf.res_encoder under autograd, and encoders.install_native_tex(fused=True).  Cases, reference and bar:
tests/res_encoder_cases.py - every comparison is against the CPU fp64 module, |native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor,
e_ref the larger deviation of two CPU fp32 runs (contiguous and channels_last) from the same fp64 result."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import layer_op_checks as loc
from tests import res_encoder_cases as ec
from tests import test_gpu_reppad as tr
from tests.parity import Spy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return ec.DeviceArrays()


# ---- the C ABI ----
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_abi_forward_state_and_gradients_against_fp64(L, B, name):
    ec.check_case(L, B, name)


@pytest.mark.parametrize("name", ["up2", "ranges"])
def test_abi_two_calls_give_equal_bits(L, B, name):
    ec.check_two_calls_equal_bits(L, B, name)


@pytest.mark.parametrize("name", ["narrow", "up2"])
def test_abi_null_grads_leave_their_buffers_untouched(L, B, name):
    ec.check_null_grads_leave_buffers_alone(L, B, name)


@pytest.mark.parametrize("name", ["narrow", "up2"])
def test_abi_zero_dy_gives_exact_zeros(L, B, name):
    ec.check_zero_dy_gives_zeros(L, B, name)


def test_abi_bad_descriptors_are_refused_with_a_message_and_launch_nothing(L, B):
    ec.check_bad_descriptors(L, B)


@pytest.mark.parametrize("name", ["narrow", "noblocks", "ranges"])
def test_abi_an_image_does_not_depend_on_its_batch(L, B, name):
    ec.check_image_does_not_depend_on_batch(L, B, name)


def test_abi_state_size_follows_the_descriptor(L):
    for c in ec.CASES.values():
        assert L.kpn_res_encoder_state_floats(ctypes.byref(ec.desc(c))) == ec.state_floats(c)


def test_abi_pack_is_the_single_layers_packs_in_layer_order(L, B):
    ec.check_pack_is_the_single_layers_packs(L, B, "narrow")


# ---- torch.ops.kpnerf.res_encoder ----
bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)  # noqa: E731


def _tensors(net):
    return [t for m in ec.convs_of(net) for t in (m.weight, m.bias)]


def _cfg(c):
    return c["n_down"], c["n_blocks"], c["n_up"], ec.EPS


def _case_on_device(name):
    net, x, g, _, _ = ec.reference(name)
    return copy.deepcopy(net).cuda(), x.cuda(), g.cuda()


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_op_autograd_gives_the_abi_bits(L, B, name):
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = ec.CASES[name]
    y_abi, _, out = ec.run(L, B, name)
    dev, x, g = _case_on_device(name)
    tensors = _tensors(dev)
    y = torch.ops.kpnerf.res_encoder(x, tensors, *_cfg(c))
    grads = torch.autograd.grad(y, tensors, g)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bits(y), bits(ec.nchw(y_abi)))
    for key, got in zip(ec.all_grads(c), grads):
        assert np.array_equal(bits(got), bits(out[key])), key


def test_op_partial_gradients_and_memory_formats():
    """asking for two gradients only gives those two, unchanged; a channels_last x gives the bits of the contiguous one"""
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = ec.CASES["narrow"]
    dev, x, g = _case_on_device("narrow")
    tensors = _tensors(dev)
    y0 = torch.ops.kpnerf.res_encoder(x, tensors, *_cfg(c))
    full = torch.autograd.grad(y0, tensors, g)
    for p in dev.parameters():
        p.requires_grad_(False)
    convs = ec.convs_of(dev)
    convs[3].weight.requires_grad_(True)            # the first convolution of the first ResBlk
    convs[-1].bias.requires_grad_(True)
    y = torch.ops.kpnerf.res_encoder(x.contiguous(memory_format=torch.channels_last), tensors, *_cfg(c))
    assert torch.equal(y, y0)
    got = torch.autograd.grad(y, [convs[3].weight, convs[-1].bias], g)
    assert torch.equal(got[0], full[2 * 3]) and torch.equal(got[1], full[-1])
    y = torch.ops.kpnerf.res_encoder(x, [t.detach() for t in tensors], *_cfg(c))
    assert not y.requires_grad and torch.equal(y, y0)


def test_op_pack_cache_is_reused_and_rebuilt_after_an_in_place_update():
    """the counts of tests/test_gpu_conv.py for the one packed buffer of an encoder: keyed on every weight, not on the first alone"""
    from keypointnerf_amd import torch_ops
    C = torch_ops._ResPackCache
    torch_ops.res_encoder_cache_clear()
    c = ec.CASES["noblocks"]
    dev, x, g = _case_on_device("noblocks")
    tensors = _tensors(dev)
    h0, m0 = C.hits, C.misses
    y1 = torch.ops.kpnerf.res_encoder(x, tensors, *_cfg(c))
    y2 = torch.ops.kpnerf.res_encoder(x, tensors, *_cfg(c))
    assert (C.misses - m0, C.hits - h0) == (1, 1) and torch.equal(y1, y2) and len(C.entries) == 1
    torch.autograd.grad(y2, tensors, g)
    assert (C.misses - m0, C.hits - h0) == (1, 2)                       # the backward reads the forward's packed buffer
    with torch.no_grad():
        tensors[-2].mul_(2.0)                                           # what an optimizer step does, to the output layer's weight
    y3 = torch.ops.kpnerf.res_encoder(x, tensors, *_cfg(c))
    assert (C.misses - m0, C.hits - h0) == (2, 2) and len(C.entries) == 1
    assert not torch.equal(y3, y1)                                      # no norm behind the output layer: a stale pack would give y1
    with torch.inference_mode():
        ti = [t.detach().clone() for t in tensors]
        yi = torch.ops.kpnerf.res_encoder(x.clone(), ti, *_cfg(c))
        torch.ops.kpnerf.res_encoder(x.clone(), ti, *_cfg(c))
    assert len(C.entries) == 1 and (C.misses - m0, C.hits - h0) == (2, 2)       # inference tensors get no cache
    assert torch.equal(yi, y3)
    torch_ops.res_encoder_cache_clear()
    assert len(C.entries) == 0


def test_op_raises_on_an_input_that_requires_a_gradient():
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = ec.CASES["noblocks"]
    dev, x, _ = _case_on_device("noblocks")
    with pytest.raises(RuntimeError, match="no input gradient"):
        torch.ops.kpnerf.res_encoder(x.requires_grad_(True), _tensors(dev), *_cfg(c))
    with pytest.raises(ValueError, match="convolutions"):
        torch.ops.kpnerf.res_encoder(x.detach(), _tensors(dev)[:-2], *_cfg(c))


def test_op_fake_kernels_agree_with_the_real_ones():
    import keypointnerf_amd.torch_ops  # noqa: F401
    for name in ("up2", "noblocks"):
        c = ec.CASES[name]
        dev, x, g = _case_on_device(name)
        tensors = [t.detach() for t in _tensors(dev)]
        checks = ("test_schema", "test_faketensor")
        torch.library.opcheck(torch.ops.kpnerf.res_encoder_cl.default, (x, tensors, *_cfg(c)), test_utils=checks)
        _, state = torch.ops.kpnerf.res_encoder_cl(x, tensors, *_cfg(c))
        assert state.numel() == ec.state_floats(c)
        mask = [i % 3 != 1 for i in range(len(tensors))]
        torch.library.opcheck(torch.ops.kpnerf.res_encoder_backward.default, (x, tensors, state, g, *_cfg(c), mask), test_utils=checks)


# ---- install_native_tex(fused=True) ----
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_fused_forward_has_the_bits_of_the_per_layer_native_path(L, B, name):
    """Same kernels, same launch geometry, the same fmaf, one commutative fp32 add per ResBlk: y of the fused operator equals y of the
    same encoder under install_native_tex(), bit for bit.  install_native_tex() leaves the `up2` and `ranges` encoders alone (their 7x7
    output layer has 4 input channels, which torch.ops.kpnerf.conv2d_replicate reads as a stem), so there the per-layer path is run as
    the calls it would make: the single layers of the C ABI on the device (kpn_conv2d_rp_forward with KPN_RP_CONV7 for that layer)."""
    from keypointnerf_amd import encoders
    dev, x, _ = _case_on_device(name)
    N_ = encoders.NativeTraining
    with torch.no_grad():
        report = encoders.install_native_tex(dev)
        if ec.layers_of(ec.CASES[name])[-1][1] <= 4:
            assert name in ("up2", "ranges")
            assert report["tex"][0] == [] and "as the stem" in report["tex"][1][""]
            plain = torch.from_numpy(ec.nchw(ec.check_layer_by_layer_bits(L, B, name))).cuda()
        else:
            assert report["tex"] == ([""], {})
            calls = N_.tex_calls, N_.fused_tex_calls
            plain = dev(x)
            assert (N_.tex_calls, N_.fused_tex_calls) == (calls[0] + 1, calls[1])
        calls = N_.tex_calls, N_.fused_tex_calls
        report = encoders.install_native_tex(dev, fused=True)
        assert report["tex"] == ([""], {}) and report["fused"] == ([""], {}) and report["strided"] == ([], {}) and report["norms"] == ([], {})
        fused = dev(x)
        assert (N_.tex_calls, N_.fused_tex_calls) == (calls[0], calls[1] + 1)
    encoders.uninstall_native_tex(dev)
    assert torch.equal(plain, fused)


@pytest.mark.parametrize("name", ["narrow", "up2"])
def test_a_fused_encoder_is_one_operator_forward_and_one_backward_and_meets_the_bar(name):
    """install_native_tex(fused=True) against the CPU fp64 module: the output and every parameter gradient within the bar; under a
    dispatch spy over forward and backward exactly one kpnerf::res_encoder_cl and one kpnerf::res_encoder_backward, no per-layer
    operator, no aten convolution, pad, norm or ReLU, and no aten::add on an activation-sized tensor"""
    from keypointnerf_amd import encoders
    c = ec.CASES[name]
    net, x, g, r64, e_ref = ec.reference(name)
    dev = copy.deepcopy(net).cuda()
    keys, names = list(dev.state_dict().keys()), [n for n, _ in dev.named_parameters()]
    report = encoders.install_native_tex(dev, fused=True)
    assert report["fused"] == ([""], {}), report
    assert list(dev.state_dict().keys()) == keys and [n for n, _ in dev.named_parameters()] == names
    N_ = encoders.NativeTraining
    calls = N_.fused_tex_calls, N_.tex_calls, N_.strided_calls, N_.norm_calls
    with Spy() as spy:
        got = loc.param_grads(dev, x.cuda(), g.cuda())
    assert (N_.fused_tex_calls, N_.tex_calls, N_.strided_calls, N_.norm_calls) == (calls[0] + 1,) + calls[1:]
    bad = sorted({n for n in spy.names if n.startswith(tr.FORBIDDEN)})
    assert not bad, bad
    assert sum(n.startswith("kpnerf::res_encoder_cl") for n in spy.names) == 1
    assert sum(n.startswith("kpnerf::res_encoder_backward") for n in spy.names) == 1
    assert not any(n.startswith(("kpnerf::conv2d", "kpnerf::conv_transpose2d", "kpnerf::group_norm")) for n in spy.names), spy.names
    smallest = min(c["N"] * h * w * co for _, _, co, _, h, w in ec.layers_of(c))
    assert not [n for n in spy.adds if n >= smallest], (spy.adds, smallest)
    for n in ["y"] + names:
        ec.check(f"installed fused {name} {n}", got[n].cpu().numpy(), r64[n], e_ref[n])
    encoders.uninstall_native_tex(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)


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


def test_a_fused_encoder_saves_its_input_and_its_state_and_nothing_else_of_that_size(L):
    """The bound is a condition, not a measurement: the fused operator saves x, `state` and the parameters, so the saved tensors with at
    least as many elements as the smallest activation total at most numel(x) + kpn_res_encoder_state_floats, and state_floats is
    sum numel(c_i) + sum numel(a_k) + 4 N sum C_norm from the descriptor.  Every parameter of the case is smaller than its smallest
    activation.  The per-layer path's total is printed beside it, not asserted."""
    from keypointnerf_amd import encoders
    c = ec.CASES["ranges"]
    dev, x, _ = _case_on_device("ranges")
    smallest = min(c["N"] * h * w * co for _, _, co, _, h, w in ec.layers_of(c))
    assert max(p.numel() for p in dev.parameters()) < smallest
    state = L.kpn_res_encoder_state_floats(ctypes.byref(ec.desc(c)))
    assert state == ec.state_floats(c)
    served = encoders.install_native_tex(dev)["tex"][0]
    per_layer = _saved_floats(dev, x, smallest)
    encoders.install_native_tex(dev, fused=True)
    fused = _saved_floats(dev, x, smallest)
    encoders.uninstall_native_tex(dev)
    # (install_native_tex() leaves this encoder alone - its output layer has 4 input channels - so its figure is the untouched module's)
    print(f"[res encoder saved activations] fused {fused} floats; install_native_tex() ({'per-layer' if served else 'left on torch'}) "
          f"{per_layer} floats; bound numel(x) + state = {x.numel() + state}")
    assert 0 < fused <= x.numel() + state


def test_the_default_install_is_the_per_layer_path_and_uninstall_leaves_nothing():
    """install_native_tex(dev) without ``fused`` still makes the per-layer calls: one conv2d_rp_forward per replication-padded
    convolution and one group_norm_forward per norm; fused_tex_calls stays where it was.  An encoder the operator does not serve stays on
    the per-layer path with its reason."""
    from keypointnerf_amd import encoders, ops
    c = ec.CASES["narrow"]
    dev, x, _ = _case_on_device("narrow")
    report = encoders.install_native_tex(dev)
    assert sorted(report) == ["norms", "strided", "tex"] and report["tex"] == ([""], {})
    assert "_kpnerf_tex_fused" not in dev.__dict__
    seen = {"norm": 0, "rp": 0}
    real_n, real_c = ops.group_norm_forward, ops.conv2d_rp_forward
    ops.group_norm_forward = lambda *a, **kw: (seen.__setitem__("norm", seen["norm"] + 1), real_n(*a, **kw))[1]
    ops.conv2d_rp_forward = lambda *a, **kw: (seen.__setitem__("rp", seen["rp"] + 1), real_c(*a, **kw))[1]
    N_ = encoders.NativeTraining
    calls = N_.tex_calls, N_.fused_tex_calls
    try:
        with torch.no_grad():
            dev(x)
    finally:
        ops.group_norm_forward, ops.conv2d_rp_forward = real_n, real_c
    assert (N_.tex_calls, N_.fused_tex_calls) == (calls[0] + 1, calls[1])
    assert seen == {"norm": 1 + c["n_down"] + 2 * c["n_blocks"] + c["n_up"], "rp": 2 + 2 * c["n_blocks"]}
    # switching between the variants does not stack, and uninstall removes everything
    assert encoders.install_native_tex(dev, fused=True)["fused"] == ([""], {})
    assert encoders.install_native_tex(dev)["tex"] == ([""], {}) and "_kpnerf_tex_fused" not in dev.__dict__
    assert encoders.install_native_tex(dev, fused=True)["fused"] == ([""], {})
    encoders.uninstall_native_tex(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)
