"""The single-operator HGFilterV2 on the MI355X: the C ABI on device memory (the same checks as tests/test_hg_filter_cpu.py runs on the
emulator), torch.ops.kpnerf.hg_filter under autograd, and encoders.install_native_geo(fused=True).  Cases, references and bar:
tests/hg_filter_cases.py - `narrow` against the CPU fp64 module, |native - fp64| <= 4 e_ref + 1 ulp(max|fp64|) per tensor; every case
against the per-layer native path, install_native_geo(fused_blocks=True), bit for bit."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import hg_filter_cases as hc
from tests import test_gpu_strided as ts
from tests.parity import Spy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return hc.DeviceArrays()


# ---- the C ABI ----
def test_abi_narrow_outputs_state_and_gradients_against_fp64(L, B):
    hc.check_against_fp64(L, B)


@pytest.mark.parametrize("name", ["narrow", "deep"])
def test_abi_the_operator_has_the_bits_of_the_single_entry_points(L, B, name):
    hc.check_per_layer_bits(L, B, name)


def test_abi_two_calls_give_equal_bits_over_nan_canaries(L, B):
    hc.check_two_calls_equal_bits(L, B, "narrow")
    hc.check_two_calls_equal_bits(L, B, "deep")


def test_abi_an_image_does_not_depend_on_its_batch(L, B):
    hc.check_image_does_not_depend_on_batch(L, B, "deep")


def test_abi_null_grads_leave_their_buffers_untouched_and_the_stem_alone_is_reached(L, B):
    hc.check_null_grads_leave_buffers_alone(L, B, "narrow")


@pytest.mark.parametrize("name", ["narrow", "deep"])
def test_abi_zero_output_gradients_give_exact_zeros(L, B, name):
    hc.check_zero_gradients_give_zeros(L, B, name)


def test_abi_bad_descriptors_are_refused_with_a_message_and_launch_nothing(L, B):
    hc.check_bad_descriptors(L, B)


def test_abi_state_size_is_the_documented_sum(L):
    for c in hc.CASES.values():
        assert L.kpn_hg_filter_state_floats(ctypes.byref(hc.desc(c))) == hc.state_floats(c)


# ---- the per-layer native path: install_native_geo(fused_blocks=True) ----
def _on_device(name):
    net, x, gs = hc.case(name)
    return copy.deepcopy(net).cuda(), x.cuda(), [g.cuda() for g in gs]


def _grads(net, x, gs, outputs=(0, 1)):
    """{"y0", "y1", parameter name: gradient or None} for the output gradients gs of the outputs asked for"""
    ys = net(x)
    params = dict(net.named_parameters())
    grads = torch.autograd.grad([ys[i] for i in outputs], list(params.values()), [gs[i] for i in outputs], allow_unused=True)
    out = {f"y{i}": y.detach() for i, y in enumerate(ys)}
    out.update(dict(zip(params, grads)))
    return out


@functools.lru_cache(maxsize=None)
def _per_layer(name, outputs=(0, 1)):
    """the case under install_native_geo(fused_blocks=True); once per (case, outputs), shared, never modified"""
    from keypointnerf_amd import encoders
    dev, x, gs = _on_device(name)
    report = encoders.install_native_geo(dev, fused_blocks=True)
    assert report["geo"] == ([""], {}) and all(not left for _, left in report.values()), report
    calls = encoders.NativeTraining.geo_calls, encoders.NativeTraining.fused_geo_calls
    got = _grads(dev, x, gs, outputs)
    assert (encoders.NativeTraining.geo_calls, encoders.NativeTraining.fused_geo_calls) == (calls[0] + 1, calls[1])
    encoders.uninstall_native_geo(dev)
    return got


def _op_grads(name, outputs=(0, 1)):
    import keypointnerf_amd.torch_ops  # noqa: F401
    dev, x, gs = _on_device(name)
    names = hc.tensor_names(dev)
    tensors = hc.tensors_of(dev)
    ys = torch.ops.kpnerf.hg_filter(x, tensors, hc.CASES[name]["depth"], hc.EPS)
    grads = torch.autograd.grad([ys[i] for i in outputs], tensors, [gs[i] for i in outputs])
    return ys, dict(zip(names, grads))


def _assert_equal_to_per_layer(name, ys, grads, outputs=(0, 1)):
    want = _per_layer(name, outputs)
    assert torch.equal(ys[0], want["y0"]) and torch.equal(ys[1], want["y1"])
    for n, g in grads.items():
        if want[n] is None:                                          # what the given output gradients do not reach: exact zeros
            assert len(outputs) == 1 and not g.any(), n
        else:
            assert torch.equal(g, want[n]), n
    assert sorted(n for n, g in want.items() if g is not None and n not in ("y0", "y1")) == sorted(n for n in grads if want[n] is not None)


@pytest.mark.parametrize("name", ["narrow", "deep", "full"])
def test_op_has_the_bits_of_the_per_layer_native_path(name):
    """out, x_hd and every parameter gradient of torch.ops.kpnerf.hg_filter equal those of the same network under
    install_native_geo(fused_blocks=True): the recursion, the order of every fan-in sum, the lazily normalised loads and
    k_enc_pool2_bwd_acc, with no ReLU margin needed at any depth"""
    ys, grads = _op_grads(name)
    for y in ys:
        assert y.is_contiguous(memory_format=torch.channels_last)
    _assert_equal_to_per_layer(name, ys, grads)
    assert all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("name", ["narrow", "deep"])
@pytest.mark.parametrize("output", [0, 1])
def test_op_with_one_output_gradient_has_the_bits_of_the_per_layer_path(name, output):
    """d_out only and d_x_hd only: the absent branch contributes nothing"""
    ys, grads = _op_grads(name, (output,))
    _assert_equal_to_per_layer(name, ys, grads, (output,))


# ---- torch.ops.kpnerf.hg_filter ----
bits = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)  # noqa: E731


@pytest.mark.parametrize("name", ["narrow", "deep"])
def test_op_autograd_gives_the_abi_bits(L, B, name):
    out, x_hd, _, grads = hc.run(L, B, name)
    ys, got = _op_grads(name)
    assert np.array_equal(bits(ys[0]), bits(hc.nchw(out))) and np.array_equal(bits(ys[1]), bits(hc.nchw(x_hd)))
    for (n, g), a in zip(got.items(), grads):
        assert np.array_equal(bits(g), bits(a)), n


def test_op_fake_kernels_agree_with_the_real_ones_and_state_has_the_documented_size():
    import keypointnerf_amd.torch_ops  # noqa: F401
    for name in ("narrow", "deep"):
        c = hc.CASES[name]
        dev, x, gs = _on_device(name)
        tensors = [t.detach() for t in hc.tensors_of(dev)]
        checks = ("test_schema", "test_faketensor")
        torch.library.opcheck(torch.ops.kpnerf.hg_filter_cl.default, (x, tensors, c["depth"], hc.EPS), test_utils=checks)
        _, _, state = torch.ops.kpnerf.hg_filter_cl(x, tensors, c["depth"], hc.EPS)
        assert state.numel() == hc.state_floats(c)
        mask = [i % 3 != 1 for i in range(len(tensors))]
        for go, gh in ((gs[0], gs[1]), (None, gs[1]), (gs[0], None)):
            torch.library.opcheck(torch.ops.kpnerf.hg_filter_backward.default, (x, tensors, state, go, gh, c["depth"], hc.EPS, mask), test_utils=checks)


def test_op_keeps_its_input_its_state_and_the_parameters_only():
    """under saved_tensors_hooks: every tensor autograd saves is x, a parameter, or the one `state` buffer, whose size is the documented sum"""
    import keypointnerf_amd.torch_ops  # noqa: F401
    c = hc.CASES["deep"]
    dev, x, _ = _on_device("deep")
    tensors = hc.tensors_of(dev)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        ys = torch.ops.kpnerf.hg_filter(x, tensors, c["depth"], hc.EPS)
    known = {x.data_ptr()} | {t.data_ptr() for t in tensors}
    other = [t for t in saved if t.data_ptr() not in known]
    assert len(other) == 1 and other[0].numel() == hc.state_floats(c) and other[0].dim() == 1, [tuple(t.shape) for t in other]
    assert not {t.data_ptr() for t in saved} & {y.data_ptr() for y in ys}
    assert len(saved) == 2 + len(tensors)


def test_op_pack_cache_is_reused_rebuilt_after_an_in_place_update_and_shared_with_res_encoder():
    """the counts of tests/test_gpu_conv.py for the one packed buffer of the network, which lives in the cache of kpnerf::res_encoder: an
    entry of either operator stays resident beside the other's"""
    from keypointnerf_amd import torch_ops
    from tests import res_encoder_cases as ec
    C = torch_ops._ResPackCache
    torch_ops.res_encoder_cache_clear()
    dev, x, gs = _on_device("narrow")
    tensors = hc.tensors_of(dev)
    run = lambda ts=tensors, xs=x: torch.ops.kpnerf.hg_filter(xs, ts, hc.CASES["narrow"]["depth"], hc.EPS)  # noqa: E731
    h0, m0 = C.hits, C.misses
    y1, y2 = run(), run()
    assert (C.misses - m0, C.hits - h0) == (1, 1) and torch.equal(y1[0], y2[0]) and torch.equal(y1[1], y2[1]) and len(C.entries) == 1
    torch.autograd.grad(y2, tensors, gs)
    assert (C.misses - m0, C.hits - h0) == (1, 2)                       # the backward reads the forward's packed buffer
    # an encoder of kpnerf::res_encoder beside it: its own slot, and both entries hit afterwards
    c = ec.CASES["noblocks"]
    enc, xe, _, _, _ = ec.reference("noblocks")
    enc, xe = copy.deepcopy(enc).cuda(), xe.cuda()
    te = [t for m in ec.convs_of(enc) for t in (m.weight, m.bias)]
    res = lambda: torch.ops.kpnerf.res_encoder(xe, te, c["n_down"], c["n_blocks"], c["n_up"], ec.EPS)  # noqa: E731
    e1 = res()
    assert (C.misses - m0, C.hits - h0) == (2, 2) and len(C.entries) == 2
    y3, e2 = run(), res()
    assert (C.misses - m0, C.hits - h0) == (2, 4) and len(C.entries) == 2
    assert torch.equal(y3[0], y1[0]) and torch.equal(e2, e1)
    with torch.no_grad():
        tensors[-2].mul_(2.0)                                           # what an optimizer step does, to l0's weight
    y4 = run()
    assert (C.misses - m0, C.hits - h0) == (3, 4) and len(C.entries) == 2
    assert not torch.equal(y4[0], y1[0]) and torch.equal(y4[1], y1[1])  # out = l0(...): a stale pack would give y1; x_hd does not read l0
    with torch.inference_mode():
        ti = [t.detach().clone() for t in tensors]
        yi = run(ti, x.clone())
        run(ti, x.clone())
    assert len(C.entries) == 2 and (C.misses - m0, C.hits - h0) == (3, 4)       # inference tensors get no cache
    assert torch.equal(yi[0], y4[0])
    torch_ops.res_encoder_cache_clear()
    assert len(C.entries) == 0


def test_op_raises_on_an_input_that_requires_a_gradient():
    import keypointnerf_amd.torch_ops  # noqa: F401
    dev, x, _ = _on_device("narrow")
    with pytest.raises(RuntimeError, match="no input gradient"):
        torch.ops.kpnerf.hg_filter(x.requires_grad_(True), hc.tensors_of(dev), 1, hc.EPS)
    with pytest.raises(ValueError, match="hg_filter"):
        torch.ops.kpnerf.hg_filter(x.detach(), hc.tensors_of(dev)[:-2], 1, hc.EPS)


# ---- install_native_geo(fused=True) ----
def test_a_fused_network_is_one_operator_forward_and_one_backward():
    """install_native_geo(fused=True) on `narrow`: under a dispatch spy over forward and backward exactly one kpnerf::hg_filter_cl and one
    kpnerf::hg_filter_backward, no per-layer operator, no aten convolution, norm, pool, upsample or ReLU, and no aten::cat or aten::add;
    its results are the operator's, and so the per-layer path's, bits"""
    from keypointnerf_amd import encoders
    dev, x, gs = _on_device("narrow")
    keys, names = list(dev.state_dict().keys()), [n for n, _ in dev.named_parameters()]
    report = encoders.install_native_geo(dev, fused=True)
    assert report["fused"] == ([""], {}) and report["geo"] == ([""], {}), report
    assert all(report[part] == ([], {}) for part in ("strided", "convs", "norms", "blocks", "hourglass")), report
    assert list(dev.state_dict().keys()) == keys and [n for n, _ in dev.named_parameters()] == names
    N_ = encoders.NativeTraining
    calls = N_.fused_geo_calls, N_.geo_calls, N_.fused_block_calls, N_.strided_calls, N_.hourglass_calls, N_.norm_calls
    with Spy() as spy:
        got = _grads(dev, x, gs)
    assert (N_.fused_geo_calls, N_.geo_calls, N_.fused_block_calls, N_.strided_calls, N_.hourglass_calls, N_.norm_calls) == (calls[0] + 1,) + calls[1:]
    bad = sorted({n for n in spy.names if n.startswith(ts.FORBIDDEN + ("aten::cat", "aten::add"))})
    assert not bad, bad
    assert sum(n.startswith("kpnerf::hg_filter_cl") for n in spy.names) == 1
    assert sum(n.startswith("kpnerf::hg_filter_backward") for n in spy.names) == 1
    assert not any(n.startswith("kpnerf::") and not n.startswith("kpnerf::hg_filter") for n in spy.names), spy.names
    want = _per_layer("narrow")
    for n, v in want.items():
        assert (v is None and got[n] is None and ".bn4." in n) or torch.equal(got[n], v), n
    encoders.uninstall_native_geo(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)


def test_the_default_install_is_the_per_layer_path():
    """without ``fused`` everything is as before the keyword: geo_calls counts, fused_geo_calls stays, the report has no "fused" entry"""
    from keypointnerf_amd import encoders
    dev, x, _ = _on_device("narrow")
    report = encoders.install_native_geo(dev)
    assert sorted(report) == ["blocks", "convs", "geo", "hourglass", "norms", "strided"] and "_kpnerf_geo_fused" not in dev.__dict__
    N_ = encoders.NativeTraining
    calls = N_.geo_calls, N_.fused_geo_calls
    with torch.no_grad():
        dev(x)
    assert (N_.geo_calls, N_.fused_geo_calls) == (calls[0] + 1, calls[1])
    # switching between the variants does not stack, and uninstall removes everything
    assert encoders.install_native_geo(dev, fused=True)["fused"] == ([""], {})
    assert "fused" not in encoders.install_native_geo(dev, fused_blocks=True) and "_kpnerf_geo_fused" not in dev.__dict__
    with pytest.raises(ValueError, match="bf16x3"):
        encoders.install_native_geo(dev, fused=True, arith="bf16x3")
    encoders.uninstall_native_geo(dev)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in dev.modules() for k in m.__dict__)


def test_networks_the_operator_does_not_serve_train_on_the_per_layer_path():
    """n_stack = 2, hd = True and one norm with another eps: listed under "fused" with the reason, and trained per layer as today"""
    from keypointnerf_amd import encoders
    net = hc.variants().cuda()
    report = encoders.install_native_geo(net, fused=True)
    assert report["fused"][0] == ["narrow", "deep"] and sorted(report["fused"][1]) == ["eps", "hd", "stacks"]
    x = hc.case("narrow")[1].cuda()
    N_ = encoders.NativeTraining
    for name in ("stacks", "hd", "eps"):
        calls = N_.geo_calls, N_.fused_geo_calls
        ys = net[name](x)
        params = [p for p in net[name].parameters()]
        grads = torch.autograd.grad([ys[0].sum() + ys[1].sum()], params, allow_unused=True)
        assert (N_.geo_calls, N_.fused_geo_calls) == (calls[0] + 1, calls[1]), name
        assert all(g is None or torch.isfinite(g).all() for g in grads) and sum(g is not None for g in grads) > 50
    calls = N_.geo_calls, N_.fused_geo_calls
    net["narrow"](x)
    assert (N_.geo_calls, N_.fused_geo_calls) == (calls[0], calls[1] + 1)
    encoders.uninstall_native_geo(net)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)
