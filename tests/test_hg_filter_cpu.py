"""The single-operator HGFilterV2 (kpn_hg_filter_forward / kpn_hg_filter_backward) on the host SIMT emulator: the very kernel sources, with
numpy buffers through the C ABI; and what of torch.ops.kpnerf.hg_filter and install_native_geo(fused=True) needs no GPU.  Cases, references
and bar: tests/hg_filter_cases.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import hg_filter_cases as hc
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = hc.HostArrays()


def test_narrow_outputs_state_and_gradients_against_fp64(L):
    hc.check_against_fp64(L, B)


@pytest.mark.parametrize("name", ["narrow", "deep"])
def test_the_operator_has_the_bits_of_the_per_layer_path(L, name):
    hc.check_per_layer_bits(L, B, name)


@pytest.mark.parametrize("branch", ["d_out", "d_x_hd"])
def test_one_output_gradient_alone_has_the_bits_of_the_per_layer_path(L, branch):
    hc.check_per_layer_bits(L, B, "narrow", **{"d_x_hd" if branch == "d_out" else "d_out": None})


def test_two_calls_give_equal_bits_over_nan_canaries(L):
    hc.check_two_calls_equal_bits(L, B, "narrow")


def test_an_image_does_not_depend_on_its_batch(L):
    hc.check_image_does_not_depend_on_batch(L, B, "deep")


def test_null_grads_leave_their_buffers_untouched_and_the_stem_alone_is_reached(L):
    hc.check_null_grads_leave_buffers_alone(L, B, "narrow")


def test_zero_output_gradients_give_exact_zeros(L):
    hc.check_zero_gradients_give_zeros(L, B, "narrow")


def test_bad_descriptors_are_refused_with_a_message(L):
    hc.check_bad_descriptors(L, B)


def test_state_size_is_the_documented_sum(L):
    from keypointnerf_amd import ops
    for name, c in hc.CASES.items():
        d = hc.desc(c)
        assert L.kpn_hg_filter_state_floats(ctypes.byref(d)) == hc.state_floats(c) == ops.hg_filter_state_floats(c["N"], c["H"], c["W"], hc.cfg_of(c))
        assert L.kpn_hg_filter_tensors(ctypes.byref(d)) == len(ops.hg_filter_shapes(hc.cfg_of(c)))
        # the backward's temporaries: at least the gradient of the widest activation, the unpack1.conv output
        assert L.kpn_hg_filter_workspace_bytes(ctypes.byref(d)) >= 4 * c["N"] * c["H"] * c["W"] * c["c_hd"]
    net = hc.case("deep")[0]
    assert [tuple(t.shape) for t in hc.tensors_of(net)] == ops.hg_filter_shapes(hc.cfg_of(hc.CASES["deep"]))


def test_fake_kernels_give_shapes_in_channels_last_and_there_is_no_cpu_kernel():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from keypointnerf_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("narrow", "deep"):
        c = hc.CASES[name]
        cfg = hc.cfg_of(c)
        with FakeTensorMode():
            tensors = [torch.empty(s, device="cuda") for s in ops.hg_filter_shapes(cfg)]
            x = torch.empty(c["N"], 3, c["H"], c["W"], device="cuda")
            out, x_hd = torch.ops.kpnerf.hg_filter(x, tensors, c["depth"], hc.EPS)
            so, sh_ = hc.out_shapes(c)
            assert tuple(out.shape) == tuple(np.array(so)[[0, 3, 1, 2]]) and out.is_contiguous(memory_format=torch.channels_last)
            assert tuple(x_hd.shape) == tuple(np.array(sh_)[[0, 3, 1, 2]]) and x_hd.is_contiguous(memory_format=torch.channels_last)
            out, x_hd, state = torch.ops.kpnerf.hg_filter_cl(x, tensors, c["depth"], hc.EPS)
            assert tuple(state.shape) == (hc.state_floats(c),)
            mask = [i % 2 == 0 for i in range(len(tensors))]
            for go, gh in ((out, x_hd), (None, x_hd), (out, None)):
                got = torch.ops.kpnerf.hg_filter_backward(x, tensors, state, go, gh, c["depth"], hc.EPS, mask)
                assert len(got) == len(tensors)
                for t, m, o in zip(tensors, mask, got):
                    assert (o.shape == t.shape) if m else o.numel() == 0
    with pytest.raises((NotImplementedError, RuntimeError)):                     # no CPU kernel
        net, x, _ = hc.case("narrow")
        torch.ops.kpnerf.hg_filter(x, hc.tensors_of(net), 1, hc.EPS)
    with pytest.raises(ValueError, match="hg_filter"):
        with FakeTensorMode():
            tensors = [torch.empty(s, device="cuda") for s in ops.hg_filter_shapes(hc.cfg_of(hc.CASES["deep"]))]
            torch.ops.kpnerf.hg_filter_cl(torch.empty(1, 3, 16, 16, device="cuda"), tensors[:-2], 2, hc.EPS)


def test_install_native_geo_fused_serves_what_the_operator_serves_and_restores_it():
    from keypointnerf_amd import encoders
    net = hc.variants()
    twin = copy.deepcopy(net)
    keys = list(net.state_dict().keys())
    bound = {n: m.forward.__func__ for n, m in net.named_modules()}
    report = encoders.install_native_geo(net, fused=True)
    assert report["geo"] == (["stacks", "hd", "eps", "narrow", "deep"], {})
    assert report["fused"][0] == ["narrow", "deep"] and list(report["fused"][1]) == ["stacks", "hd", "eps"], report["fused"]
    why = report["fused"][1]
    assert "n_stack" in why["stacks"] and "hd" in why["hd"] and "eps" in why["eps"]
    # those the operator does not serve get the per-layer installers exactly as without the keyword; those it serves get none
    for part in ("strided", "convs", "norms", "blocks", "hourglass"):
        assert report[part][0] and all(n.split(".")[0] in ("stacks", "hd", "eps") for n in report[part][0]), part
    assert [n for n, m in net.named_modules() if "_kpnerf_geo_fused" in m.__dict__] == ["narrow", "deep"]
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == [n for n, _ in twin.named_parameters()]
    N_ = encoders.NativeTraining
    calls = N_.fused_geo_calls, N_.geo_calls
    x = hc.case("narrow")[1]
    with torch.no_grad():
        for a, b in zip(net["narrow"](x), twin["narrow"](x)):                   # CPU input: the original forward
            assert torch.equal(a, b)
    assert (N_.fused_geo_calls, N_.geo_calls) == calls
    # the default keeps today's report: no "fused" entry, and the five installers on every served network
    plain = encoders.install_native_geo(net)
    assert sorted(plain) == ["blocks", "convs", "geo", "hourglass", "norms", "strided"]
    assert any(n.startswith("narrow.") for n in plain["blocks"][0]) and not any("_kpnerf_geo_fused" in m.__dict__ for m in net.modules())
    assert encoders.install_native_geo(net, fused=True)["fused"][0] == ["narrow", "deep"]        # installing again does not stack
    with pytest.raises(ValueError, match="bf16x3"):
        encoders.install_native_geo(net, fused=True, arith="bf16x3")
    encoders.uninstall_native_geo(net)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)
    assert {n: m.forward.__func__ for n, m in net.named_modules()} == bound
