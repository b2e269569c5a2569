"""The single-operator ResBlkEncoder (kpn_res_encoder_forward / kpn_res_encoder_backward) on the host SIMT emulator: the very kernel
sources, with numpy buffers through the C ABI; and what of torch.ops.kpnerf.res_encoder and install_native_tex(fused=True) needs no GPU.
Cases, reference and bar: tests/res_encoder_cases.py."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import reppad_cases as rc
from tests import res_encoder_cases as ec
from tests import simt_harness as sh
from tests import strided_cases as sc


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = ec.HostArrays()


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_forward_state_and_gradients_against_fp64(L, name):
    ec.check_case(L, B, name)


def test_two_calls_give_equal_bits(L):
    ec.check_two_calls_equal_bits(L, B, "up2")
    ec.check_two_calls_equal_bits(L, B, "ranges")


@pytest.mark.parametrize("name", ["narrow", "up2"])
def test_null_grads_leave_their_buffers_untouched(L, name):
    ec.check_null_grads_leave_buffers_alone(L, B, name)


def test_zero_dy_gives_exact_zeros(L):
    ec.check_zero_dy_gives_zeros(L, B, "narrow")
    ec.check_zero_dy_gives_zeros(L, B, "up2")


def test_bad_descriptors_are_refused_with_a_message(L):
    ec.check_bad_descriptors(L, B)


@pytest.mark.parametrize("name", ["narrow", "ranges"])
def test_an_image_does_not_depend_on_its_batch(L, name):
    ec.check_image_does_not_depend_on_batch(L, B, name)


def test_state_and_workspace_sizes(L):
    for name, c in ec.CASES.items():
        d = ec.desc(c)
        assert L.kpn_res_encoder_state_floats(ctypes.byref(d)) == ec.state_floats(c)
        assert L.kpn_res_encoder_layers(ctypes.byref(d)) == len(ec.layers_of(c))
        # the backward's temporaries: at least the gradient of the widest activation, the stem's output
        assert L.kpn_res_encoder_workspace_bytes(ctypes.byref(d)) >= 4 * c["N"] * c["H"] * c["W"] * c["ngf"]


def test_the_packed_weights_are_the_per_kind_packers_in_layer_order(L):
    """kpn_res_encoder_pack_device against kpn_conv2d_rp_pack_device / kpn_conv2d_s2_pack_device per layer, concatenated"""
    for name in ("up2", "noblocks"):
        c = ec.CASES[name]
        net = ec.reference(name)[0]
        params = ec.Params(L, B, c, net)
        parts = []
        for (kind, cin, cout, k, _, _), m in zip(ec.layers_of(c), ec.convs_of(net)):
            w = m.weight.detach().numpy()
            if kind in ("down", "up"):
                parts.append(sc.pack(L, B, dict(kind=sc.CONV3 if kind == "down" else sc.DECONV3, cin=cin, cout=cout, N=1, H=2, W=2, bias=True), w))
            else:
                rk = rc.STEM7 if kind == "stem" else (rc.CONV3 if k == 3 else rc.CONV7)
                parts.append(rc.pack(L, B, dict(kind=rk, cin=cin, cout=cout, N=1, H=1, W=1, bias=True), w))
        want = np.concatenate([np.asarray(p).reshape(-1) for p in parts])
        assert np.array_equal(np.asarray(params.packed).view(np.uint32), want.view(np.uint32))


def test_pack_is_the_single_layers_packs_in_layer_order(L):
    ec.check_pack_is_the_single_layers_packs(L, B, "narrow")


def test_fake_kernels_give_shapes_in_channels_last_and_there_is_no_cpu_kernel():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name, c in ec.CASES.items():
        cfg = (c["n_down"], c["n_blocks"], c["n_up"], ec.EPS)
        with FakeTensorMode():
            tensors = [torch.empty(s, device="cuda") for l in ec.layers_of(c) for s in (ec.w_shape(l), (l[2],))]
            x = torch.empty(c["N"], ec.IN_CH, c["H"], c["W"], device="cuda")
            y = torch.ops.kpnerf.res_encoder(x, tensors, *cfg)
            assert tuple(y.shape) == tuple(np.array(ec.y_shape(c))[[0, 3, 1, 2]]) and y.is_contiguous(memory_format=torch.channels_last)
            y, state = torch.ops.kpnerf.res_encoder_cl(x, tensors, *cfg)
            assert tuple(state.shape) == (ec.state_floats(c),)
            mask = [i % 2 == 0 for i in range(len(tensors))]
            out = torch.ops.kpnerf.res_encoder_backward(x, tensors, state, y, *cfg, mask)
            assert len(out) == len(tensors)
            for t, m, o in zip(tensors, mask, out):
                assert (o.shape == t.shape) if m else o.numel() == 0
    with pytest.raises((NotImplementedError, RuntimeError)):                     # no CPU kernel
        c = ec.CASES["noblocks"]
        net = ec.reference("noblocks")[0]
        torch.ops.kpnerf.res_encoder(torch.zeros(1, 3, 8, 8), [t for m in ec.convs_of(net) for t in (m.weight, m.bias)], c["n_down"], c["n_blocks"],
                                     c["n_up"], ec.EPS)


def test_install_native_tex_fused_serves_what_the_operator_serves_and_restores_it():
    from keypointnerf_amd import encoders
    from tests import encoder_golden as eg
    net = torch.nn.ModuleDict({"tex": ec.encoder(ec.CASES["narrow"]), "deep": eg.ResBlkEncoder(out_ch=4, ngf=8, n_downsample=1, n_blocks=65, n_upsample=1),
                               "odd": eg.ResBlkEncoder(out_ch=6, ngf=8, n_downsample=1, n_blocks=0, n_upsample=1),
                               "op_only": ec.encoder(ec.CASES["ranges"])})
    twin = copy.deepcopy(net)
    keys = list(net.state_dict().keys())
    bound = {n: m.forward.__func__ for n, m in net.named_modules()}
    report = encoders.install_native_tex(net, fused=True)
    # "odd" is served by neither path; "deep" by the per-layer path only, and stays there with the operator's reason; "op_only" by the
    # operator only (the per-layer operator reads its 7x7 output layer with 4 input channels as a stem)
    assert report["tex"][0] == ["tex", "deep", "op_only"] and list(report["tex"][1]) == ["odd"]
    assert report["fused"][0] == ["tex", "op_only"] and list(report["fused"][1]) == ["deep"] and "n_blocks" in report["fused"][1]["deep"]
    assert all(n.startswith("deep.") for part in ("strided", "norms") for n in report[part][0]) and report["strided"][0] and report["norms"][0]
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == [n for n, _ in twin.named_parameters()]
    assert [n for n, m in net.named_modules() if "_kpnerf_tex_fused" in m.__dict__] == ["tex", "op_only"]
    x = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    N_ = encoders.NativeTraining
    calls = N_.fused_tex_calls, N_.tex_calls
    with torch.no_grad():
        assert torch.equal(net["tex"](x), twin["tex"](x))                        # CPU input: the original forward
    assert (N_.fused_tex_calls, N_.tex_calls) == calls
    # the default keeps today's report: no "fused" entry, and the two installers on every served encoder
    plain = encoders.install_native_tex(net)
    assert sorted(plain) == ["norms", "strided", "tex"] and plain["tex"][0] == ["tex", "deep"] and sorted(plain["tex"][1]) == ["odd", "op_only"]
    assert any(n.startswith("tex.") for n in plain["norms"][0]) and not any("_kpnerf_tex_fused" in m.__dict__ for m in net.modules())
    assert encoders.install_native_tex(net, fused=True)["fused"][0] == ["tex", "op_only"]    # installing again does not stack
    encoders.uninstall_native_tex(net)
    assert not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)
    assert {n: m.forward.__func__ for n, m in net.named_modules()} == bound


@pytest.mark.parametrize("name", ["narrow", "up2", "noblocks"])
def test_forward_has_the_bits_of_the_encoder_computed_layer_by_layer(L, name):
    """y and every kept tensor of kpn_res_encoder_forward against kpn_conv2d_rp_forward / kpn_conv2d_s2_forward /
    kpn_group_norm_forward per layer and one fp32 add per ResBlk - the dataflow of install_native_tex(): same kernels, same launch
    geometry, the same fmaf, one commutative add"""
    ec.check_layer_by_layer_bits(L, B, name)
