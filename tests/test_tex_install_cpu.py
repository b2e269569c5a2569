"""encoders.install_native_tex on CPU modules: what it serves and leaves, that CPU input reaches the original forward bit for bit, and
that uninstall restores everything.  The native path itself is tests/test_gpu_reppad.py's."""
import copy

import torch
import torch.nn as nn

from tests import encoder_golden as eg


def _narrow(**over):
    a = dict(out_ch=4, ngf=4, n_downsample=2, n_blocks=2, n_upsample=1)
    a.update(over)
    return eg.seeded(eg.ResBlkEncoder(**a), 2).train()


def _clean(net):
    return not any(k.startswith("_kpnerf") or k == "forward" for m in net.modules() for k in m.__dict__)


def test_install_serves_the_encoder_and_cpu_input_reaches_the_original_forward():
    from keypointnerf_amd import encoders
    net, twin = _narrow(), _narrow()
    keys, names = list(net.state_dict().keys()), [n for n, _ in net.named_parameters()]
    report = encoders.install_native_tex(net)
    assert report["tex"] == ([""], {}) and all(not left for _, left in report.values()), report
    assert sorted(report["strided"][0]) == sorted(n for n, m in net.named_modules()
                                                  if type(m) is nn.ConvTranspose2d or (type(m) is nn.Conv2d and m.stride == (2, 2)))
    assert len(report["strided"][0]) == 3
    assert sorted(report["norms"][0]) == sorted(n for n, m in net.named_modules() if type(m) is nn.InstanceNorm2d)
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_parameters()] == names
    assert "forward" in net.__dict__
    x = torch.randn(2, 3, 12, 8, generator=torch.Generator().manual_seed(72))
    calls = encoders.NativeTraining.tex_calls
    assert torch.equal(net(x), twin(x))                                    # CPU input: the module's own forward, bit for bit
    assert encoders.NativeTraining.tex_calls == calls
    again = encoders.install_native_tex(net)                               # installing twice equals installing once
    assert again == report
    assert net.__dict__["_kpnerf_tex_saved"] is None
    encoders.uninstall_native_tex(net)
    assert _clean(net) and torch.equal(net(x), twin(x))
    assert list(net.state_dict().keys()) == keys


def test_an_encoder_under_a_parent_is_found_and_named():
    from keypointnerf_amd import encoders
    holder = nn.Module()
    holder.image_filter_tex = _narrow()
    holder.other = nn.Conv2d(4, 4, 3, stride=2, padding=1)                # not under the encoder: not touched
    report = encoders.install_native_tex(holder)
    assert report["tex"] == (["image_filter_tex"], {})
    assert all(n.startswith("image_filter_tex.") for part in ("strided", "norms") for n in report[part][0])
    assert "forward" not in holder.other.__dict__
    encoders.uninstall_native_tex(holder)
    assert _clean(holder)


def test_ineligible_encoders_are_left_alone_with_a_reason_that_names_the_layer():
    from keypointnerf_amd import encoders
    batch = _narrow()
    for i, m in enumerate(batch.layers):
        if type(m) is nn.InstanceNorm2d:
            batch.layers[i] = nn.BatchNorm2d(m.num_features)                # norm="batch"
    no_up = _narrow(n_upsample=0)
    six = _narrow(out_ch=6)
    wide_stem = _narrow(n_downsample=1, n_upsample=1)                     # 4 channels in front of the output layer: the operator's stem rule
    for net, layer, word in ((batch, "layers.2", "BatchNorm2d"), (no_up, f"layers.{len(no_up.layers) - 1}", "n_upsample=0"),
                             (six, f"layers.{len(six.layers) - 1}", "out_ch 6"), (wide_stem, f"layers.{len(wide_stem.layers) - 1}", "stem")):
        twin = copy.deepcopy(net)
        report = encoders.install_native_tex(net)
        assert report["tex"][0] == [] and list(report["tex"][1]) == [""], report
        why = report["tex"][1][""]
        assert layer in why and word in why, why
        assert report["strided"] == ([], {}) and report["norms"] == ([], {})
        assert _clean(net)
        x = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(3))
        assert torch.equal(net(x), twin(x))


def test_the_op_has_no_cpu_kernel_and_names_a_bad_weight():
    import pytest
    import keypointnerf_amd.torch_ops  # noqa: F401
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.kpnerf.conv2d_replicate_cl(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3), None)
    with pytest.raises(ValueError, match="3x3 under ReplicationPad2d"):
        torch.ops.kpnerf.conv2d_replicate(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 5, 5), None)
