"""install_encoders on the reference's own KeypointNeRF class, on the CPU with the emulator build behind the ops (skips without
the reference source tree), the fake kernels of torch.ops.kpnerf.geo_encode / tex_encode, and the remaining exact properties
of the geometry encoder on the emulator."""
import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import encoder_golden as eg

needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference source tree (KPNERF_REFERENCE_ROOT)")


@pytest.fixture
def emulated(monkeypatch):
    from keypointnerf_amd import lib as kl, ops, torch_ops
    from tests.simt_harness import simt_lib
    L = simt_lib()
    monkeypatch.setattr(kl, "get_library", lambda: L)
    monkeypatch.setattr(ops, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    with torch.library._scoped_library("kpnerf", "FRAGMENT") as frag:
        for name in ("geo_encode", "tex_encode"):
            frag.impl(name, getattr(torch_ops, name)._init_fn, "CPU")
        yield L


@needs_reference
def test_install_encoders_on_the_live_class(emulated):
    from keypointnerf_amd import encoders
    net = ref_shim.build_reference_net(seed=0)
    eg.perturb(net.geo_encoder, 41)
    eg.perturb(net.tex_encoder, 42)
    img = eg.case_image((1, 1, 3, 128, 128), 43)
    net.eval()
    with torch.no_grad():
        # (the reference's attach_im_feat builds its dictionary and does not return it, src/model.py:641-651)
        ref = {"feat_geo": net.attach_geo_feat(img, return_val=True), "feat_tex": net.attach_tex_feat(img, return_val=True)}
    bound = (net.attach_geo_feat.__func__, net.attach_tex_feat.__func__)
    encoders.install_encoders(net, tex=True)
    g0, t0 = encoders.NativeGeoEncoder.calls, encoders.NativeTexEncoder.calls
    with torch.no_grad():
        net.attach_im_feat(img)
    assert (encoders.NativeGeoEncoder.calls, encoders.NativeTexEncoder.calls) == (g0 + 1, t0 + 1)
    assert torch.equal(net.im, img)
    for name, a, b in (("geo", net.feat_geo[0], ref["feat_geo"][0]), ("hd", net.feat_geo[1], ref["feat_geo"][1]), ("tex", net.feat_tex, ref["feat_tex"])):
        assert a.shape == b.shape and a.dtype == b.dtype
        e = float((a - b).abs().max())
        print(f"{name}: max|native - module fp32| = {e:.3e} (max {float(b.abs().max()):.2f})")
        assert e <= 1e-4
    net.train()
    out = {"feat_geo": net.attach_geo_feat(img, return_val=True), "feat_tex": net.attach_tex_feat(img, return_val=True)}
    assert (encoders.NativeGeoEncoder.calls, encoders.NativeTexEncoder.calls) == (g0 + 1, t0 + 1)
    (out["feat_geo"][0].sum() + out["feat_tex"].sum()).backward()
    assert net.geo_encoder.conv1.weight.grad is not None and net.tex_encoder.layers[1].weight.grad is not None
    encoders.uninstall_encoders(net)
    assert "attach_geo_feat" not in net.__dict__ and "attach_tex_feat" not in net.__dict__
    assert (net.attach_geo_feat.__func__, net.attach_tex_feat.__func__) == bound


def test_torch_ops_are_registered_with_fake_kernels():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        img, p = torch.empty(3, 3, 512, 512, device="cuda"), torch.empty(16, device="cuda")
        f, fhd = torch.ops.kpnerf.geo_encode(img, p, [1, 64, 8], 1e-5)
        assert tuple(f.shape) == (3, 64, 64, 64) and tuple(fhd.shape) == (3, 256, 256, 8)
        t = torch.ops.kpnerf.tex_encode(torch.empty(1, 3, 50, 38, device="cuda"), p, [0, 64, 3, 4, 2, 8], 1e-5)
        assert tuple(t.shape) == (1, 28, 20, 8)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.kpnerf.geo_encode(torch.zeros(1, 3, 64, 64), torch.zeros(16), [0, 64, 8], 1e-5)


def test_geo_alone_first_and_last_of_three_and_two_calls():
    from keypointnerf_amd import encoders
    from tests import simt_harness as sh
    L = sh.simt_lib()
    params, oc, ochd, eps = encoders.geo_params(eg.stand_in_geo(5))
    plain = encoders.flat_plain(params).numpy()
    three = eg.case_image((3, 3, 64, 64), 6).numpy()
    f3, h3, _ = eg.emu_geo(L, plain, three, 0, oc, ochd, eps, want_stages=False)
    for i in (0, 2):
        f1, h1, _ = eg.emu_geo(L, plain, three[i:i + 1], 0, oc, ochd, eps, want_stages=False)
        assert np.array_equal(f1[0], f3[i]) and np.array_equal(h1[0], h3[i])
    f1b, h1b, _ = eg.emu_geo(L, plain, three[2:3], 0, oc, ochd, eps, want_stages=False)
    assert np.array_equal(f1, f1b) and np.array_equal(h1, h1b)
    assert L.kpn_geo_encoder_workspace_bytes(1, 256, 256, 2, 64, 8) == 0        # two average pools: refused
