"""The native image encoders (csrc/encoder_kernels.hip, kpn_geo_encode / kpn_tex_encode) on the emulator build, against the
reference's fp64 outputs recorded in tests/golden/case_w_encoders.npz, and the structure checks of keypointnerf_amd/encoders.py.

Bar: the reference's own fp32 run deviates from its fp64 run by e_ref (recorded in the golden per output and per named stage; the stage tensors themselves come from the
fp64 run of the stand-in of tests/encoder_golden.py, which scripts/make_encoder_golden.py pins bit for bit to the reference,
outputs and hooked stages).  The native result
is another fp32 evaluation order, so it has to stay within FACTOR * e_ref + one fp32 ulp of the tensor's maximum, every element.
FACTOR = 4 (the starting value of the issue; measured ratios are in profiles/encoders.md, all below 4)."""
import numpy as np
import pytest
import torch

from keypointnerf_amd import encoders
from tests import encoder_golden as eg
from tests import simt_harness as sh

FACTOR = 4.0


def _bar(e_ref, ref):
    return FACTOR * e_ref + float(np.spacing(np.float32(np.abs(ref).max())))


def _check(name, nat_nhwc, ref, idx, e_ref):
    nat = np.ascontiguousarray(nat_nhwc.transpose(0, 3, 1, 2)).astype(np.float64)
    assert np.isfinite(nat).all(), name
    got = nat if idx is None else nat.reshape(-1)[idx]
    err = float(np.abs(got - ref).max())
    print(f"{name}: max|native - fp64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio = {err / max(e_ref, 1e-30):.2f}")
    assert err <= _bar(e_ref, ref), name
    return err


@pytest.fixture(scope="module")
def G():
    return np.load(eg.GOLDEN)


@pytest.fixture(scope="module")
def nets(G):
    geo, tex = eg.stand_in_geo(int(G["seed_geo"])), eg.stand_in_tex(int(G["seed_tex"]))
    assert np.array_equal(eg.checksums(geo), G["checksum_geo"]) and np.array_equal(eg.checksums(tex), G["checksum_tex"])
    return geo, tex


def _stage_refs(G, tag, net, x, names):
    """fp64 stage tensors of the stand-in (the golden maker asserts its hooked fp32 stages equal the live reference's bit for
    bit) and the reference's e_ref per stage, recorded in the golden"""
    net.double()
    _, s64 = eg.run_with_stages(net, x.double(), names)
    net.float()
    return {k: (s64[k].numpy(), float(G[f"a_{tag}_stage_eref_{k}"])) for k in s64}


def test_geo_parity_by_stage_and_bits(G, nets):
    geo, _ = nets
    L = sh.simt_lib()
    img = eg.case_image(G["a_img_shape"], G["a_img_seed"])
    ds = int(G["a_ds"])
    params, oc, ochd, eps = encoders.geo_params(geo)
    plain = encoders.flat_plain(params).numpy()
    feat, hd, st = eg.emu_geo(L, plain, img.numpy(), ds, oc, ochd, eps)
    for i, nat in enumerate((feat, hd)):
        ref, idx, shape, e_ref = eg.golden_reference(G, "a", "geo", i)
        assert nat.transpose(0, 3, 1, 2).shape == shape
        _check(f"geo output {i}", nat, ref, idx, e_ref)
    refs = _stage_refs(G, "geo", geo, eg.net_input(img, ds), {n: n for n in eg.GEO_STAGE_MODULES})
    assert set(st) == set(refs)
    for k in st:
        _check(f"geo stage {k}", st[k], refs[k][0], None, refs[k][1])
    # the same bits without the stage buffer, and on a second call
    feat2, hd2, _ = eg.emu_geo(L, plain, img.numpy(), ds, oc, ochd, eps, want_stages=False)
    assert np.array_equal(feat, feat2) and np.array_equal(hd, hd2)


def test_tex_parity_by_stage_and_bits(G, nets):
    _, tex = nets
    L = sh.simt_lib()
    img = eg.case_image(G["a_img_shape"], G["a_img_seed"])
    ds = int(G["a_ds"])
    params, cfg, eps = encoders.tex_params(tex)
    plain = encoders.flat_plain(params).numpy()
    feat, st = eg.emu_tex(L, plain, img.numpy(), ds, cfg, eps)
    ref, idx, shape, e_ref = eg.golden_reference(G, "a", "tex", 0)
    assert feat.transpose(0, 3, 1, 2).shape == shape
    _check("tex output", feat, ref, idx, e_ref)
    refs = _stage_refs(G, "tex", tex, eg.net_input(img, ds), eg.TEX_STAGE_MODULES)
    assert set(st) == set(refs)
    for k in st:
        _check(f"tex stage {k}", st[k], refs[k][0], None, refs[k][1])
    feat2, _ = eg.emu_tex(L, plain, img.numpy(), ds, cfg, eps, want_stages=False)
    assert np.array_equal(feat, feat2)


def test_tex_odd_size_and_view_independence(G, nets):
    _, tex = nets
    L = sh.simt_lib()
    params, cfg, eps = encoders.tex_params(tex)
    plain = encoders.flat_plain(params).numpy()
    img = eg.case_image(G["odd_img_shape"], G["odd_img_seed"])
    feat, _ = eg.emu_tex(L, plain, img.numpy(), int(G["odd_ds"]), cfg, eps, want_stages=False)
    ref, idx, shape, e_ref = eg.golden_reference(G, "odd", "tex", 0)
    assert feat.transpose(0, 3, 1, 2).shape == shape
    _check("tex odd size", feat, ref, idx, e_ref)
    # InstanceNorm is per image: view i alone, first or last of three
    three = eg.case_image((3, 3, 20, 12), 5).numpy()
    all3, _ = eg.emu_tex(L, plain, three, 0, cfg, eps, want_stages=False)
    for i in (0, 2):
        one, _ = eg.emu_tex(L, plain, three[i:i + 1], 0, cfg, eps, want_stages=False)
        assert np.array_equal(one[0], all3[i])


def test_geo_view_independence(G, nets):
    geo, _ = nets
    L = sh.simt_lib()
    params, oc, ochd, eps = encoders.geo_params(geo)
    plain = encoders.flat_plain(params).numpy()
    two = eg.case_image((2, 3, 64, 64), 6).numpy()
    f2, h2, _ = eg.emu_geo(L, plain, two, 0, oc, ochd, eps, want_stages=False)
    f1, h1, _ = eg.emu_geo(L, plain, two[1:2], 0, oc, ochd, eps, want_stages=False)
    assert np.array_equal(f1[0], f2[1]) and np.array_equal(h1[0], h2[1])


def test_bad_sizes_are_error_codes():
    L = sh.simt_lib()
    assert L.kpn_geo_encoder_workspace_bytes(1, 64, 96, 0, 64, 8) == 0
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data
    assert L.kpn_geo_encode(p, 1, 64, 96, 0, 64, 8, p, 1e-5, p, p, None, p, 64, None) == -1
    assert b"multiples of 64" in L.kpn_last_error()
    assert L.kpn_tex_encoder_workspace_bytes(1, 64, 64, 0, 48, 3, 4, 2, 8) == 0
    assert L.kpn_tex_encode(p, 1, 64, 64, 0, 64, 3, 4, 0, 8, p, 1e-5, p, None, p, 64, None) == -1


def test_refusals_name_the_cause():
    geo = eg.HGFilterV2()
    geo.hd = True
    with pytest.raises(NotImplementedError, match="hd=True"):
        encoders.geo_params(geo)
    geo = eg.HGFilterV2()
    geo.n_stack = 2
    with pytest.raises(NotImplementedError, match="n_stack=2"):
        encoders.geo_params(geo)
    geo = eg.HGFilterV2()
    geo.bn1 = torch.nn.BatchNorm2d(64)
    with pytest.raises(NotImplementedError, match="batch"):
        encoders.geo_params(geo)
    geo = eg.HGFilterV2()
    geo.extra = torch.nn.Linear(2, 2)
    with pytest.raises(NotImplementedError, match="extra"):
        encoders.geo_params(geo)
    tex = eg.ResBlkEncoder()
    tex.layers[2] = torch.nn.BatchNorm2d(64)
    with pytest.raises(NotImplementedError, match="another norm"):
        encoders.tex_params(tex)
    tex = eg.ResBlkEncoder()
    tex.layers[3] = torch.nn.LeakyReLU()
    with pytest.raises(NotImplementedError, match="layers.3"):
        encoders.tex_params(tex)
    # the shipped configuration is accepted, with the parameter count the library expects
    L = sh.simt_lib()
    p, oc, ochd, _ = encoders.geo_params(eg.HGFilterV2())
    assert sum(t.numel() for t in p) == L.kpn_geo_encoder_plain_floats(oc, ochd)
    p, cfg, _ = encoders.tex_params(eg.ResBlkEncoder())
    assert cfg == (64, 3, 4, 2, 8) and sum(t.numel() for t in p) == L.kpn_tex_encoder_plain_floats(*cfg)
