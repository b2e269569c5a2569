"""The native image encoders on the GPU against the reference's fp64 outputs of tests/golden/case_w_encoders.npz: all small
cases (every element of the first, the recorded sample of the others), the odd-sized texture case and the sample lattice of
the shipped 3 x 512^2 source set; the exact properties; the wrappers' re-pack.  Bar: FACTOR * e_ref + one fp32 ulp of the
tensor's maximum with FACTOR = 4 (see tests/test_encoders_cpu.py); measured ratios are in profiles/encoders.md."""
import numpy as np
import pytest
import torch

from tests import encoder_golden as eg

pytestmark = pytest.mark.gpu
FACTOR = 4.0


def _check(name, nat_nchw, ref, idx, e_ref):
    nat = nat_nchw.contiguous().double().cpu().numpy()
    assert np.isfinite(nat).all(), name
    got = nat if idx is None else nat.reshape(-1)[idx]
    err = float(np.abs(got - ref).max())
    print(f"{name}: max|native - fp64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio = {err / max(e_ref, 1e-30):.2f}")
    assert err <= FACTOR * e_ref + float(np.spacing(np.float32(np.abs(ref).max()))), name


@pytest.fixture(scope="module")
def G():
    return np.load(eg.GOLDEN)


@pytest.fixture(scope="module")
def native(G):
    from keypointnerf_amd import encoders
    geo, tex = eg.stand_in_geo(int(G["seed_geo"])), eg.stand_in_tex(int(G["seed_tex"]))
    # on the CPU, where the golden's checksums were added up (a device sum has another order)
    assert np.array_equal(eg.checksums(geo), G["checksum_geo"]) and np.array_equal(eg.checksums(tex), G["checksum_tex"])
    return encoders.NativeGeoEncoder(geo.cuda()), encoders.NativeTexEncoder(tex.cuda())


@pytest.mark.parametrize("case", ["a", "b", "c", "odd", "full"])
def test_parity_with_the_reference(G, native, case):
    ng, nt = native
    img = eg.case_image(G[f"{case}_img_shape"], G[f"{case}_img_seed"]).cuda()
    ds = int(G[f"{case}_ds"])
    if case != "odd":
        outs = ng(img, ds=ds)
        for i, o in enumerate(outs):
            ref, idx, shape, e_ref = eg.golden_reference(G, case, "geo", i)
            assert tuple(o.shape) == shape
            _check(f"{case} geo output {i}", o, ref, idx, e_ref)
    o = nt(img, ds=ds)
    ref, idx, shape, e_ref = eg.golden_reference(G, case, "tex", 0)
    assert tuple(o.shape) == shape
    _check(f"{case} tex output", o, ref, idx, e_ref)


def test_stages_against_the_stand_in_fp64(G, native):
    ng, nt = native
    img = eg.case_image(G["a_img_shape"], G["a_img_seed"])
    ds = int(G["a_ds"])
    x = eg.net_input(img, ds)
    for enc, names in ((ng, {n: n for n in eg.GEO_STAGE_MODULES}), (nt, eg.TEX_STAGE_MODULES)):
        cpu = (eg.stand_in_geo(int(G["seed_geo"])) if enc is ng else eg.stand_in_tex(int(G["seed_tex"])))
        tag = "geo" if enc is ng else "tex"
        _, s64 = eg.run_with_stages(cpu.double(), x.double(), names)
        out, st = enc(img.cuda(), ds=ds, want_stages=True)
        plain = enc(img.cuda(), ds=ds)
        for a, b in zip(out if isinstance(out, list) else [out], plain if isinstance(plain, list) else [plain]):
            assert torch.equal(a, b)                       # stage buffer on / off: the same bits
        assert set(st) == set(s64)
        for k in st:
            _check(f"stage {k}", st[k].permute(0, 3, 1, 2), s64[k].numpy(), None, float(G[f"a_{tag}_stage_eref_{k}"]))


def test_exact_properties(native):
    ng, nt = native
    img = eg.case_image((3, 3, 128, 128), 9).cuda()
    g3, t3 = ng(img, ds=1), nt(img, ds=1)
    g3b, t3b = ng(img, ds=1), nt(img, ds=1)
    assert all(torch.equal(a, b) for a, b in zip(g3, g3b)) and torch.equal(t3, t3b)
    for i in (0, 2):                                        # alone, first or last of three
        g1, t1 = ng(img[i:i + 1], ds=1), nt(img[i:i + 1], ds=1)
        assert all(torch.equal(a[0], b[i]) for a, b in zip(g1, g3)) and torch.equal(t1[0], t3[i])


def test_repack_after_an_in_place_change(G):
    from keypointnerf_amd import encoders
    img = eg.case_image((1, 3, 64, 64), 10).cuda()
    geo, tex = eg.stand_in_geo(3).cuda(), eg.stand_in_tex(4).cuda()
    ng, nt = encoders.NativeGeoEncoder(geo), encoders.NativeTexEncoder(tex)
    g0, t0 = [o.clone() for o in ng(img)], nt(img).clone()
    with torch.no_grad():
        geo.l0.bias.add_(0.5)
        tex.layers[1].weight.mul_(1.5)
    g1, t1 = ng(img), nt(img)
    assert not torch.equal(g0[0], g1[0]) and not torch.equal(t0, t1)
    gf, tf = encoders.NativeGeoEncoder(geo)(img), encoders.NativeTexEncoder(tex)(img)
    assert all(torch.equal(a, b) for a, b in zip(g1, gf)) and torch.equal(t1, tf)


def test_python_errors():
    from keypointnerf_amd import encoders
    ng = encoders.NativeGeoEncoder(eg.stand_in_geo(3).cuda())
    with pytest.raises(ValueError, match="multiples of 64"):
        ng(torch.rand(1, 3, 64, 96, device="cuda"))
    with pytest.raises(RuntimeError, match="forward only"):
        ng(torch.rand(1, 3, 64, 64, device="cuda", requires_grad=True))
