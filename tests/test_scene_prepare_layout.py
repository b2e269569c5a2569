"""kpn_scene_prepare read back through kpn_scene_layout: every prepared map is the channels-last copy of its input, bit for bit,
and flags[0] is the maximum |value| of the images and the maps as an int bit pattern (a NaN ranks above +inf and survives).  The same
cases on the emulator build (numpy buffers) and, under the gpu marker, on the product library (device tensors).

Shapes: no map size is a multiple of a copy kernel's tile (64 pixels of geo0, 512 of geo1 / tex, 1,024 of the image), a 33 x 65 geo0
spreads every view over 34 tiles, and one case has maps whose h * w is a multiple of 4 - the float4 loads - once 16-byte aligned
and once a float off."""
import ctypes

import numpy as np
import pytest
import torch

from keypointnerf_amd import lib as kl
from tests.parity import DeviceArrays, HostArrays, bits

#        V, image,    geo0,     geo1,     tex
CASES = {"odd": (2, (19, 23), (9, 11), (7, 5), (10, 13)),
         "straddle": (3, (19, 23), (33, 65), (7, 5), (10, 13)),
         "vec": (2, (36, 32), (8, 10), (24, 24), (4, 6))}          # 1,152 pixels, 80, 576 and 24: two tiles each but tex, all % 4 == 0
BIG_BITS = int(np.float32(7e4).view(np.uint32))
BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


def _env(backend):
    if backend == "emu":
        from tests import simt_harness as sh
        return sh.simt_lib(), HostArrays()
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return kl.get_library(), DeviceArrays()


def inputs(case, seed=0):
    V, (H, W), g0, g1, tx = CASES[case]
    rng = np.random.default_rng(100 + seed + 10 * sorted(CASES).index(case))
    a = {"img": rng.random((V, 3, H, W), dtype=np.float32),
         "geo0": rng.standard_normal((V, 64, *g0), dtype=np.float32) * 3.0,
         "geo1": rng.standard_normal((V, 8, *g1), dtype=np.float32),
         "tex": rng.standard_normal((V, 8, *tx), dtype=np.float32),
         "fg_mask": (rng.random((V, H, W)) < 0.6).astype(np.uint8),
         "KRT": (np.eye(4, dtype=np.float32) + 0.2 * rng.standard_normal((V, 4, 4)).astype(np.float32)),
         "extrin": (np.eye(4, dtype=np.float32) + 0.2 * rng.standard_normal((V, 4, 4)).astype(np.float32)),
         "kpt3d": rng.standard_normal((24, 3)).astype(np.float32)}
    return a


def put(B, a, off=0):
    """the array on the build's side; off = 1: in a buffer that starts one element before it (a float map is then 4 bytes off 16-byte
    alignment)"""
    flat = np.concatenate([np.zeros(off, a.dtype), np.ascontiguousarray(a).reshape(-1)])
    buf = flat.copy() if isinstance(B, HostArrays) else torch.from_numpy(flat).cuda()
    return buf[off:]


def prepare(L, B, a, disable_fg_mask=False, off=0, ws=None):
    """-> (workspace as numpy floats, offsets, the workspace buffer)"""
    V, _, H, W = a["img"].shape
    d = kl.SceneDesc()
    d.n_views, d.src_h, d.src_w = V, H, W
    d.geo0_h, d.geo0_w = a["geo0"].shape[-2:]
    d.geo1_h, d.geo1_w = a["geo1"].shape[-2:]
    d.tex_h, d.tex_w = a["tex"].shape[-2:]
    d.disable_fg_mask = int(disable_fg_mask)
    d.znear, d.zfar, d.nml_scale, d.sigma = 2.0, 5.0, 100.0, 0.1
    dev = {k: put(B, v, off if k in ("img", "geo0", "geo1", "tex") else 0) for k, v in a.items()}
    for k, v in dev.items():
        if k == "fg_mask" and disable_fg_mask:
            continue
        setattr(d, k, v.ctypes.data if isinstance(B, HostArrays) else v.data_ptr())
    nbytes = L.kpn_scene_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0, L.kpn_last_error()
    if ws is None:
        ws = B.full(nbytes // 4, np.nan)          # whatever a fresh workspace holds: the flags are zeroed by the call
    off6 = (ctypes.c_size_t * 6)()
    L.check(L.kpn_scene_layout(ctypes.byref(d), off6))
    L.check(L.kpn_scene_prepare(ctypes.byref(d), B.ptr(ws), B.stream))
    return B.get(ws), list(off6), ws


def region(w, o, shape):
    return w[o:o + int(np.prod(shape))].reshape(shape)


def want_flag(a):
    return max(int((bits(a[k]) & 0x7FFFFFFF).max()) for k in ("img", "geo0", "geo1", "tex"))


def check_maps(w, off, a, disable_fg_mask):
    V, _, H, W = a["img"].shape
    for k, o in (("geo0", off[2]), ("geo1", off[3]), ("tex", off[4])):
        ref = torch.from_numpy(a[k]).permute(0, 2, 3, 1).contiguous().numpy()
        assert np.array_equal(bits(region(w, o, ref.shape)), bits(ref)), k
    m = np.ones((V, H, W), np.float32) if disable_fg_mask else (a["fg_mask"] != 0).astype(np.float32)
    rgbm = np.concatenate([a["img"].transpose(0, 2, 3, 1), m[..., None]], -1)
    assert np.array_equal(bits(region(w, off[1], rgbm.shape)), bits(rgbm))
    assert int(bits(w[off[5]:off[5] + 1])[0]) == want_flag(a)
    assert (bits(w[off[5] + 1:off[5] + 16]) == 0).all()


def check_table(w, off, a):
    V = a["img"].shape[0]
    tb = region(w, off[0], (V, 112))
    assert np.array_equal(tb[:, 0:12], a["KRT"].reshape(V, 16)[:, :12]) and np.array_equal(tb[:, 12:24], a["extrin"].reshape(V, 16)[:, :12])
    cpos = np.linalg.inv(a["KRT"].astype(np.float64))[:, :3, 3]
    np.testing.assert_allclose(tb[:, 24:27], cpos, rtol=1e-6, atol=1e-6)       # the fp64 inverse, rounded once
    E = a["extrin"].astype(np.float64)
    kcam = np.einsum("vij,kj->vki", E[:, :3, :3], a["kpt3d"].astype(np.float64)) + E[:, None, :3, 3]
    np.testing.assert_allclose(tb[:, 28:100].reshape(V, 24, 3), kcam, rtol=0, atol=4e-6)   # four fp32 roundings at |value| < 8
    assert (bits(tb[:, 27]) == 0).all() and (bits(tb[:, 100:]) == 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("disable_fg_mask", [False, True])
@pytest.mark.parametrize("case,off", [("odd", 0), ("straddle", 0), ("vec", 0), ("vec", 1)])
def test_prepared_maps_are_the_channels_last_inputs(backend, case, off, disable_fg_mask):
    L, B = _env(backend)
    a = inputs(case)
    w, o, _ = prepare(L, B, a, disable_fg_mask, off)
    assert o[0] == 0 and all(x % 64 == 0 for x in o) and sorted(o) == o
    check_maps(w, o, a, disable_fg_mask)
    check_table(w, o, a)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ["odd", "straddle", "vec"])
def test_flag_shows_a_planted_maximum_a_nan_and_is_zeroed_again(backend, case):
    L, B = _env(backend)
    clean = inputs(case)
    big = {k: v.copy() for k, v in clean.items()}
    big["tex"].reshape(-1)[-1] = 7e4                         # the last element the last copy kernel reads
    w, o, ws = prepare(L, B, big)
    assert int(bits(w[o[5]:o[5] + 1])[0]) == BIG_BITS == want_flag(big)
    check_maps(w, o, big, False)
    # the same workspace, smaller values: the flag comes down, so the call zeroed it before its copies raised it
    w, o, ws = prepare(L, B, clean, ws=ws)
    assert int(bits(w[o[5]:o[5] + 1])[0]) == want_flag(clean) < BIG_BITS
    w2, _, _ = prepare(L, B, clean, ws=ws)
    assert np.array_equal(bits(w2), bits(w))                 # two consecutive prepares: the same flag, and the same everything
    nan = {k: v.copy() for k, v in clean.items()}
    nan["geo1"].reshape(-1)[0] = np.nan
    nan["geo0"].reshape(-1)[5] = np.inf                      # a NaN ranks above +inf
    w, o, _ = prepare(L, B, nan, ws=ws)
    f = w[o[5]]
    assert np.isnan(f) and int(bits(w[o[5]:o[5] + 1])[0]) == want_flag(nan) > 0x7F800000
    check_maps(w, o, nan, False)


def test_layout_refuses_a_bad_descriptor():
    from tests import simt_harness as sh
    L = sh.simt_lib()
    off6 = (ctypes.c_size_t * 6)()
    assert L.kpn_scene_layout(ctypes.byref(kl.SceneDesc()), off6) != 0 and L.kpn_last_error()
