"""Test infrastructure of the native stride-2, stem and transposed convolutions (kpn_conv2d_s2_*): the cases, their fp64 reference
and one driver of the C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.  The
buffers, the bar and its factor are those of tests/conv_cases.py.

Reference: seeded normal x, w, b and seed gradient g give y, dX, dW, db from torch.nn.functional.conv2d / conv_transpose2d and
torch.autograd.grad on the CPU in fp64.  e_ref is the max deviation of the same computation in CPU fp32 from that, per tensor.
The bar, for every element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)).
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from keypointnerf_amd import lib as kl
from tests.conv_cases import CANARY, DeviceArrays, HostArrays, check, nchw, nhwc, ratio  # noqa: F401  (re-exported to the two test files)

CONV3, STEM7, DECONV3 = kl.S2_CONV3, kl.S2_STEM7, kl.S2_DECONV3

# what each case can catch:
CASES = {
    # the 128 x 32 tile, a ragged 30-pixel tile, the top / left pad taps; dX: every parity class without split K
    "s2_4to8": dict(kind=CONV3, N=2, H=6, W=10, cin=4, cout=8, bias=True),
    # the 64 x 64 tile, channels that fill no tile (padded ones must not leak); dX with split K and the deconv combine
    "s2_12to36": dict(kind=CONV3, N=1, H=8, W=8, cin=12, cout=36, bias=False),
    # one output pixel: every dX class has a tap outside the source
    "s2_2x2": dict(kind=CONV3, N=1, H=2, W=2, cin=4, cout=4, bias=False),
    # 768 output pixels = 48 chunks: three wgrad ranges of 20, 20 and 8 chunks
    "s2_ranges": dict(kind=CONV3, N=3, H=32, W=32, cin=16, cout=32, bias=True),
    # the 64 x 64 tile; K = 49 * 4 = 196 rows of which 147 are real (the padded channel); pad taps on all four borders
    "stem_3to64": dict(kind=STEM7, N=2, H=10, W=6, cin=3, cout=64, bias=True),
    # the 128 x 32 tile; odd sizes: 9 x 7 -> 5 x 4
    "stem_odd": dict(kind=STEM7, N=1, H=9, W=7, cin=3, cout=8, bias=False),
    # 32 x 24 = 768 output pixels: three ranges over stem loads
    "stem_ranges": dict(kind=STEM7, N=1, H=64, W=48, cin=3, cout=64, bias=False),
    # the four parity classes with a ragged tile and a bias; dX is a stride-2 convolution with border taps; swapped-role dW
    "up_8to4": dict(kind=DECONV3, N=2, H=3, W=5, cin=8, cout=4, bias=True),
    # padded channels in the swapped-role dW (its GEMM has 12 input and 36 output channels); the 64 x 64 tile
    "up_36to12": dict(kind=DECONV3, N=1, H=4, W=4, cin=36, cout=12, bias=False),
    # one source pixel: three of the four classes have only taps outside it
    "up_1x1": dict(kind=DECONV3, N=1, H=1, W=1, cin=4, cout=4, bias=False),
    # 768 source pixels: three ranges of the swapped-role dW
    "up_ranges": dict(kind=DECONV3, N=3, H=16, W=16, cin=32, cout=16, bias=False),
}
ONE_PER_KIND = ("s2_12to36", "stem_3to64", "up_36to12")


def out_hw(c):
    if c["kind"] == DECONV3:
        return 2 * c["H"], 2 * c["W"]
    return (c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1


def k_of(c):
    return 7 if c["kind"] == STEM7 else 3


def w_shape(c):
    k = k_of(c)
    return (c["cin"], c["cout"], k, k) if c["kind"] == DECONV3 else (c["cout"], c["cin"], k, k)


def desc(c, **over):
    d = kl.Conv2dS2Desc()
    v = dict(c, has_bias=int(c["bias"]))
    v.update(over)
    for n in ("N", "H", "W", "cin", "cout", "kind", "has_bias"):
        setattr(d, n, int(v[n]))
    return d


def expected_ranges(c):
    """The range rule of include/kpnerf.h, restated: chunks of 16 GEMM pixels; tiles = ceil(taps cin_p / BM) ceil(cout / BN) of the
    GEMM whose rows the weight gradient takes (the transposed layer: cout -> cin over the source pixels); a range is
    max(20, ceil(chunks / clamp(1024 / tiles, 1, 64))) chunks."""
    Ho, Wo = out_hw(c)
    gin, gout, pix = (c["cout"], c["cin"], c["N"] * c["H"] * c["W"]) if c["kind"] == DECONV3 else (c["cin"], c["cout"], c["N"] * Ho * Wo)
    chunks = -(-pix // 16)
    bm, bn = (64, 64) if gout > 32 else (128, 32)
    tiles = -(-k_of(c) ** 2 * (-(-gin // 4) * 4) // bm) * -(-gout // bn)
    rmax = max(1, min(64, 1024 // tiles))
    cpr = max(20, -(-chunks // rmax))
    return -(-chunks // cpr), chunks, cpr


def inputs(c, seed=0):
    """x (N, cin, H, W), w, b (cout) or None, g (N, cout, Ho, Wo): seeded normal, fp32, NCHW"""
    gen = torch.Generator().manual_seed(2000 + seed)
    Ho, Wo = out_hw(c)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)  # noqa: E731
    x, w = r(c["N"], c["cin"], c["H"], c["W"]), r(*w_shape(c))
    b = r(c["cout"]) if c["bias"] else None
    return x, w, b, r(c["N"], c["cout"], Ho, Wo)


def torch_layer(c, x, w, b):
    if c["kind"] == DECONV3:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, b, stride=2, padding=3 if c["kind"] == STEM7 else 1)


def _torch_run(c, x, w, b, g, dtype):
    x, w, g = (t.clone().to(dtype).requires_grad_(True) for t in (x, w, g))
    b = None if b is None else b.clone().to(dtype).requires_grad_(True)
    y = torch_layer(c, x, w, b)
    grads = torch.autograd.grad(y, [x, w] + ([b] if b is not None else []), g.detach())
    out = {"y": y.detach(), "dx": grads[0], "dw": grads[1]}
    if b is not None:
        out["db"] = grads[2]
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name, seed=0):
    """-> (inputs, {tensor: fp64 array (NCHW; the weight in the layer's layout)}, {tensor: e_ref}); computed once per case and shared"""
    c = CASES[name]
    x, w, b, g = inputs(c, seed)
    r64, r32 = _torch_run(c, x, w, b, g, torch.float64), _torch_run(c, x, w, b, g, torch.float32)
    e_ref = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64}
    for v in r64.values():
        v.setflags(write=False)
    return (x, w, b, g), r64, e_ref


def x_layout(c, x):
    """the layer's input as the ABI takes it: NCHW as it is for the stem, NHWC otherwise"""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(a, dtype=np.float32) if c["kind"] == STEM7 else nhwc(a)


def pack(L, B, c, w):
    d = desc(c)
    n = L.kpn_conv2d_s2_packed_floats(ctypes.byref(d))
    assert n > 0
    packed = B.full(n, np.nan)
    w_dev = B.put(w)
    L.check(L.kpn_conv2d_s2_pack_device(ctypes.byref(d), B.ptr(w_dev), B.ptr(packed), B.stream))
    return packed


def workspace(L, B, c):
    nb = L.kpn_conv2d_s2_workspace_bytes(ctypes.byref(desc(c)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


def forward(L, B, c, x, packed, b):
    """kpn_conv2d_s2_forward -> y NHWC (numpy)"""
    d = desc(c)
    Ho, Wo = out_hw(c)
    y = B.full((c["N"], Ho, Wo, c["cout"]), np.nan)
    ws, nb = workspace(L, B, c)
    x_dev, b_dev = B.put(x), (None if b is None else B.put(b))
    L.check(L.kpn_conv2d_s2_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb, B.stream))
    return B.get(y)


def legs_of(c):
    return tuple(k for k, on in (("dx", c["kind"] != STEM7), ("dw", True), ("db", c["bias"])) if on)


def backward(L, B, c, x, dy_nhwc, packed, legs=None, nan_behind_x=False):
    """kpn_conv2d_s2_backward -> {dx NHWC, dw in the layer's layout, db}: every buffer is pre-filled with CANARY and returned whether
    or not its leg ran.  nan_behind_x: the memory that follows x holds NaNs"""
    legs = legs_of(c) if legs is None else legs
    d = desc(c)
    bufs = {"dx": B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), "dw": B.full(w_shape(c), CANARY), "db": B.full(c["cout"], CANARY)}
    ws, nb = workspace(L, B, c)
    x = np.asarray(x, np.float32)
    x_dev = B.put(np.concatenate([x.reshape(-1), np.full(256, np.nan, np.float32)]) if nan_behind_x else x)
    dy_dev = B.put(dy_nhwc)
    L.check(L.kpn_conv2d_s2_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), B.ptr(packed),
                                     *[B.ptr(bufs[k]) if k in legs else None for k in ("dx", "dw", "db")], B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


# ---- the properties both builds are held to (tests/test_strided_cpu.py on the emulator, tests/test_gpu_strided.py on the device) ----
def check_case(L, B, name):
    """y, dX, dW, db of one case against the fp64 reference, each within the bar; -> {tensor: ratio}"""
    c = CASES[name]
    (x, w, b, g), r64, e_ref = reference(name)
    packed = pack(L, B, c, w.numpy())
    y = forward(L, B, c, x_layout(c, x), packed, None if b is None else b.numpy())
    out = backward(L, B, c, x_layout(c, x), nhwc(g), packed)
    ratios = {"y": check(f"{name} y", nchw(y), r64["y"], e_ref["y"]), "dw": check(f"{name} dw", out["dw"], r64["dw"], e_ref["dw"])}
    if c["kind"] != STEM7:
        ratios["dx"] = check(f"{name} dx", nchw(out["dx"]), r64["dx"], e_ref["dx"])
    else:
        assert (out["dx"] == CANARY).all()
    if c["bias"]:
        ratios["db"] = check(f"{name} db", out["db"], r64["db"], e_ref["db"])
    else:
        assert (out["db"] == CANARY).all()
    return ratios


def check_two_calls_equal_bits(L, B, name):
    c = CASES[name]
    (x, w, b, g), _, _ = reference(name)
    runs = []
    for _ in range(2):
        packed = pack(L, B, c, w.numpy())
        y = forward(L, B, c, x_layout(c, x), packed, None if b is None else b.numpy())
        out = backward(L, B, c, x_layout(c, x), nhwc(g), packed)
        runs.append([B.get(packed), y] + [out[k] for k in ("dx", "dw", "db")])
    for a, b2 in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b2.view(np.uint32))


def check_null_legs_leave_buffers_alone(L, B, name):
    c = CASES[name]
    assert c["bias"]
    (x, w, b, g), _, _ = reference(name)
    packed = pack(L, B, c, w.numpy())
    full = backward(L, B, c, x_layout(c, x), nhwc(g), packed)
    for only in legs_of(c):
        out = backward(L, B, c, x_layout(c, x), nhwc(g), packed, legs=(only,))
        for k in ("dx", "dw", "db"):
            if k == only:
                assert np.array_equal(out[k], full[k]), (only, k)       # a leg does not depend on the others
            else:
                assert (out[k] == CANARY).all(), (only, k)
    assert not any((full[k] == CANARY).all() for k in legs_of(c))


def check_zero_dy_gives_zeros(L, B, name):
    c = CASES[name]
    (x, w, b, g), _, _ = reference(name)
    out = backward(L, B, c, x_layout(c, x), np.zeros_like(nhwc(g)), pack(L, B, c, w.numpy()))
    for k in legs_of(c):
        assert (out[k] == 0.0).all(), k


def check_range_counts(L):
    for name in ("s2_ranges", "stem_ranges", "up_ranges"):
        c = CASES[name]
        n, chunks, cpr = expected_ranges(c)
        assert (n, chunks, cpr) == (3, 48, 20)                                  # 20 / 20 / 8: a ragged last range
        assert L.kpn_conv2d_s2_wgrad_ranges(ctypes.byref(desc(c))) == n
    for name in ("s2_4to8", "stem_odd", "up_1x1"):
        assert L.kpn_conv2d_s2_wgrad_ranges(ctypes.byref(desc(CASES[name]))) == expected_ranges(CASES[name])[0] == 1


def check_padded_stem_channel(L, B):
    """dw of stem_3to64 is the same, bit for bit, when NaNs follow x in memory: the loader never touches the fourth channel"""
    c = CASES["stem_3to64"]
    (x, w, b, g), _, _ = reference("stem_3to64")
    packed = pack(L, B, c, w.numpy())
    plain = backward(L, B, c, x_layout(c, x), nhwc(g), packed, legs=("dw",))["dw"]
    nan = backward(L, B, c, x_layout(c, x), nhwc(g), packed, legs=("dw",), nan_behind_x=True)["dw"]
    assert np.isfinite(plain).all() and np.array_equal(plain.view(np.uint32), nan.view(np.uint32))


def check_refusals(L, B):
    """every refusal names its field, and a refused call launches nothing"""
    canaries = []

    def calls(name):
        c = CASES[name]
        (x, w, b, g), _, _ = reference(name)
        packed = pack(L, B, c, w.numpy())
        ws, nb = workspace(L, B, c)
        x_dev, g_dev = B.put(x_layout(c, x)), B.put(nhwc(g))
        b_dev = None if b is None else B.put(b.numpy())
        Ho, Wo = out_hw(c)
        y = B.full((c["N"], Ho, Wo, c["cout"]), CANARY)
        dx, dw = B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), B.full(w_shape(c), CANARY)
        canaries.extend([y, dx, dw])

        def fwd(d, x_=x_dev, nb_=nb):
            return L.kpn_conv2d_s2_forward(ctypes.byref(d), B.ptr(x_), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb_, B.stream)

        def bwd(d, dy_=g_dev, nb_=nb, dx_=dx):
            return L.kpn_conv2d_s2_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_), B.ptr(packed), B.ptr(dx_), B.ptr(dw), None, B.ptr(ws), nb_,
                                            B.stream)
        return c, fwd, bwd, x_dev, packed

    c, fwd, bwd, x_dev, packed = calls("s2_4to8")
    for over, word in ((dict(H=5), b"H, W must be even"), (dict(cin=6), b"cin must"), (dict(cout=10), b"cout must"), (dict(kind=3), b"kind must"),
                       (dict(kind=-1), b"kind must"), (dict(N=0), b"N, H, W"), (dict(has_bias=2), b"has_bias")):
        d = desc(c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_conv2d_s2_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_conv2d_s2_wgrad_ranges(ctypes.byref(d)) == 0
    d6 = desc(c, cin=6)
    assert L.kpn_conv2d_s2_packed_floats(ctypes.byref(d6)) == 0
    assert L.kpn_conv2d_s2_pack_device(ctypes.byref(d6), B.ptr(x_dev), B.ptr(packed), B.stream) == -1 and b"cin must" in L.kpn_last_error()
    d = desc(c)
    assert fwd(d, x_=None) == -1 and b"null" in L.kpn_last_error()
    assert bwd(d, dy_=None) == -1 and b"null" in L.kpn_last_error()
    assert fwd(d, nb_=nb_less(L, c)) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb_less(L, c)) == -1 and b"workspace" in L.kpn_last_error()
    cs, fwd_s, bwd_s, _, _ = calls("stem_3to64")
    ds = desc(cs, cin=5)
    for call in (fwd_s, bwd_s):
        assert call(ds) == -1 and b"cin must" in L.kpn_last_error()
    assert L.kpn_conv2d_s2_packed_floats(ctypes.byref(ds)) == 0
    assert bwd_s(desc(cs)) == -1 and b"dx must be NULL" in L.kpn_last_error()
    for buf in canaries:
        assert (B.get(buf) == CANARY).all()                                    # a refused call launches nothing
    assert fwd(d) == 0 and bwd(d) == 0 and fwd_s(desc(cs)) == 0 and bwd_s(desc(cs), dx_=None) == 0
    assert L.kpn_abi_version() == 10


def nb_less(L, c):
    return L.kpn_conv2d_s2_workspace_bytes(ctypes.byref(desc(c))) - 1
