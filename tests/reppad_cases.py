"""Test infrastructure of the native replication-padded convolutions (kpn_conv2d_rp_*): the cases, their fp64 reference and one driver
of the C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.  The buffers, the bar and
its factor are those of tests/conv_cases.py.

Reference: seeded normal x, w, b and seed gradient g give y, dX, dW, db from F.conv2d(F.pad(x, (p,) * 4, mode="replicate"), w, b) and
torch.autograd.grad on the CPU in fp64.  e_ref is the max deviation of the same computation in CPU fp32 from that, per tensor.
The bar, for every element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)).

The native dX adds the ring's dy values before the product, torch adds the products: another rounding, not a larger one (a sum of at
most 16 values, one rounding each, in front of a chain of 9 cout or 49 cout products).  tests/test_reppad_cpu.py checks on the CPU that
no case needs more than the factor 4 for it.
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from keypointnerf_amd import lib as kl
from tests.conv_cases import CANARY, DeviceArrays, HostArrays, check, nchw, nhwc, ratio  # noqa: F401  (re-exported to the two test files)

CONV3, CONV7, STEM7 = kl.RP_CONV3, kl.RP_CONV7, kl.RP_STEM7

# what each case can catch:
CASES = {
    # odd sizes, the 128 x 32 tile, a ragged 70-pixel tile, all four edges and corners
    "rp3_4to8": dict(kind=CONV3, N=2, H=5, W=7, cin=4, cout=8, bias=True),
    # the 64 x 64 tile, padded channels, dX with split K
    "rp3_12to36": dict(kind=CONV3, N=1, H=8, W=8, cin=12, cout=36, bias=False),
    # both ends of the range on one pixel: dx is the sum over all nine taps
    "rp3_1x1": dict(kind=CONV3, N=1, H=1, W=1, cin=4, cout=4, bias=False),
    # every row is a border row, W has one interior column
    "rp3_2x3": dict(kind=CONV3, N=1, H=2, W=3, cin=4, cout=4, bias=True),
    # 768 pixels = 48 chunks: three wgrad ranges of 20, 20 and 8 chunks
    "rp3_ranges": dict(kind=CONV3, N=3, H=16, W=16, cin=16, cout=32, bias=True),
    # H smaller than the kernel, ring sums of up to 4 per axis
    "rp7_8to4": dict(kind=CONV7, N=2, H=5, W=9, cin=8, cout=4, bias=True),
    # a tensor smaller than the pad: every pixel is a corner
    "rp7_2x2": dict(kind=CONV7, N=1, H=2, W=2, cin=4, cout=4, bias=False),
    # the shipped output layer's proportions (cout < cin), interior and ring together
    "rp7_16to8": dict(kind=CONV7, N=1, H=12, W=12, cin=16, cout=8, bias=False),
    # NCHW loads with the clamp, the padded fourth channel, no dx
    "rp7stem_3to16": dict(kind=STEM7, N=2, H=10, W=6, cin=3, cout=16, bias=True),
    # 768 pixels: three ranges over stem loads, the 64 x 64 tile
    "rp7stem_ranges": dict(kind=STEM7, N=1, H=32, W=24, cin=3, cout=64, bias=False),
}
ONE_PER_KIND = ("rp3_12to36", "rp7_8to4", "rp7stem_3to16")
CLOSED_FORM = ("rp3_1x1", "rp7_2x2")


def k_of(c):
    return 3 if c["kind"] == CONV3 else 7


def w_shape(c):
    return (c["cout"], c["cin"], k_of(c), k_of(c))


def desc(c, **over):
    d = kl.Conv2dRpDesc()
    v = dict(c, has_bias=int(c["bias"]))
    v.update(over)
    for n in ("N", "H", "W", "cin", "cout", "kind", "has_bias"):
        setattr(d, n, int(v[n]))
    return d


def expected_ranges(c):
    """The range rule of include/kpnerf.h, restated: chunks of 16 pixels; tiles = ceil(k k cin_p / BM) ceil(cout / BN); a range is
    max(20, ceil(chunks / clamp(1024 / tiles, 1, 64))) chunks."""
    chunks = -(-c["N"] * c["H"] * c["W"] // 16)
    bm, bn = (64, 64) if c["cout"] > 32 else (128, 32)
    tiles = -(-k_of(c) ** 2 * (-(-c["cin"] // 4) * 4) // bm) * -(-c["cout"] // bn)
    rmax = max(1, min(64, 1024 // tiles))
    cpr = max(20, -(-chunks // rmax))
    return -(-chunks // cpr), chunks, cpr


def inputs(c, seed=0):
    """x (N, cin, H, W), w OIHW, b (cout) or None, g (N, cout, H, W): seeded normal, fp32, NCHW"""
    gen = torch.Generator().manual_seed(3000 + seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)  # noqa: E731
    x, w = r(c["N"], c["cin"], c["H"], c["W"]), r(*w_shape(c))
    b = r(c["cout"]) if c["bias"] else None
    return x, w, b, r(c["N"], c["cout"], c["H"], c["W"])


def torch_layer(c, x, w, b):
    p = k_of(c) // 2
    return F.conv2d(F.pad(x, (p,) * 4, mode="replicate"), w, b)


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
    """-> (inputs, {tensor: fp64 array (NCHW / OIHW)}, {tensor: e_ref}); computed once per case and shared"""
    c = CASES[name]
    x, w, b, g = inputs(c, seed)
    r64, r32 = _torch_run(c, x, w, b, g, torch.float64), _torch_run(c, x, w, b, g, torch.float32)
    e_ref = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64}
    for v in r64.values():
        v.setflags(write=False)
    return (x, w, b, g), r64, e_ref


def closed_form_dx(name):
    """dx of a case in which every pixel is a corner of the 3x3 (1 x 1) or 7x7 (2 x 2) kernel, without the reference driver, in fp64.
    1 x 1: every tap reads the one pixel, so dx[ci] = sum_co (sum_taps w[co][ci]) dy[co].  2 x 2 under pad 3: source row 0 serves the
    taps ky <= 3 - oy and row 1 the others, for either output row oy, so dx[n, ci, y, x] = sum_co sum_(oy, ox) S[co, ci, y, oy, x, ox]
    dy[n, co, oy, ox] with S the weight summed over those tap sets."""
    c = CASES[name]
    (x, w, b, g), _, _ = reference(name)
    w64, g64 = w.numpy().astype(np.float64), g.numpy().astype(np.float64)
    if (c["H"], c["W"]) == (1, 1):
        return np.einsum("oi,no->ni", w64.sum(axis=(2, 3)), g64[:, :, 0, 0])[:, :, None, None]
    assert (c["H"], c["W"], k_of(c)) == (2, 2, 7)
    sets = {(0, 0): slice(0, 4), (1, 0): slice(4, 7), (0, 1): slice(0, 3), (1, 1): slice(3, 7)}     # (source row, output row) -> taps
    dx = np.zeros((c["N"], c["cin"], 2, 2))
    for (sy, oy), ty in sets.items():
        for (sx, ox), tx in sets.items():
            dx[:, :, sy, sx] += np.einsum("oi,no->ni", w64[:, :, ty, tx].sum(axis=(2, 3)), g64[:, :, oy, ox])
    return dx


def x_layout(c, x):
    """the layer's input as the ABI takes it: NCHW as it is for the stem, NHWC otherwise"""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(a, dtype=np.float32) if c["kind"] == STEM7 else nhwc(a)


def pack(L, B, c, w):
    d = desc(c)
    n = L.kpn_conv2d_rp_packed_floats(ctypes.byref(d))
    assert n > 0
    packed = B.full(n, np.nan)
    w_dev = B.put(w)
    L.check(L.kpn_conv2d_rp_pack_device(ctypes.byref(d), B.ptr(w_dev), B.ptr(packed), B.stream))
    return packed


def workspace(L, B, c):
    nb = L.kpn_conv2d_rp_workspace_bytes(ctypes.byref(desc(c)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


def forward(L, B, c, x, packed, b):
    """kpn_conv2d_rp_forward -> y NHWC (numpy)"""
    d = desc(c)
    y = B.full((c["N"], c["H"], c["W"], c["cout"]), np.nan)
    ws, nb = workspace(L, B, c)
    x_dev, b_dev = B.put(x), (None if b is None else B.put(b))
    L.check(L.kpn_conv2d_rp_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb, B.stream))
    return B.get(y)


def legs_of(c):
    return tuple(k for k, on in (("dx", c["kind"] != STEM7), ("dw", True), ("db", c["bias"])) if on)


def backward(L, B, c, x, dy_nhwc, packed, legs=None, nan_behind_x=False):
    """kpn_conv2d_rp_backward -> {dx NHWC, dw OIHW, db}: every buffer is pre-filled with CANARY and returned whether or not its leg
    ran.  nan_behind_x: the memory that follows x holds NaNs"""
    legs = legs_of(c) if legs is None else legs
    d = desc(c)
    bufs = {"dx": B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), "dw": B.full(w_shape(c), CANARY), "db": B.full(c["cout"], CANARY)}
    ws, nb = workspace(L, B, c)
    x = np.asarray(x, np.float32)
    x_dev = B.put(np.concatenate([x.reshape(-1), np.full(256, np.nan, np.float32)]) if nan_behind_x else x)
    dy_dev = B.put(dy_nhwc)
    L.check(L.kpn_conv2d_rp_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), B.ptr(packed),
                                     *[B.ptr(bufs[k]) if k in legs else None for k in ("dx", "dw", "db")], B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


# ---- the properties both builds are held to (tests/test_reppad_cpu.py on the emulator, tests/test_gpu_reppad.py on the device) ----
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
        if name in CLOSED_FORM:         # a reference of its own: a bug shared with the driver above cannot hide
            ratios["dx_closed"] = check(f"{name} dx (closed form)", nchw(out["dx"]), closed_form_dx(name), e_ref["dx"])
    else:
        assert (out["dx"] == CANARY).all()
    if c["bias"]:
        ratios["db"] = check(f"{name} db", out["db"], r64["db"], e_ref["db"])
    else:
        assert (out["db"] == CANARY).all()
    return ratios


def check_a_wrong_ring_fails(name="rp3_4to8"):
    """the case a wrong ring fails: the zero-padded input gradient, which is right on every interior pixel, misses the bar of this case
    by orders of magnitude - on the ring"""
    c = CASES[name]
    (x, w, b, g), r64, e_ref = reference(name)
    xz = x.double().requires_grad_(True)
    zero = torch.autograd.grad(F.conv2d(xz, w.double(), padding=k_of(c) // 2), xz, g.double())[0].numpy()
    assert ratio(zero, r64["dx"], e_ref["dx"]) > 1e3
    assert ratio(zero[:, :, 1:-1, 1:-1], r64["dx"][:, :, 1:-1, 1:-1], e_ref["dx"]) <= 4.0


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
    for name in ("rp3_ranges", "rp7stem_ranges"):
        c = CASES[name]
        n, chunks, cpr = expected_ranges(c)
        assert (n, chunks, cpr) == (3, 48, 20)                                  # 20 / 20 / 8: a ragged last range
        assert L.kpn_conv2d_rp_wgrad_ranges(ctypes.byref(desc(c))) == n
    for name in ("rp3_4to8", "rp3_1x1", "rp7_2x2", "rp7_16to8", "rp7stem_3to16"):
        assert L.kpn_conv2d_rp_wgrad_ranges(ctypes.byref(desc(CASES[name]))) == expected_ranges(CASES[name])[0] == 1


def check_padded_stem_channel(L, B):
    """dw of rp7stem_3to16 is the same, bit for bit, when NaNs follow x in memory: the loader never touches the fourth channel"""
    c = CASES["rp7stem_3to16"]
    (x, w, b, g), _, _ = reference("rp7stem_3to16")
    packed = pack(L, B, c, w.numpy())
    plain = backward(L, B, c, x_layout(c, x), nhwc(g), packed, legs=("dw",))["dw"]
    nan = backward(L, B, c, x_layout(c, x), nhwc(g), packed, legs=("dw",), nan_behind_x=True)["dw"]
    assert np.isfinite(plain).all() and np.array_equal(plain.view(np.uint32), nan.view(np.uint32))


def nb_less(L, c):
    return L.kpn_conv2d_rp_workspace_bytes(ctypes.byref(desc(c))) - 1


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
        y = B.full((c["N"], c["H"], c["W"], c["cout"]), CANARY)
        dx, dw = B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), B.full(w_shape(c), CANARY)
        canaries.extend([y, dx, dw])

        def fwd(d, x_=x_dev, nb_=nb):
            return L.kpn_conv2d_rp_forward(ctypes.byref(d), B.ptr(x_), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb_, B.stream)

        def bwd(d, dy_=g_dev, nb_=nb, dx_=dx):
            return L.kpn_conv2d_rp_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_), B.ptr(packed), B.ptr(dx_), B.ptr(dw), None, B.ptr(ws), nb_,
                                            B.stream)
        return c, fwd, bwd, x_dev, packed

    c, fwd, bwd, x_dev, packed = calls("rp3_4to8")
    for over, word in ((dict(cin=6), b"cin must"), (dict(cout=10), b"cout must"), (dict(kind=3), b"kind must"), (dict(kind=-1), b"kind must"),
                       (dict(N=0), b"N, H, W"), (dict(has_bias=2), b"has_bias")):
        d = desc(c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_conv2d_rp_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_conv2d_rp_wgrad_ranges(ctypes.byref(d)) == 0
    d6 = desc(c, cin=6)
    assert L.kpn_conv2d_rp_packed_floats(ctypes.byref(d6)) == 0
    assert L.kpn_conv2d_rp_pack_device(ctypes.byref(d6), B.ptr(x_dev), B.ptr(packed), B.stream) == -1 and b"cin must" in L.kpn_last_error()
    d = desc(c)
    assert fwd(d, x_=None) == -1 and b"null" in L.kpn_last_error()
    assert bwd(d, dy_=None) == -1 and b"null" in L.kpn_last_error()
    assert fwd(d, nb_=nb_less(L, c)) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb_less(L, c)) == -1 and b"workspace" in L.kpn_last_error()
    cs, fwd_s, bwd_s, _, _ = calls("rp7stem_3to16")
    ds = desc(cs, cin=5)
    for call in (fwd_s, bwd_s):
        assert call(ds) == -1 and b"cin must" in L.kpn_last_error()
    assert L.kpn_conv2d_rp_packed_floats(ctypes.byref(ds)) == 0
    assert bwd_s(desc(cs)) == -1 and b"dx must be NULL" in L.kpn_last_error()
    for buf in canaries:
        assert (B.get(buf) == CANARY).all()                                    # a refused call launches nothing
    assert fwd(d) == 0 and bwd(d) == 0 and fwd_s(desc(cs)) == 0 and bwd_s(desc(cs), dx_=None) == 0
    assert L.kpn_abi_version() == 10
