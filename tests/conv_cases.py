"""Test infrastructure of the native convolution (kpn_conv2d_*): the cases, their fp64 reference, the bar and one driver of the
C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.

Reference: seeded normal x, w, b and seed gradient g give y, dX, dW, db from torch.nn.functional.conv2d and torch.autograd.grad
on the CPU in fp64.  e_ref is the max deviation of the same computation in CPU fp32 from that, per tensor.  The bar, for every
element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)) - the project's standing rule and factor
(tests/test_encoders_cpu.py, the train-loss tests).
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from keypointnerf_amd import lib as kl

# what each case can catch:
CASES = {
    # the 128 x 32 tile, a ragged pixel tile (70 pixels), every border tap, K = 36 (no multiple of 16)
    "k3_4to8": dict(N=2, H=5, W=7, cin=4, cout=8, k=3, pad=1, bias=True),
    # the 64 x 64 tile with a single tap; dX has cout as its K
    "k1_8to64": dict(N=1, H=6, W=6, cin=8, cout=64, k=1, pad=0, bias=False),
    # cin no multiple of 16, cout no multiple of 32: padded channels must not leak into dW; transposed pad k - 1 - p = 2
    "k5_12to36": dict(N=2, H=9, W=9, cin=12, cout=36, k=5, pad=2, bias=True),
    # the output size differs from the input size, and the input-gradient pad (2 / 0) differs from p (0 / 2)
    "k3_p0": dict(N=1, H=8, W=8, cin=4, cout=4, k=3, pad=0, bias=True),
    "k3_p2": dict(N=1, H=8, W=8, cin=4, cout=4, k=3, pad=2, bias=False),
    # 768 output pixels = 48 chunks: three wgrad ranges of 20, 20 and 8 chunks
    "ranges3": dict(N=3, H=16, W=16, cin=16, cout=32, k=3, pad=1, bias=True),
    # 320 output pixels = 20 chunks: exactly one full range (one pixel more would open a second)
    "range1": dict(N=1, H=16, W=20, cin=8, cout=8, k=3, pad=1, bias=True),
}
FACTOR = 4.0


def out_hw(c):
    return c["H"] + 2 * c["pad"] - c["k"] + 1, c["W"] + 2 * c["pad"] - c["k"] + 1


def desc(c, **over):
    d = kl.Conv2dDesc()
    v = dict(c, has_bias=int(c["bias"]))
    v.update(over)
    for n in ("N", "H", "W", "cin", "cout", "k", "pad", "has_bias"):
        setattr(d, n, int(v[n]))
    return d


def expected_ranges(c):
    """The range rule of include/kpnerf.h (kpn_conv2d_wgrad_ranges), restated: a range is max(20, ceil(chunks / rmax)) chunks of
    16 output pixels, rmax = clamp(1024 / tiles, 1, 64), tiles those of the (k k cin) x cout result."""
    Ho, Wo = out_hw(c)
    chunks = -(-c["N"] * Ho * Wo // 16)
    bm, bn = (64, 64) if c["cout"] > 32 else (128, 32)
    tiles = -(-c["k"] * c["k"] * c["cin"] // bm) * -(-c["cout"] // bn)
    rmax = max(1, min(64, 1024 // tiles))
    cpr = max(20, -(-chunks // rmax))
    return -(-chunks // cpr), chunks, cpr


def inputs(c, seed=0):
    """x (N, cin, H, W), w (cout, cin, k, k), b (cout) or None, g (N, cout, Ho, Wo): seeded normal, fp32, NCHW"""
    gen = torch.Generator().manual_seed(1000 + seed)
    Ho, Wo = out_hw(c)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    x, w = r(c["N"], c["cin"], c["H"], c["W"]), r(c["cout"], c["cin"], c["k"], c["k"])
    b = r(c["cout"]) if c["bias"] else None
    return x, w, b, r(c["N"], c["cout"], Ho, Wo)


def _torch_run(c, x, w, b, g, dtype):
    x, w, g = (t.clone().to(dtype).requires_grad_(True) for t in (x, w, g))
    b = None if b is None else b.clone().to(dtype).requires_grad_(True)
    y = F.conv2d(x, w, b, stride=1, padding=c["pad"])
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


def ratio(native, f64, e_ref):
    """(max|native - fp64| - 1 ulp of max|fp64|) / e_ref, floored at 0: the bar is ratio <= FACTOR"""
    err = float(np.abs(np.asarray(native, np.float64) - f64).max())
    over = max(0.0, err - float(np.spacing(np.float32(np.abs(f64).max()))))
    if over == 0.0:
        return 0.0
    return over / e_ref if e_ref > 0.0 else float("inf")


def check(label, native, f64, e_ref):
    assert np.isfinite(np.asarray(native)).all(), label
    r = ratio(native, f64, e_ref)
    print(f"[conv parity] {label}: ratio {r:.3f} (e_ref {e_ref:.3e}, bar {FACTOR:g})")
    assert r <= FACTOR, (label, r, e_ref)
    return r


def nhwc(t):
    """NCHW torch / numpy -> contiguous NHWC numpy fp32"""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1), dtype=np.float32)


def nchw(a):
    return np.asarray(a).transpose(0, 3, 1, 2)


class HostArrays:
    """numpy buffers: the emulator build"""
    stream = None

    def put(self, a):
        return np.ascontiguousarray(a, dtype=np.float32)

    def full(self, shape, value, dtype=np.float32):
        return np.full(shape, value, dtype)

    def ptr(self, a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def get(self, a):
        return None if a is None else a.copy()


class DeviceArrays:
    """torch tensors on the GPU: the product library"""

    @property
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def full(self, shape, value, dtype=np.float32):
        return torch.full(tuple(int(v) for v in np.atleast_1d(shape)), value, dtype={np.float32: torch.float32, np.uint8: torch.uint8}[dtype],
                          device="cuda")

    def ptr(self, a):
        return None if a is None else ctypes.c_void_p(a.data_ptr())

    def get(self, a):
        return None if a is None else a.cpu().numpy()


CANARY = -7.25


def pack(L, B, c, w):
    d = desc(c)
    n = L.kpn_conv2d_packed_floats(ctypes.byref(d))
    assert n > 0
    packed = B.full(n, np.nan)
    w_dev = B.put(w)
    L.check(L.kpn_conv2d_pack_device(ctypes.byref(d), B.ptr(w_dev), B.ptr(packed), B.stream))
    return packed


def workspace(L, B, c):
    nb = L.kpn_conv2d_workspace_bytes(ctypes.byref(desc(c)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


def forward(L, B, c, x_nhwc, packed, b):
    """kpn_conv2d_forward -> y NHWC (numpy)"""
    d = desc(c)
    Ho, Wo = out_hw(c)
    y = B.full((c["N"], Ho, Wo, c["cout"]), np.nan)
    ws, nb = workspace(L, B, c)
    x_dev, b_dev = B.put(x_nhwc), (None if b is None else B.put(b))
    L.check(L.kpn_conv2d_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb, B.stream))
    return B.get(y)


def backward(L, B, c, x_nhwc, dy_nhwc, packed, legs=("dx", "dw", "db")):
    """kpn_conv2d_backward -> {dx NHWC, dw OIHW, db}: every buffer is pre-filled with CANARY and returned whether or not its leg ran"""
    d = desc(c)
    bufs = {"dx": B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), "dw": B.full((c["cout"], c["cin"], c["k"], c["k"]), CANARY),
            "db": B.full(c["cout"], CANARY)}
    ws, nb = workspace(L, B, c)
    x_dev, dy_dev = B.put(x_nhwc), B.put(dy_nhwc)
    L.check(L.kpn_conv2d_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), B.ptr(packed), *[B.ptr(bufs[k]) if k in legs else None
                                                                                                for k in ("dx", "dw", "db")],
                                  B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


def legs_of(c):
    return ("dx", "dw", "db") if c["bias"] else ("dx", "dw")


# ---- the properties both builds are held to (tests/test_conv_cpu.py on the emulator, tests/test_gpu_conv.py on the device) ----
def check_case(L, B, name):
    """y, dX, dW, db of one case against the fp64 reference, each within the bar; -> {tensor: ratio}"""
    c = CASES[name]
    (x, w, b, g), r64, e_ref = reference(name)
    packed = pack(L, B, c, w.numpy())
    y = forward(L, B, c, nhwc(x), packed, None if b is None else b.numpy())
    out = backward(L, B, c, nhwc(x), nhwc(g), packed, legs_of(c))
    ratios = {"y": check(f"{name} y", nchw(y), r64["y"], e_ref["y"]),
              "dx": check(f"{name} dx", nchw(out["dx"]), r64["dx"], e_ref["dx"]),
              "dw": check(f"{name} dw", out["dw"], r64["dw"], e_ref["dw"])}
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
        y = forward(L, B, c, nhwc(x), packed, None if b is None else b.numpy())
        out = backward(L, B, c, nhwc(x), nhwc(g), packed, legs_of(c))
        runs.append([B.get(packed), y] + [out[k] for k in ("dx", "dw", "db")])
    for a, b2 in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b2.view(np.uint32))


def check_null_legs_leave_buffers_alone(L, B, name):
    c = CASES[name]
    assert c["bias"]
    (x, w, b, g), _, _ = reference(name)
    packed = pack(L, B, c, w.numpy())
    full = backward(L, B, c, nhwc(x), nhwc(g), packed)
    for only in ("dx", "dw", "db"):
        out = backward(L, B, c, nhwc(x), nhwc(g), packed, legs=(only,))
        for k in ("dx", "dw", "db"):
            if k == only:
                assert np.array_equal(out[k], full[k]), (only, k)       # a leg does not depend on the others
            else:
                assert (out[k] == CANARY).all(), (only, k)
    assert not any((full[k] == CANARY).all() for k in full)


def check_zero_dy_gives_zeros(L, B, name):
    c = CASES[name]
    (x, w, b, g), _, _ = reference(name)
    out = backward(L, B, c, nhwc(x), np.zeros_like(nhwc(g)), pack(L, B, c, w.numpy()), legs_of(c))
    for k in legs_of(c):
        assert (out[k] == 0.0).all(), k


def check_bad_descriptors(L, B):
    c = CASES["k3_4to8"]
    (x, w, b, g), _, _ = reference("k3_4to8")
    packed = pack(L, B, c, w.numpy())
    ws, nb = workspace(L, B, c)
    x_dev, g_dev, b_dev = B.put(nhwc(x)), B.put(nhwc(g)), B.put(b.numpy())
    Ho, Wo = out_hw(c)
    y = B.full((c["N"], Ho, Wo, c["cout"]), CANARY)
    dx = B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY)

    def fwd(d, x_=x_dev, nb_=nb):
        return L.kpn_conv2d_forward(ctypes.byref(d), B.ptr(x_), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb_, B.stream)

    def bwd(d, dy_=g_dev, nb_=nb):
        return L.kpn_conv2d_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_), B.ptr(packed), B.ptr(dx), None, None, B.ptr(ws), nb_, B.stream)

    # the stems (k = 7, the only stride-2 / 7 x 7 layers), p >= k, channels that are no multiple of 4: each names its field
    for over, word in ((dict(k=7, pad=3), b"k must"), (dict(pad=3), b"pad must"), (dict(cin=6), b"cin must"), (dict(cout=10), b"cout must"),
                       (dict(H=0), b"N, H, W")):
        d = desc(c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_conv2d_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_conv2d_wgrad_ranges(ctypes.byref(d)) == 0
    d7 = desc(c, k=7)
    assert L.kpn_conv2d_packed_floats(ctypes.byref(d7)) == 0
    assert L.kpn_conv2d_pack_device(ctypes.byref(d7), B.ptr(x_dev), B.ptr(packed), B.stream) == -1 and b"k must" in L.kpn_last_error()
    d = desc(c)
    assert fwd(d, x_=None) == -1 and b"null" in L.kpn_last_error()
    assert bwd(d, dy_=None) == -1 and b"null" in L.kpn_last_error()
    assert fwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert (B.get(y) == CANARY).all() and (B.get(dx) == CANARY).all()          # a refused call launches nothing
    assert fwd(d) == 0 and bwd(d) == 0


def check_range_counts(L):
    for name, want in (("ranges3", 3), ("range1", 1)):
        c = CASES[name]
        n, chunks, cpr = expected_ranges(c)
        assert n == want and L.kpn_conv2d_wgrad_ranges(ctypes.byref(desc(c))) == want
        if name == "ranges3":
            assert chunks % cpr != 0 and chunks - (n - 1) * cpr < cpr          # a ragged last range
        else:
            assert chunks == cpr                                               # exactly full
    # one pixel row more than range1 opens a second range
    assert L.kpn_conv2d_wgrad_ranges(ctypes.byref(desc(dict(CASES["range1"], H=17)))) == 2


def stand_in_stack(seed=3):
    """the small stack install_native_convs is tried on: two convolutions it serves around a GroupNorm, and a stride-2 one it leaves"""
    nn = torch.nn
    net = nn.Sequential(nn.Conv2d(8, 16, 3, padding=1, bias=False), nn.GroupNorm(4, 16), nn.ReLU(), nn.Conv2d(16, 8, 1),
                        nn.Conv2d(8, 8, 3, stride=2, padding=1))
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * seed + i)) * (0.3 if p.dim() > 1 else 1.0))
    return net
