"""One driver for the three single-layer convolution families of the C ABI (kpn_conv2d_*, kpn_conv2d_s2_*, kpn_conv2d_rp_*): the fp64
reference, the restated range rule, the ABI calls and the properties both builds are held to, each written once against a Family.
tests/conv_cases.py, tests/strided_cases.py and tests/reppad_cases.py hold the cases and their Family and bind these functions to it
under the names their test files use.  The bar and the buffers: tests/parity.py.

Reference: seeded normal x, w, b and seed gradient g give y, dX, dW, db from the family's torch layer and torch.autograd.grad on the
CPU in fp64.  e_ref is the max deviation of the same computation in CPU fp32 from that, per tensor.
"""
import ctypes
import dataclasses
import functools
import typing

import numpy as np
import torch

from tests.parity import CANARY, check, fp64_and_e_ref, nchw, nhwc


@dataclasses.dataclass(frozen=True, eq=False)
class Family:
    """what differs between the families; c is a case: N, H, W, cin, cout, bias and k, pad or kind"""
    cases: dict
    Desc: type                          # the ctypes descriptor
    fields: tuple                       # its fields, each the case's entry of that name (has_bias: the case's bias)
    prefix: str                         # of the entry points
    seed: int                           # the generator of a case's inputs is seeded with seed + the seed asked for
    k_of: typing.Callable               # c -> kernel size
    w_shape: typing.Callable            # c -> the weight as the layer holds it (IOHW for the transposed layer)
    out_hw: typing.Callable             # c -> (Ho, Wo)
    torch_layer: typing.Callable        # (c, x, w, b) -> y
    has_dx: typing.Callable             # c -> False for the stems, which have no input gradient
    x_is_nchw: typing.Callable          # c -> True where the ABI reads x as NCHW (the stems)
    wgrad_gemm: typing.Callable         # c -> (input channels, output channels, pixels) of the GEMM whose rows the weight gradient takes
    closed_form_dx: dict = dataclasses.field(default_factory=dict)      # case name -> a second fp64 reference of dx: name -> array

    def fn(self, L, name):
        return getattr(L, self.prefix + name)


def desc(fam, c, **over):
    d = fam.Desc()
    v = dict(c, has_bias=int(c["bias"]))
    v.update(over)
    for n in fam.fields:
        setattr(d, n, int(v[n]))
    return d


def expected_ranges(fam, c, tile=lambda cout: (64, 64) if cout > 32 else (128, 32)):
    """The range rule of include/kpnerf.h (kpn_conv2d*_wgrad_ranges), restated: chunks of 16 GEMM pixels; tiles = ceil(k k cin_p / BM)
    ceil(cout / BN) of the GEMM whose rows the weight gradient takes (cin_p: cin padded to 4, which only the stems need; the transposed
    layer: cout -> cin over the source pixels); a range is max(20, ceil(chunks / rmax)) chunks, rmax = clamp(1024 / tiles, 1, 64).
    -> (ranges, chunks, chunks per range)"""
    gin, gout, pix = fam.wgrad_gemm(c)
    chunks = -(-pix // 16)
    bm, bn = tile(gout)
    tiles = -(-fam.k_of(c) ** 2 * (-(-gin // 4) * 4) // bm) * -(-gout // bn)
    rmax = max(1, min(64, 1024 // tiles))
    cpr = max(20, -(-chunks // rmax))
    return -(-chunks // cpr), chunks, cpr


def inputs(fam, c, seed=0):
    """x (N, cin, H, W), w in the layer's layout, b (cout) or None, g (N, cout, Ho, Wo): seeded normal, fp32, NCHW"""
    gen = torch.Generator().manual_seed(fam.seed + seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)  # noqa: E731
    x, w = r(c["N"], c["cin"], c["H"], c["W"]), r(*fam.w_shape(c))
    b = r(c["cout"]) if c["bias"] else None
    return x, w, b, r(c["N"], c["cout"], *fam.out_hw(c))


def _torch_run(fam, c, x, w, b, g, dtype):
    x, w, g = (t.clone().to(dtype).requires_grad_(True) for t in (x, w, g))
    b = None if b is None else b.clone().to(dtype).requires_grad_(True)
    y = fam.torch_layer(c, x, w, b)
    grads = torch.autograd.grad(y, [x, w] + ([b] if b is not None else []), g.detach())
    out = {"y": y.detach(), "dx": grads[0], "dw": grads[1]}
    if b is not None:
        out["db"] = grads[2]
    return {k: v.numpy() for k, v in out.items()}


def reference_of(fam, c, seed=0):
    """-> (inputs, {tensor: fp64 array (NCHW; the weight in the layer's layout)}, {tensor: e_ref}) of a case given as its dict"""
    x, w, b, g = inputs(fam, c, seed)
    return ((x, w, b, g),) + fp64_and_e_ref(lambda dtype: _torch_run(fam, c, x, w, b, g, dtype))


@functools.lru_cache(maxsize=None)
def reference(fam, name, seed=0):
    """reference_of a case of the family by its name; computed once per case and shared"""
    return reference_of(fam, fam.cases[name], seed)


def x_layout(fam, c, x):
    """the layer's input as the ABI takes it: NCHW as it is for the stems, NHWC otherwise"""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(a, dtype=np.float32) if fam.x_is_nchw(c) else nhwc(a)


def pack(fam, L, B, c, w):
    d = desc(fam, c)
    n = fam.fn(L, "packed_floats")(ctypes.byref(d))
    assert n > 0
    packed = B.full(n, np.nan)
    w_dev = B.put(w)
    L.check(fam.fn(L, "pack_device")(ctypes.byref(d), B.ptr(w_dev), B.ptr(packed), B.stream))
    return packed


def workspace(fam, L, B, c):
    nb = fam.fn(L, "workspace_bytes")(ctypes.byref(desc(fam, c)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


def forward(fam, L, B, c, x, packed, b):
    """<prefix>forward -> y NHWC (numpy); x as x_layout gives it"""
    d = desc(fam, c)
    y = B.full((c["N"],) + tuple(fam.out_hw(c)) + (c["cout"],), np.nan)
    ws, nb = workspace(fam, L, B, c)
    x_dev, b_dev = B.put(x), (None if b is None else B.put(b))
    L.check(fam.fn(L, "forward")(ctypes.byref(d), B.ptr(x_dev), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb, B.stream))
    return B.get(y)


def legs_of(fam, c):
    return tuple(k for k, on in (("dx", fam.has_dx(c)), ("dw", True), ("db", c["bias"])) if on)


def backward(fam, L, B, c, x, dy_nhwc, packed, legs=None, nan_behind_x=False):
    """<prefix>backward -> {dx NHWC, dw in the layer's layout, db}: every buffer is pre-filled with CANARY and returned whether or not
    its leg ran.  legs: those of the case unless given.  nan_behind_x: the memory that follows x holds NaNs"""
    legs = legs_of(fam, c) if legs is None else legs
    d = desc(fam, c)
    bufs = {"dx": B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), "dw": B.full(fam.w_shape(c), CANARY), "db": B.full(c["cout"], CANARY)}
    ws, nb = workspace(fam, L, B, c)
    x = np.asarray(x, np.float32)
    x_dev = B.put(np.concatenate([x.reshape(-1), np.full(256, np.nan, np.float32)]) if nan_behind_x else x)
    dy_dev = B.put(dy_nhwc)
    L.check(fam.fn(L, "backward")(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), B.ptr(packed),
                                  *[B.ptr(bufs[k]) if k in legs else None for k in ("dx", "dw", "db")], B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


def _run(fam, L, B, name):
    """pack, forward and backward of one case -> (packed, y NHWC, backward's buffers)"""
    c = fam.cases[name]
    (x, w, b, g), _, _ = reference(fam, name)
    packed = pack(fam, L, B, c, w.numpy())
    y = forward(fam, L, B, c, x_layout(fam, c, x), packed, None if b is None else b.numpy())
    return packed, y, backward(fam, L, B, c, x_layout(fam, c, x), nhwc(g), packed)


# ---- the properties both builds are held to (tests/test_*_cpu.py on the emulator, tests/test_gpu_*.py on the device) ----
def check_case(fam, L, B, name):
    """y, dX, dW, db of one case against the fp64 reference, each within the bar; -> {tensor: ratio}"""
    c = fam.cases[name]
    _, r64, e_ref = reference(fam, name)
    _, y, out = _run(fam, L, B, name)
    ratios = {"y": check(f"{name} y", nchw(y), r64["y"], e_ref["y"]), "dw": check(f"{name} dw", out["dw"], r64["dw"], e_ref["dw"])}
    if fam.has_dx(c):
        ratios["dx"] = check(f"{name} dx", nchw(out["dx"]), r64["dx"], e_ref["dx"])
        if name in fam.closed_form_dx:  # a reference of its own: a bug shared with the driver above cannot hide
            ratios["dx_closed"] = check(f"{name} dx (closed form)", nchw(out["dx"]), fam.closed_form_dx[name](name), e_ref["dx"])
    else:
        assert (out["dx"] == CANARY).all()
    if c["bias"]:
        ratios["db"] = check(f"{name} db", out["db"], r64["db"], e_ref["db"])
    else:
        assert (out["db"] == CANARY).all()
    return ratios


def check_two_calls_equal_bits(fam, L, B, name):
    runs = []
    for _ in range(2):
        packed, y, out = _run(fam, L, B, name)
        runs.append([B.get(packed), y] + [out[k] for k in ("dx", "dw", "db")])
    for a, b2 in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b2.view(np.uint32))


def check_null_legs_leave_buffers_alone(fam, L, B, name):
    c = fam.cases[name]
    assert c["bias"]
    (x, w, b, g), _, _ = reference(fam, name)
    packed = pack(fam, L, B, c, w.numpy())
    full = backward(fam, L, B, c, x_layout(fam, c, x), nhwc(g), packed)
    for only in legs_of(fam, c):
        out = backward(fam, L, B, c, x_layout(fam, c, x), nhwc(g), packed, legs=(only,))
        for k in ("dx", "dw", "db"):
            if k == only:
                assert np.array_equal(out[k], full[k]), (only, k)       # a leg does not depend on the others
            else:
                assert (out[k] == CANARY).all(), (only, k)
    assert not any((full[k] == CANARY).all() for k in legs_of(fam, c))


def check_zero_dy_gives_zeros(fam, L, B, name):
    c = fam.cases[name]
    (x, w, b, g), _, _ = reference(fam, name)
    out = backward(fam, L, B, c, x_layout(fam, c, x), np.zeros_like(nhwc(g)), pack(fam, L, B, c, w.numpy()))
    for k in legs_of(fam, c):
        assert (out[k] == 0.0).all(), k


def check_padded_stem_channel(fam, L, B, name):
    """dw of a stem case is the same, bit for bit, when NaNs follow x in memory: the loader never touches the fourth channel"""
    c = fam.cases[name]
    assert fam.x_is_nchw(c) and c["cin"] == 3
    (x, w, b, g), _, _ = reference(fam, name)
    packed = pack(fam, L, B, c, w.numpy())
    plain = backward(fam, L, B, c, x_layout(fam, c, x), nhwc(g), packed, legs=("dw",))["dw"]
    nan = backward(fam, L, B, c, x_layout(fam, c, x), nhwc(g), packed, legs=("dw",), nan_behind_x=True)["dw"]
    assert np.isfinite(plain).all() and np.array_equal(plain.view(np.uint32), nan.view(np.uint32))


def refusal_calls(fam, L, B, name, canaries):
    """forward and backward of one case as closures over a descriptor that return the ABI's status:
    -> (c, fwd(d, x_=, nb_=), bwd(d, dy_=, nb_=, dx_=), x on B, packed, workspace bytes).  bwd asks for dx and dw, never db.  Their
    output buffers y, dx, dw are filled with CANARY and appended to `canaries`"""
    c = fam.cases[name]
    (x, w, b, g), _, _ = reference(fam, name)
    packed = pack(fam, L, B, c, w.numpy())
    ws, nb = workspace(fam, L, B, c)
    x_dev, g_dev = B.put(x_layout(fam, c, x)), B.put(nhwc(g))
    b_dev = None if b is None else B.put(b.numpy())
    y = B.full((c["N"],) + tuple(fam.out_hw(c)) + (c["cout"],), CANARY)
    dx, dw = B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY), B.full(fam.w_shape(c), CANARY)
    canaries.extend([y, dx, dw])

    def fwd(d, x_=x_dev, nb_=nb):
        return fam.fn(L, "forward")(ctypes.byref(d), B.ptr(x_), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb_, B.stream)

    def bwd(d, dy_=g_dev, nb_=nb, dx_=dx):
        return fam.fn(L, "backward")(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_), B.ptr(packed), B.ptr(dx_), B.ptr(dw), None, B.ptr(ws), nb_, B.stream)
    return c, fwd, bwd, x_dev, packed, nb


def check_refusals(fam, L, B, name, bad, bad_pack, stem_name=None):
    """every refusal names its field, and a refused call launches nothing.  bad: (changed fields of the case, word of the message) that
    forward, backward and the size queries refuse; bad_pack: one such pair that the packer refuses too; stem_name: a stem case, which
    also refuses cin = 5 and a dx"""
    canaries = []
    c, fwd, bwd, x_dev, packed, nb = refusal_calls(fam, L, B, name, canaries)
    for over, word in bad:
        d = desc(fam, c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert fam.fn(L, "workspace_bytes")(ctypes.byref(d)) == 0 and fam.fn(L, "wgrad_ranges")(ctypes.byref(d)) == 0
    dp = desc(fam, c, **bad_pack[0])
    assert fam.fn(L, "packed_floats")(ctypes.byref(dp)) == 0
    assert fam.fn(L, "pack_device")(ctypes.byref(dp), B.ptr(x_dev), B.ptr(packed), B.stream) == -1 and bad_pack[1] in L.kpn_last_error()
    d = desc(fam, c)
    assert fwd(d, x_=None) == -1 and b"null" in L.kpn_last_error()
    assert bwd(d, dy_=None) == -1 and b"null" in L.kpn_last_error()
    assert fwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    if stem_name is not None:
        cs, fwd_s, bwd_s, _, _, _ = refusal_calls(fam, L, B, stem_name, canaries)
        ds = desc(fam, cs, cin=5)
        for call in (fwd_s, bwd_s):
            assert call(ds) == -1 and b"cin must" in L.kpn_last_error()
        assert fam.fn(L, "packed_floats")(ctypes.byref(ds)) == 0
        assert bwd_s(desc(fam, cs)) == -1 and b"dx must be NULL" in L.kpn_last_error()
    for buf in canaries:
        assert (B.get(buf) == CANARY).all()                                    # a refused call launches nothing
    assert fwd(d) == 0 and bwd(d) == 0
    if stem_name is not None:
        assert fwd_s(desc(fam, cs)) == 0 and bwd_s(desc(fam, cs), dx_=None) == 0
