"""Test infrastructure of the native GroupNorm / InstanceNorm [+ ReLU] (kpn_group_norm_*): the cases, their fp64 reference, the bar
and one driver of the C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.

Reference: seeded normal x (+ offset), gamma, beta and seed gradient g give y, dX, dgamma, dbeta from
torch.nn.functional.group_norm (+ relu) and torch.autograd.grad on the CPU in fp64.  e_ref is the max deviation of the same
computation in CPU fp32 from that, per tensor.  The bar, for every element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|))
- the project's standing rule and factor (tests/parity.py).  ReLU cases first assert, on the reference alone, that the smallest
|pre-activation| exceeds 8 e_ref(y): no rounding can flip a mask.
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from keypointnerf_amd import lib as kl
from tests import parity
from tests.parity import CANARY, FACTOR, DeviceArrays, HostArrays, nchw, nhwc, ratio  # noqa: F401  (one bar, one pair of array kinds)

EPS = 1e-5
# what each case can catch:
CASES = {
    # 2 threads per pixel and 35 pixels against 128 pixel slots: idle threads enter the reduction; cpg = 2
    "gn4x8_ragged": dict(N=2, C=8, H=5, W=7, G=4, affine=1, offset=0.0),
    # the encoder's bn1 grouping
    "gn32x64": dict(N=1, C=64, H=6, W=6, G=32, affine=1, offset=0.0),
    # 64 threads per pixel, 4 pixel slots, cpg = 8
    "cpg8_256": dict(N=1, C=256, H=4, W=4, G=32, affine=1, offset=0.0),
    # the channel limit: one pixel slot per block
    "c1024": dict(N=1, C=1024, H=2, W=2, G=32, affine=1, offset=0.0),
    # InstanceNorm: G = C, no gamma / beta, NULL dgamma / dbeta
    "in16": dict(N=2, C=16, H=9, W=9, G=16, affine=0, offset=0.0),
    # HW = 768: three chunks per image; three images are summed into dgamma / dbeta; cpg = 1
    "chunks3": dict(N=3, C=32, H=24, W=32, G=32, affine=1, offset=0.0),
    # mean >> std: the B - mean A cancellation
    "offset": dict(N=2, C=32, H=16, W=16, G=32, affine=1, offset=3.0),
}
RELU = (0, 1)


def desc(c, relu_flag, **over):
    d = kl.GroupNormDesc()
    v = dict(c, relu=relu_flag, eps=EPS)
    v.update(over)
    for n in ("N", "H", "W", "C", "G", "affine", "relu"):
        setattr(d, n, int(v[n]))
    d.eps = float(v["eps"])
    return d


def nchunks(c):
    """the chunk rule of include/kpnerf.h, restated"""
    return max(1, min(64, c["H"] * c["W"] // 256))


def inputs(c):
    """x (N, C, H, W) (+ offset), gamma (C), beta (C), g (N, C, H, W): seeded normal, fp32, drawn in this order whatever `affine` says"""
    gen = torch.Generator().manual_seed(1000)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    x = r(c["N"], c["C"], c["H"], c["W"]) + c["offset"]
    gamma, beta = r(c["C"]), r(c["C"])
    return x, gamma, beta, r(c["N"], c["C"], c["H"], c["W"])


def _torch_run(c, relu, x, gamma, beta, g, dtype):
    x = x.clone().to(dtype).requires_grad_(True)
    wb = [t.clone().to(dtype).requires_grad_(True) for t in (gamma, beta)] if c["affine"] else [None, None]
    pre = F.group_norm(x, c["G"], wb[0], wb[1], EPS)
    y = F.relu(pre) if relu else pre
    grads = torch.autograd.grad(y, [x] + (wb if c["affine"] else []), g.to(dtype))
    out = {"y": y.detach(), "dx": grads[0], "pre": pre.detach()}
    if c["affine"]:
        out["dgamma"], out["dbeta"] = grads[1], grads[2]
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name, relu):
    """-> (inputs, {tensor: fp64 array}, {tensor: e_ref}); computed once per (case, relu) and shared.  For ReLU cases the input
    condition is asserted here, on the reference alone."""
    c = CASES[name]
    x, gamma, beta, g = inputs(c)
    r64, r32 = (_torch_run(c, relu, x, gamma, beta, g, dt) for dt in (torch.float64, torch.float32))
    e_ref = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64}
    if relu:
        margin = float(np.abs(r64["pre"]).min())
        assert margin > 8.0 * e_ref["y"], (name, margin, e_ref["y"])
    for v in r64.values():
        v.setflags(write=False)
    return (x, gamma, beta, g), r64, e_ref


check = functools.partial(parity.check, tag="norm")


def workspace(L, B, c, relu=0):
    nb = L.kpn_group_norm_workspace_bytes(ctypes.byref(desc(c, relu)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


def forward(L, B, c, relu, x_nhwc, gamma, beta):
    """kpn_group_norm_forward -> (y NHWC numpy, stats buffer of B)"""
    d = desc(c, relu)
    ns = L.kpn_group_norm_stats_floats(ctypes.byref(d))
    assert ns == 2 * c["N"] * c["C"] + 2 * c["N"] * c["G"]
    y, stats = B.full((c["N"], c["H"], c["W"], c["C"]), np.nan), B.full(ns, np.nan)
    ws, nb = workspace(L, B, c, relu)
    x_dev = B.put(x_nhwc)
    gb = [B.put(t) for t in (gamma, beta)] if c["affine"] else [None, None]
    L.check(L.kpn_group_norm_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(gb[0]), B.ptr(gb[1]), B.ptr(y), B.ptr(stats), B.ptr(ws), nb, B.stream))
    return B.get(y), stats


def backward(L, B, c, relu, x_nhwc, dy_nhwc, gamma, stats, legs=("dx", "dgamma", "dbeta")):
    """kpn_group_norm_backward -> {dx NHWC, dgamma, dbeta}: every buffer is pre-filled with CANARY and returned whether or not its leg ran"""
    d = desc(c, relu)
    bufs = {"dx": B.full((c["N"], c["H"], c["W"], c["C"]), CANARY), "dgamma": B.full(c["C"], CANARY), "dbeta": B.full(c["C"], CANARY)}
    ws, nb = workspace(L, B, c, relu)
    x_dev, dy_dev = B.put(x_nhwc), B.put(dy_nhwc)
    g_dev = B.put(gamma) if c["affine"] else None
    L.check(L.kpn_group_norm_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), B.ptr(g_dev), B.ptr(stats),
                                      *[B.ptr(bufs[k]) if k in legs else None for k in ("dx", "dgamma", "dbeta")], B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


def legs_of(c):
    return ("dx", "dgamma", "dbeta") if c["affine"] else ("dx",)


def run(L, B, name, relu, dy=None, legs=None):
    """forward + backward of one case through the C ABI -> (y NHWC, stats numpy, {dx NHWC, dgamma, dbeta})"""
    c = CASES[name]
    (x, gamma, beta, g), _, _ = reference(name, relu)
    y, stats = forward(L, B, c, relu, nhwc(x), gamma.numpy(), beta.numpy())
    out = backward(L, B, c, relu, nhwc(x), nhwc(g) if dy is None else dy, gamma.numpy(), stats, legs_of(c) if legs is None else legs)
    return y, B.get(stats), out


# ---- the properties both builds are held to (tests/test_norm_cpu.py on the emulator, tests/test_gpu_norm.py on the device) ----
def check_case(L, B, name, relu):
    """y, dX, dgamma, dbeta of one case against the fp64 reference, each within the bar; -> {tensor: ratio}"""
    c = CASES[name]
    _, r64, e_ref = reference(name, relu)
    y, _, out = run(L, B, name, relu)
    tag = f"{name} relu={relu}"
    ratios = {"y": check(f"{tag} y", nchw(y), r64["y"], e_ref["y"]), "dx": check(f"{tag} dx", nchw(out["dx"]), r64["dx"], e_ref["dx"])}
    for k in ("dgamma", "dbeta"):
        if c["affine"]:
            ratios[k] = check(f"{tag} {k}", out[k], r64[k], e_ref[k])
        else:
            assert (out[k] == CANARY).all()
    return ratios


def check_stats_buffer(L, B, name):
    """scale [N][C], shift [N][C], mean [N][G], rstd [N][G]: the fp64 statistics (biased variance, eps as the fp32 the descriptor
    holds), folded in fp64 and rounded once.  The kernel adds in chunk / thread order and numpy pairwise: the two fp64 sums differ by
    about 1e-16 relative, which moves a rounding to fp32 (6e-8) only on a tie - so each entry is within one fp32 spacing, not more."""
    c = CASES[name]
    (x, gamma, beta, _), _, _ = reference(name, 0)
    _, stats, _ = run(L, B, name, 0)
    N, C, G = c["N"], c["C"], c["G"]
    xg = x.numpy().astype(np.float64).reshape(N, G, -1)
    mean = xg.mean(-1)
    var = (xg * xg).mean(-1) - mean * mean
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(EPS)))
    cpg = C // G
    gm = gamma.numpy().astype(np.float64) if c["affine"] else np.ones(C)
    bt = beta.numpy().astype(np.float64) if c["affine"] else np.zeros(C)
    scale = gm[None] * np.repeat(rstd, cpg, 1)
    shift = bt[None] - np.repeat(mean, cpg, 1) * scale
    want = np.concatenate([v.reshape(-1) for v in (scale, shift, mean, rstd)])
    assert stats.size == want.size == 2 * N * C + 2 * N * G
    w32 = want.astype(np.float32)
    assert (np.abs(stats.astype(np.float64) - w32) <= np.spacing(np.abs(w32))).all()
    assert (stats == w32).mean() > 0.99


def check_two_calls_equal_bits(L, B, name, relu=1):
    runs = [run(L, B, name, relu) for _ in range(2)]
    for a, b in zip(*[[r[0], r[1], r[2]["dx"], r[2]["dgamma"], r[2]["dbeta"]] for r in runs]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_null_legs_leave_buffers_alone(L, B, name, relu=1):
    assert CASES[name]["affine"]
    full = run(L, B, name, relu)[2]
    for only in ("dx", "dgamma", "dbeta"):
        out = run(L, B, name, relu, legs=(only,))[2]
        for k in ("dx", "dgamma", "dbeta"):
            if k == only:
                assert np.array_equal(out[k], full[k]), (only, k)       # a leg does not depend on the others
            else:
                assert (out[k] == CANARY).all(), (only, k)
    assert not any((full[k] == CANARY).any() for k in full)
    none = run(L, B, name, relu, legs=())[2]
    assert all((v == CANARY).all() for v in none.values())


def check_zero_dy_gives_zeros(L, B, name, relu=1):
    c = CASES[name]
    out = run(L, B, name, relu, dy=np.zeros((c["N"], c["H"], c["W"], c["C"]), np.float32))[2]
    for k in legs_of(c):
        assert (out[k] == 0.0).all(), k


def check_bad_descriptors(L, B):
    name, relu = "gn4x8_ragged", 1
    c = CASES[name]
    (x, gamma, beta, g), _, _ = reference(name, relu)
    y0, stats = forward(L, B, c, relu, nhwc(x), gamma.numpy(), beta.numpy())
    ws, nb = workspace(L, B, c)
    x_dev, g_dev, gm, bt = B.put(nhwc(x)), B.put(nhwc(g)), B.put(gamma.numpy()), B.put(beta.numpy())
    shape = (c["N"], c["H"], c["W"], c["C"])
    y, dx, dgm = B.full(shape, CANARY), B.full(shape, CANARY), B.full(c["C"], CANARY)
    scratch = B.full(int(stats.shape[0]), CANARY)

    def off4(a):
        """the buffer's address 4 bytes on: misaligned"""
        return ctypes.c_void_p(B.ptr(a).value + 4)

    def fwd(d, x_=None, gamma_=None, nb_=nb):
        return L.kpn_group_norm_forward(ctypes.byref(d), B.ptr(x_dev) if x_ is None else x_, B.ptr(gm) if gamma_ is None else gamma_[0],
                                        B.ptr(bt), B.ptr(y), B.ptr(scratch), B.ptr(ws), nb_, B.stream)

    def bwd(d, dy_=None, gamma_=None, dgamma_=None, nb_=nb):
        return L.kpn_group_norm_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(g_dev) if dy_ is None else dy_,
                                         B.ptr(gm) if gamma_ is None else gamma_[0], B.ptr(stats), B.ptr(dx), dgamma_, None, B.ptr(ws), nb_, B.stream)

    for over, word in ((dict(C=12, G=4), b"C must"), (dict(G=3), b"G must"), (dict(eps=0.0), b"eps must"), (dict(H=0), b"N, H, W"),
                       (dict(relu=2), b"relu must"), (dict(affine=2), b"affine must")):
        d = desc(c, relu, **over)
        for call in (fwd, bwd):
            assert call(d) == -1
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_group_norm_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_group_norm_stats_floats(ctypes.byref(d)) == 0
    d = desc(c, relu)
    for call in (fwd, bwd):
        assert call(d, gamma_=[None]) == -1 and b"gamma" in L.kpn_last_error()             # gamma missing under affine
    d0 = desc(c, relu, affine=0)
    assert bwd(d0, gamma_=[None], dgamma_=B.ptr(dgm)) == -1 and b"dgamma" in L.kpn_last_error()     # dgamma under affine = 0
    assert fwd(d, x_=off4(x_dev)) == -1 and b"aligned" in L.kpn_last_error()
    assert bwd(d, dy_=off4(g_dev)) == -1 and b"aligned" in L.kpn_last_error()
    assert fwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    # a refused call launches nothing
    assert all((B.get(v) == CANARY).all() for v in (y, dx, dgm, scratch))
    assert fwd(d) == 0 and bwd(d, dgamma_=B.ptr(dgm)) == 0
    assert np.array_equal(B.get(y), y0) and not (B.get(dx) == CANARY).any() and not (B.get(dgm) == CANARY).any()


def check_workspace_covers_partials(L):
    """the workspace query is at least the fp64 (A, B) partials per (image, chunk, channel) and the three coefficient vectors"""
    c = CASES["chunks3"]
    assert nchunks(c) == 3
    nb = L.kpn_group_norm_workspace_bytes(ctypes.byref(desc(c, 1)))
    assert nb >= c["N"] * 3 * c["C"] * 2 * 8 + 3 * c["N"] * c["C"] * 4
