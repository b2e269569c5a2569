"""Test infrastructure of the single-operator ConvBlock (kpn_conv_block_*): the cases, their fp64 reference, the bar and one driver of
the C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.

Reference: tests.encoder_golden.ConvBlock with seeded weights, seeded normal x and seed gradient g, on the CPU in fp64: y, dX, every
parameter gradient, and the outputs of conv1 and conv2 (what `state` keeps).  A ConvBlock is a chain of seven ops, so e_ref per tensor
is the larger deviation of two CPU fp32 runs from fp64, one contiguous and one channels_last (tests/test_gpu_norm.py).  The bar, for
every element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)) (tests/parity.py).  Every case first asserts, on the
reference alone, that every norm's smallest |pre-activation| exceeds 8 e_ref of that pre-activation: no rounding can flip a ReLU mask.
"""
import copy
import ctypes
import functools

import numpy as np
import torch

from keypointnerf_amd import lib as kl
from tests import conv_cases as cc
from tests import parity
from tests.parity import CANARY, FACTOR, DeviceArrays, HostArrays, nchw, nhwc, ratio  # noqa: F401  (one bar, one pair of array kinds)

EPS = 1e-5
# what each case can catch:
CASES = {
    # the downsample leg; 128 x 32 tiles
    "d16to32": dict(cin=16, cout=32, N=2, H=8, W=8),
    # the identity residual; a ragged pixel tile (120 pixels)
    "i32": dict(cin=32, cout=32, N=2, H=6, W=10),
    # 768 pixels = 48 chunks: three weight-gradient ranges; a wrong rhs_cs or range offset shows here
    "i16_ranges3": dict(cin=16, cout=16, N=3, H=16, W=16),
    # the narrowest legal widths, one channel per group, 35 pixels: less than one 64-row tile, and every border tap
    "d4to16": dict(cin=4, cout=16, N=1, H=5, W=7),
    # the 64 x 64 tile (cout > 32), K = 576
    "d64to128": dict(cin=64, cout=128, N=1, H=4, W=4),
}
SEED_W, SEED_X = 3, 1003


def legs_of(c):
    return 4 if c["cin"] != c["cout"] else 3


def widths(c):
    """(input widths, output widths, kernel sizes) of the legs"""
    n, co = legs_of(c), c["cout"]
    return (c["cin"], co // 2, co // 4, c["cin"])[:n], (co // 2, co // 4, co // 4, co)[:n], (3, 3, 3, 1)[:n]


def block(cin, cout, seed=SEED_W):
    from tests.encoder_golden import ConvBlock
    net = ConvBlock(cin, cout)
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * seed + i)) * (0.3 if p.dim() > 1 else 1.0))
    return net


def leg_modules(net):
    """[(norm, convolution)] per leg"""
    legs = [(net.bn1, net.conv1), (net.bn2, net.conv2), (net.bn3, net.conv3)]
    if net.downsample is not None:
        legs.append((net.bn4, net.downsample[2]))
    return legs


def param_names(c):
    """the parameter of each (leg, kind) as the module names it"""
    names = {}
    for i in range(legs_of(c)):
        names[(i, "dgamma")], names[(i, "dbeta")] = f"bn{i + 1}.weight", f"bn{i + 1}.bias"
        names[(i, "dw")] = f"conv{i + 1}.weight" if i < 3 else "downsample.2.weight"
    return names


def inputs(c, seed=SEED_X):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(c["N"], c["cin"], c["H"], c["W"], generator=gen), torch.randn(c["N"], c["cout"], c["H"], c["W"], generator=gen))


def block_run(net, x, g, memory_format=torch.contiguous_format):
    """-> ({tensor name: value}, {norm name: its output before the in-place ReLU}); "o1" / "o2" are the outputs of conv1 / conv2"""
    pre, kept, hooks = {}, {}, []
    for n in ("bn1", "bn2", "bn3", "bn4"):
        hooks.append(getattr(net, n).register_forward_hook(lambda m, i, o, n=n: pre.__setitem__(n, o.detach().clone())))
    for n, k in (("conv1", "o1"), ("conv2", "o2")):
        hooks.append(getattr(net, n).register_forward_hook(lambda m, i, o, k=k: kept.__setitem__(k, o.detach().clone())))
    x = x.clone().contiguous(memory_format=memory_format).requires_grad_(True)
    y = net(x)
    (y * g).sum().backward()
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), "dx": x.grad, **kept}
    out.update({n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    return out, pre


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (net, x, g, {tensor: fp64 array}, {tensor: e_ref}); computed once per case and shared.  The ReLU-margin condition is
    asserted here, on the reference alone."""
    c = CASES[name]
    net = block(c["cin"], c["cout"])
    x, g = inputs(c)
    r64, pre64 = block_run(copy.deepcopy(net).double(), x.double(), g.double())
    runs32 = [block_run(copy.deepcopy(net), x, g, mf) for mf in (torch.contiguous_format, torch.channels_last)]
    dev_err = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
    assert sorted(pre64) == ["bn1", "bn2", "bn3", "bn4"][:legs_of(c)]
    for n, p in pre64.items():
        e_pre, margin = max(dev_err(r[1][n], p) for r in runs32), float(p.abs().min())
        print(f"[block {name}] {n}: min|pre-activation| {margin:.3e} against 8 e_ref = {8 * e_pre:.3e} ({margin / (8 * e_pre):.1f}x)")
        assert margin > 8.0 * e_pre, (name, n, margin, e_pre)
    e_ref = {k: max(dev_err(r[0][k], v) for r in runs32) for k, v in r64.items()}
    r64 = {k: v.numpy() for k, v in r64.items()}
    for v in r64.values():
        v.setflags(write=False)
    return net, x, g, r64, e_ref


check = functools.partial(parity.check, tag="block")


# ---- the C ABI ----
def desc(c, **over):
    d = kl.ConvBlockDesc()
    v = dict(c, eps=EPS)
    v.update(over)
    for n in ("N", "H", "W", "cin", "cout"):
        setattr(d, n, int(v[n]))
    d.eps = float(v["eps"])
    return d


def state_floats(c):
    """include/kpnerf.h, restated: S (N, H, W, 3 cout / 4), then per leg scale, shift [N][C] and mean, rstd [N][G]"""
    P = c["N"] * c["H"] * c["W"]
    return P * (c["cout"] // 2 + c["cout"] // 4) + sum(2 * c["N"] * C + 2 * c["N"] * min(32, C) for C in widths(c)[0])


def workspace(L, B, c):
    nb = L.kpn_conv_block_workspace_bytes(ctypes.byref(desc(c)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


class Params:
    """kpn_conv_block_params of a module on the buffers of B (the weights packed by kpn_conv2d_pack_device), and what it points to"""

    def __init__(self, L, B, c, net):
        self.keep, self.struct = [], kl.ConvBlockParams()
        win, wout, ks = widths(c)
        for i, (bn, conv) in enumerate(leg_modules(net)):
            gamma, beta = B.put(bn.weight.detach().numpy()), B.put(bn.bias.detach().numpy())
            packed = cc.pack(L, B, dict(N=1, H=1, W=1, cin=win[i], cout=wout[i], k=ks[i], pad=0, bias=False), conv.weight.detach().numpy())
            self.keep += [gamma, beta, packed]
            self.struct.gamma[i], self.struct.beta[i], self.struct.packed[i] = (B.ptr(t).value for t in (gamma, beta, packed))


def forward(L, B, c, params, x_nhwc):
    """kpn_conv_block_forward -> (y NHWC numpy, state buffer of B)"""
    d = desc(c)
    ns = L.kpn_conv_block_state_floats(ctypes.byref(d))
    assert ns == state_floats(c)
    y, state = B.full((c["N"], c["H"], c["W"], c["cout"]), np.nan), B.full(ns, np.nan)
    ws, nb = workspace(L, B, c)
    x_dev = B.put(x_nhwc)
    L.check(L.kpn_conv_block_forward(ctypes.byref(d), B.ptr(x_dev), ctypes.byref(params.struct), B.ptr(y), B.ptr(state), B.ptr(ws), nb, B.stream))
    return B.get(y), state


def all_legs(c):
    return ("dx",) + tuple(sorted(param_names(c)))


def backward(L, B, c, params, x_nhwc, dy_nhwc, state, legs=None):
    """kpn_conv_block_backward -> {"dx": NHWC, (leg, "dgamma" | "dbeta" | "dw"): array}: every buffer is pre-filled with CANARY and
    returned whether or not its leg ran"""
    d = desc(c)
    legs = all_legs(c) if legs is None else legs
    win, wout, ks = widths(c)
    bufs = {"dx": B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY)}
    gr = kl.ConvBlockGrads()
    for i in range(legs_of(c)):
        bufs[(i, "dgamma")], bufs[(i, "dbeta")] = B.full(win[i], CANARY), B.full(win[i], CANARY)
        bufs[(i, "dw")] = B.full((wout[i], win[i], ks[i], ks[i]), CANARY)
        for kind in ("dgamma", "dbeta", "dw"):
            if (i, kind) in legs:
                getattr(gr, kind)[i] = B.ptr(bufs[(i, kind)]).value
    ws, nb = workspace(L, B, c)
    x_dev, dy_dev = B.put(x_nhwc), B.put(dy_nhwc)
    L.check(L.kpn_conv_block_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), ctypes.byref(params.struct), B.ptr(state),
                                      B.ptr(bufs["dx"]) if "dx" in legs else None, ctypes.byref(gr), B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


def run(L, B, name, dy=None, legs=None):
    """forward + backward of one case through the C ABI -> (y NHWC, state numpy, gradients)"""
    c = CASES[name]
    net, x, g, _, _ = reference(name)
    params = Params(L, B, c, net)
    y, state = forward(L, B, c, params, nhwc(x))
    out = backward(L, B, c, params, nhwc(x), nhwc(g) if dy is None else dy, state, legs)
    return y, B.get(state), out


def state_slices(c, state):
    """the outputs of conv1 and conv2 as `state` keeps them -> (o1, o2) NCHW"""
    P, cs = c["N"] * c["H"] * c["W"], c["cout"] // 2 + c["cout"] // 4
    S = state[:P * cs].reshape(c["N"], c["H"], c["W"], cs)
    return nchw(S[..., :c["cout"] // 2]), nchw(S[..., c["cout"] // 2:])


# ---- the properties both builds are held to (tests/test_block_cpu.py on the emulator, tests/test_gpu_block.py on the device) ----
def check_case(L, B, name):
    """y, dX, every parameter gradient and the kept slices of one case against the fp64 reference, each within the bar"""
    c = CASES[name]
    _, _, _, r64, e_ref = reference(name)
    y, state, out = run(L, B, name)
    ratios = {"y": check(f"{name} y", nchw(y), r64["y"], e_ref["y"]), "dx": check(f"{name} dx", nchw(out["dx"]), r64["dx"], e_ref["dx"])}
    for key, pname in param_names(c).items():
        ratios[pname] = check(f"{name} {pname}", out[key], r64[pname], e_ref[pname])
    for k, v in zip(("o1", "o2"), state_slices(c, state)):
        ratios[k] = check(f"{name} state {k}", v, r64[k], e_ref[k])
    assert not any((v == CANARY).all() for v in out.values())
    return ratios


def check_two_calls_equal_bits(L, B, name):
    runs = [run(L, B, name) for _ in range(2)]
    flat = lambda r: [r[0], r[1]] + [r[2][k] for k in all_legs(CASES[name])]  # noqa: E731
    for a, b in zip(flat(runs[0]), flat(runs[1])):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_null_legs_leave_buffers_alone(L, B, name):
    c = CASES[name]
    full = run(L, B, name)[2]
    every = all_legs(c)
    subsets = [("dx",), ((2, "dw"),), ((1, "dgamma"), (1, "dbeta")), ((0, "dbeta"),), ((legs_of(c) - 1, "dw"), (legs_of(c) - 1, "dgamma")), ()]
    for legs in subsets:
        out = run(L, B, name, legs=legs)[2]
        for k in every:
            if k in legs:
                assert np.array_equal(out[k].view(np.uint32), full[k].view(np.uint32)), (legs, k)     # a leg does not depend on the others
            else:
                assert (out[k] == CANARY).all(), (legs, k)


def check_zero_dy_gives_zeros(L, B, name):
    c = CASES[name]
    out = run(L, B, name, dy=np.zeros((c["N"], c["H"], c["W"], c["cout"]), np.float32))[2]
    for k in all_legs(c):
        assert (out[k] == 0.0).all(), k


def check_bad_descriptors(L, B):
    name = "d4to16"
    c = CASES[name]
    net, x, g, _, _ = reference(name)
    params = Params(L, B, c, net)
    y0, state = forward(L, B, c, params, nhwc(x))
    ws, nb = workspace(L, B, c)
    x_dev, g_dev = B.put(nhwc(x)), B.put(nhwc(g))
    y, dx = B.full((c["N"], c["H"], c["W"], c["cout"]), CANARY), B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY)
    scratch = B.full(int(state.shape[0]), CANARY)
    gr = kl.ConvBlockGrads()

    def off4(a):
        """the buffer's address 4 bytes on: misaligned"""
        return ctypes.c_void_p(B.ptr(a).value + 4)

    def fwd(d, x_=None, nb_=nb):
        return L.kpn_conv_block_forward(ctypes.byref(d), B.ptr(x_dev) if x_ is None else x_, ctypes.byref(params.struct), B.ptr(y),
                                        B.ptr(scratch), B.ptr(ws), nb_, B.stream)

    def bwd(d, dy_=None, nb_=nb):
        return L.kpn_conv_block_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(g_dev) if dy_ is None else dy_, ctypes.byref(params.struct),
                                         B.ptr(state), B.ptr(dx), ctypes.byref(gr), B.ptr(ws), nb_, B.stream)

    for over, word in ((dict(cin=12), b"cin must"), (dict(cout=48), b"cout / 2 must"), (dict(cout=8), b"cout / 4 must"), (dict(cout=2048), b"cout must"),
                       (dict(H=0), b"N, H, W"), (dict(eps=0.0), b"eps must"), (dict(N=1 << 16), b"N must"), (dict(H=1 << 14, W=1 << 14), b"below 2^31")):
        d = desc(c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_conv_block_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_conv_block_state_floats(ctypes.byref(d)) == 0
    d = desc(c)
    assert fwd(d, x_=off4(x_dev)) == -1 and b"aligned" in L.kpn_last_error()
    assert bwd(d, dy_=off4(g_dev)) == -1 and b"aligned" in L.kpn_last_error()
    assert fwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    hole = kl.ConvBlockParams.from_buffer_copy(params.struct)
    hole.packed[1] = None
    assert L.kpn_conv_block_forward(ctypes.byref(d), B.ptr(x_dev), ctypes.byref(hole), B.ptr(y), B.ptr(scratch), B.ptr(ws), nb, B.stream) == -1
    assert b"null" in L.kpn_last_error()
    # a refused call launches nothing
    assert all((B.get(v) == CANARY).all() for v in (y, dx, scratch))
    assert fwd(d) == 0 and bwd(d) == 0
    assert np.array_equal(B.get(y), y0) and not (B.get(dx) == CANARY).any()


def check_image_does_not_depend_on_batch(L, B, name, image=1):
    """one image of the case alone and inside its batch: y, the kept slices and dX have equal bits"""
    c = CASES[name]
    assert c["N"] > image
    net, x, g, _, _ = reference(name)
    yb, stateb, outb = run(L, B, name, legs=("dx",))
    c1 = dict(c, N=1)
    params = Params(L, B, c1, net)
    x1, g1 = nhwc(x[image:image + 1]), nhwc(g[image:image + 1])
    y1, state1 = forward(L, B, c1, params, x1)
    dx1 = backward(L, B, c1, params, x1, g1, state1, legs=("dx",))["dx"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(y1), bits(yb[image:image + 1]))
    assert np.array_equal(bits(dx1), bits(outb["dx"][image:image + 1]))
    for a, b in zip(state_slices(c1, B.get(state1)), state_slices(c, stateb)):
        assert np.array_equal(bits(a), bits(b[image:image + 1]))
