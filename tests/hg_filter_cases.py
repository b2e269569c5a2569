"""Test infrastructure of the single-operator HGFilterV2 (kpn_hg_filter_*): the cases, their references and one driver of the C ABI that
runs on host arrays (the emulator build) and on device tensors (the product library) alike.

Cases - the smallest at which the walk can go wrong:
  narrow  the net and inputs of tests/test_gpu_strided.narrow_case(): widths 8 / 16 / 16 / 32, HourGlass(1, 32), 1 x 3 x 16 x 16.  It meets
          the ReLU-margin condition on the reference alone (asserted again in reference()), so it is compared against fp64.
  deep    the same widths with HourGlass(2, 32), N = 2, 3 x 32 x 48: levels 8 x 12, 4 x 6 and 2 x 3 - two recursion levels, two fan-in sums
          inside the HourGlass, a non-square shape, an odd width at the bottom, two images.
  full    (GPU only) tests.encoder_golden.HGFilterV2(), seeded, 1 x 3 x 64 x 64: the shipped widths and depth 4, down to a 1 x 1 level.

References: the CPU fp64 module for `narrow` (both outputs, every parameter gradient, the kept tensors of `state`), with e_ref per tensor
the larger deviation of two CPU fp32 runs (contiguous and channels_last) and the bar of tests/parity.py,
|native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)); and, for every case, the same dataflow composed from the existing entry points -
per_layer() below on the C ABI, install_native_geo(fused_blocks=True) on the GPU - which the operator must equal bit for bit.
"""
import copy
import ctypes
import functools

import numpy as np
import torch

from keypointnerf_amd import lib as kl
from tests import block_cases as bc
from tests import conv_cases as cc
from tests import encoder_golden as eg
from tests import layer_op_checks as loc
from tests import norm_cases as nc
from tests import parity
from tests import resample_cases as rs
from tests import strided_cases as sc
from tests import test_gpu_strided as ts
from tests.parity import CANARY, DeviceArrays, HostArrays, nchw, nhwc  # noqa: F401  (one bar, one pair of array kinds)

EPS = 1e-5
FIELDS = ("in_ch", "c_stem", "c2", "c3", "c4", "depth", "c_hd", "out_ch_hd", "out_ch")
NARROW_W = dict(in_ch=3, c_stem=8, c2=16, c3=16, c4=32, c_hd=8, out_ch_hd=8, out_ch=16)
CASES = {
    "narrow": dict(NARROW_W, depth=1, N=1, H=16, W=16),
    "deep": dict(NARROW_W, depth=2, N=2, H=32, W=48),
    "full": dict(in_ch=3, c_stem=64, c2=128, c3=128, c4=256, depth=4, c_hd=32, out_ch_hd=8, out_ch=64, N=1, H=64, W=64),
}
DEEP_SEED, FULL_SEED = 5, 3


def _deep_net():
    def init(self):
        ts.HGFilterV2.__init__(self)
        self.m0 = eg.HourGlass(2, 32)
    # the class name is what install_native_geo looks for
    return type("HGFilterV2", (ts.HGFilterV2,), {"__init__": init})()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (net (CPU fp32, train mode), x (N, 3, H, W), [g_out, g_x_hd]); made once per case, never modified"""
    c = CASES[name]
    if name == "narrow":
        return ts.narrow_case()
    gen = torch.Generator().manual_seed(900 + len(name))
    if name == "deep":
        net = rs.seed_parameters(_deep_net(), DEEP_SEED)
        x = torch.randn(c["N"], 3, c["H"], c["W"], generator=gen)
    else:
        net = eg.stand_in_geo(FULL_SEED).train()
        x = 2.0 * torch.rand(c["N"], 3, c["H"], c["W"], generator=gen) - 1.0
    gs = [torch.randn(c["N"], c["out_ch"], c["H"] // 4, c["W"] // 4, generator=gen), torch.randn(c["N"], c["out_ch_hd"], c["H"], c["W"], generator=gen)]
    return net, x, gs


def variants():
    """networks install_native_geo(fused=True) must leave on the per-layer path - n_stack = 2, hd = True, one norm with another eps - beside
    `narrow` and `deep`, which it serves: a ModuleDict of fresh copies"""

    def two_stacks(self):
        ts.HGFilterV2.__init__(self)
        self.n_stack = 2
        self.m1, self.top_m_1 = eg.HourGlass(1, 32), eg.ConvBlock(32, 32)
        self.conv_last1, self.bn_end1, self.l1 = torch.nn.Conv2d(32, 32, 1), torch.nn.GroupNorm(32, 32), torch.nn.Conv2d(32, 16, 1)
        self.bl0, self.al0 = torch.nn.Conv2d(32, 32, 1), torch.nn.Conv2d(16, 32, 1)

    def hd(self):
        ts.HGFilterV2.__init__(self)
        self.hd = True

    def other_eps(self):
        ts.HGFilterV2.__init__(self)
        self.m0.b3_1.bn2.eps = 1e-3

    made = {n: type("HGFilterV2", (ts.HGFilterV2,), {"__init__": f})() for n, f in (("stacks", two_stacks), ("hd", hd), ("eps", other_eps))}
    return torch.nn.ModuleDict(dict(made, narrow=copy.deepcopy(case("narrow")[0]), deep=copy.deepcopy(case("deep")[0])))


def cfg_of(c):
    return tuple(c[f] for f in FIELDS)


def blocks_of(net):
    """[(name, ConvBlock)] in tensor order: conv2, conv3, conv4, the HourGlass in dataflow (= module) order, top_m_0"""
    hg = net.m0
    names = ["conv2", "conv3", "conv4"] + [f"m0.b{j}_{k}" for k in range(hg.depth, 0, -1) for j in (1, 2)] + ["m0.b2_plus_1"] + \
            [f"m0.b3_{k}" for k in range(1, hg.depth + 1)] + ["top_m_0"]
    return [(n, net.get_submodule(n)) for n in names]


def tensor_names(net):
    """the parameter names in the tensor order of include/kpnerf.h"""
    out = ["conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias"]
    for n, b in blocks_of(net):
        for i in range(4 if b.downsample is not None else 3):
            out += [f"{n}.bn{i + 1}.weight", f"{n}.bn{i + 1}.bias", f"{n}.conv{i + 1}.weight" if i < 3 else f"{n}.downsample.2.weight"]
    return out + ["unpack1.conv.weight", "unpack1.norm.weight", "unpack1.norm.bias", "conv_out.weight", "conv_out.bias", "conv_last0.weight",
                  "conv_last0.bias", "bn_end0.weight", "bn_end0.bias", "l0.weight", "l0.bias"]


def tensors_of(net):
    p = dict(net.named_parameters())
    return [p[n] for n in tensor_names(net)]


# ---- `state`, from the descriptor alone (include/kpnerf.h, restated) ----
def layout(c):
    """[(name or None, NHWC shape or float count)] in the order of `state`; None: a block's own state or a norm's statistics"""
    N, H, W, depth, c4 = c["N"], c["H"], c["W"], c["depth"], c["c4"]
    h1, w1, h2, w2 = H // 2, W // 2, H // 4, W // 4
    stats = lambda C: (None, 2 * N * C + 2 * N * min(32, C))  # noqa: E731

    def block(cin, cout, h, w):
        return (None, bc.state_floats(dict(N=N, H=h, W=w, cin=cin, cout=cout)))

    out = [("conv1", (N, h1, w1, c["c_stem"])), stats(c["c_stem"]), ("a1", (N, h1, w1, c["c_stem"])), block(c["c_stem"], c["c2"], h1, w1),
           ("conv2", (N, h1, w1, c["c2"])), ("unpack1.conv", (N, H, W, c["c_hd"])), stats(c["c_hd"]), ("p", (N, h2, w2, c["c2"])),
           block(c["c2"], c["c3"], h2, w2), ("conv3", (N, h2, w2, c["c3"])), block(c["c3"], c4, h2, w2), ("conv4", (N, h2, w2, c4))]
    for k in range(depth):                              # level depth - k in the module's names
        h, w, lvl = h2 >> k, w2 >> k, depth - k
        out += [block(c4, c4, h, w), (f"hg{lvl}", (N, h, w, c4)), (f"low{lvl}", (N, h // 2, w // 2, c4)), block(c4, c4, h // 2, w // 2),
                (f"m0.b2_{lvl}", (N, h // 2, w // 2, c4))]
    h, w = h2 >> depth, w2 >> depth
    out += [block(c4, c4, h, w), ("m0.b2_plus_1", (N, h, w, c4))]
    for k in range(depth - 1, -1, -1):
        out.append(block(c4, c4, h2 >> (k + 1), w2 >> (k + 1)))           # b3
    return out + [block(c4, c4, h2, w2), ("top_m_0", (N, h2, w2, c4)), ("conv_last0", (N, h2, w2, c4)), stats(c4)]


def state_floats(c):
    return sum(int(np.prod(s)) for _, s in layout(c))


def state_slices(c, state):
    """the kept tensors as `state` lays them out -> {name: NCHW}"""
    out, o = {}, 0
    for name, s in layout(c):
        n = int(np.prod(s))
        if name is not None:
            out[name] = nchw(state[o:o + n].reshape(s))
        o += n
    assert o == state.size
    return out


def kept_run(net, x, gs, memory_format=torch.contiguous_format):
    """-> {"out", "x_hd", every name of layout(), parameter name: gradient} of the torch module"""
    kept, hooks = {}, []
    depth = net.m0.depth
    watch = {"conv1": "conv1", "conv2": "conv2", "unpack1.conv": "unpack1.conv", "conv3": "conv3", "conv4": "conv4", "m0": f"hg{depth}",
             "top_m_0": "top_m_0", "conv_last0": "conv_last0", "m0.b2_plus_1": "m0.b2_plus_1"}
    watch.update({f"m0.b2_{k}": f"m0.b2_{k}" for k in range(1, depth + 1)})
    for mod, key in watch.items():
        hooks.append(net.get_submodule(mod).register_forward_hook(lambda m, i, o, key=key: kept.__setitem__(key, o.detach().clone())))
    # the input of b2_k is the pooled input of level k; the output of b3_k + the skip is level k's output, the input of b3_{k+1}
    for k in range(1, depth + 1):
        hooks.append(net.get_submodule(f"m0.b2_{k}").register_forward_hook(lambda m, i, o, k=k: kept.__setitem__(f"low{k}", i[0].detach().clone())))
    for k in range(2, depth + 1):
        hooks.append(net.get_submodule(f"m0.b3_{k}").register_forward_hook(lambda m, i, o, k=k: kept.__setitem__(f"hg{k - 1}", i[0].detach().clone())))
    hooks.append(net.conv2.register_forward_hook(lambda m, i, o: kept.__setitem__("a1", i[0].detach().clone())))
    hooks.append(net.conv3.register_forward_hook(lambda m, i, o: kept.__setitem__("p", i[0].detach().clone())))
    out, x_hd = net(x.contiguous(memory_format=memory_format))
    params = dict(net.named_parameters())
    grads = torch.autograd.grad([out, x_hd], list(params.values()), gs, allow_unused=True)
    for h in hooks:
        h.remove()
    res = {"out": out.detach(), "x_hd": x_hd.detach(), **kept}
    res.update({n: g for n, g in zip(params, grads) if g is not None})
    return res


@functools.lru_cache(maxsize=None)
def reference():
    """`narrow` on the CPU in fp64 -> ({tensor: fp64 array}, {tensor: e_ref}); once, shared, read-only.  The ReLU-margin condition is
    asserted first, on the reference alone: the smallest |GroupNorm output| exceeds 8x the largest fp32 deviation of those outputs."""
    net, x, gs = case("narrow")
    margin, e_pre = loc.narrow_margin(net, x, loc.group_norms, ts.NARROW_NORMS)
    print(f"[hg filter narrow] min|GroupNorm output| {margin:.3e} against 8 e_pre = {8 * e_pre:.3e}")
    assert margin > 8.0 * e_pre, (margin, e_pre)
    r64 = kept_run(copy.deepcopy(net).double(), x.double(), [g.double() for g in gs])
    runs32 = [kept_run(copy.deepcopy(net), x, gs, mf) for mf in (torch.contiguous_format, torch.channels_last)]
    e_ref = {k: max(float((r[k].double() - v).abs().max()) for r in runs32) for k, v in r64.items()}
    r64 = {k: v.numpy() for k, v in r64.items()}
    for v in r64.values():
        v.setflags(write=False)
    assert {k for k, _ in layout(CASES["narrow"]) if k} <= set(r64) and set(tensor_names(net)) <= set(r64)
    return r64, e_ref


check = functools.partial(parity.check, tag="hg filter")


# ---- the C ABI ----
def desc(c, **over):
    d = kl.HgFilterDesc()
    v = dict(c, eps=EPS)
    v.update(over)
    for n in ("N", "H", "W") + FIELDS:
        setattr(d, n, int(v[n]))
    d.eps = float(v["eps"])
    return d


def pointers(B, tensors):
    """a host array of the tensors' addresses (None stays NULL)"""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else B.ptr(t).value for t in tensors])


def workspace(L, B, c, fill=0.0):
    nb = L.kpn_hg_filter_workspace_bytes(ctypes.byref(desc(c)))
    assert nb > 0
    return B.full(nb // 4 + 4, fill), nb


class Params:
    """kpn_hg_filter_params of a module on the buffers of B: the tensors in order and the packed weights (kpn_hg_filter_pack_device)"""

    def __init__(self, L, B, c, net):
        d = desc(c)
        ts_ = tensors_of(net)
        assert len(ts_) == L.kpn_hg_filter_tensors(ctypes.byref(d))
        self.tensors = [B.put(t.detach().numpy()) for t in ts_]
        self.shapes = [tuple(t.shape) for t in ts_]
        n = L.kpn_hg_filter_packed_floats(ctypes.byref(d))
        assert n > 0
        self.packed = B.full(n, np.nan)
        self.ptrs = pointers(B, self.tensors)
        L.check(L.kpn_hg_filter_pack_device(ctypes.byref(d), self.ptrs, B.ptr(self.packed), B.stream))
        # the forward and the backward never read a plain convolution weight: those entries are NULL from here on
        self.ptrs = pointers(B, [None if len(s) == 4 else t for t, s in zip(self.tensors, self.shapes)])
        self.struct = kl.HgFilterParams()
        self.struct.tensors = ctypes.cast(self.ptrs, ctypes.POINTER(ctypes.c_void_p))
        self.struct.packed = B.ptr(self.packed).value


def out_shapes(c):
    return (c["N"], c["H"] // 4, c["W"] // 4, c["out_ch"]), (c["N"], c["H"], c["W"], c["out_ch_hd"])


def forward(L, B, c, params, x_nchw, state=None, ws_fill=0.0):
    """kpn_hg_filter_forward -> (out NHWC numpy, x_hd NHWC numpy, state buffer of B)"""
    d = desc(c)
    ns = L.kpn_hg_filter_state_floats(ctypes.byref(d))
    assert ns == state_floats(c)
    so, sh = out_shapes(c)
    out, x_hd = B.full(so, np.nan), B.full(sh, np.nan)
    state = B.full(ns, np.nan) if state is None else state
    ws, nb = workspace(L, B, c, ws_fill)
    x_dev = B.put(x_nchw)
    L.check(L.kpn_hg_filter_forward(ctypes.byref(d), B.ptr(x_dev), ctypes.byref(params.struct), B.ptr(out), B.ptr(x_hd), B.ptr(state), B.ptr(ws), nb,
                                    B.stream))
    return B.get(out), B.get(x_hd), state


def backward(L, B, c, params, x_nchw, d_out, d_x_hd, state, want=None, ws_fill=0.0):
    """kpn_hg_filter_backward -> [array per tensor]: every buffer is pre-filled with CANARY and returned whether or not it was asked for.
    d_out / d_x_hd: NHWC numpy or None.  want: indices of the tensors whose gradient is asked for (default: all)"""
    d = desc(c)
    want = range(len(params.shapes)) if want is None else want
    bufs = [B.full(s, CANARY) for s in params.shapes]
    gptrs = pointers(B, [b if i in want else None for i, b in enumerate(bufs)])
    gr = kl.HgFilterGrads()
    gr.tensors = ctypes.cast(gptrs, ctypes.POINTER(ctypes.c_void_p))
    ws, nb = workspace(L, B, c, ws_fill)
    x_dev = B.put(x_nchw)
    go, gh = (None if g is None else B.put(g) for g in (d_out, d_x_hd))
    L.check(L.kpn_hg_filter_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(go), B.ptr(gh), ctypes.byref(params.struct), B.ptr(state), ctypes.byref(gr),
                                     B.ptr(ws), nb, B.stream))
    return [B.get(b) for b in bufs]


def run(L, B, name, d_out="g", d_x_hd="g", want=None, ws_fill=0.0, state=None):
    """forward + backward of one case through the C ABI -> (out NHWC, x_hd NHWC, state numpy, [gradient per tensor]); "g": the case's own
    output gradient"""
    c = CASES[name]
    net, x, gs = case(name)
    params = Params(L, B, c, net)
    out, x_hd, state = forward(L, B, c, params, x.numpy(), state, ws_fill)
    d_out = nhwc(gs[0]) if isinstance(d_out, str) else d_out
    d_x_hd = nhwc(gs[1]) if isinstance(d_x_hd, str) else d_x_hd
    grads = backward(L, B, c, params, x.numpy(), d_out, d_x_hd, state, want, ws_fill)
    return out, x_hd, B.get(state), grads


@functools.lru_cache(maxsize=None)
def full_run(L, B, name):
    """run(L, B, name) with both output gradients and every gradient asked for; once per build and case, shared, never modified"""
    return run(L, B, name)


# ---- the same dataflow composed from the existing entry points of the C ABI: what install_native_geo(fused_blocks=True) launches ----
def per_layer(L, B, name, d_out="g", d_x_hd="g"):
    """-> (out NHWC, x_hd NHWC, {parameter name: gradient}); the sums where a tensor has two consumers are fp32 numpy adds"""
    c = CASES[name]
    net, x, gs = case(name)
    N, depth, grads = c["N"], c["depth"], {}
    d_out = nhwc(gs[0]) if isinstance(d_out, str) else d_out
    d_x_hd = nhwc(gs[1]) if isinstance(d_x_hd, str) else d_x_hd
    npy = lambda t: t.detach().numpy()  # noqa: E731

    class Conv:
        def __init__(self, mod, m, name, cd):
            self.mod, self.m, self.name, self.cd = mod, m, name, cd
            self.packed = mod.pack(L, B, cd, npy(m.weight))

        def fwd(self, t):
            self.x = t
            return self.mod.forward(L, B, self.cd, t, self.packed, None if self.m.bias is None else npy(self.m.bias))

        def bwd(self, dy):
            r = self.mod.backward(L, B, self.cd, self.x, dy, self.packed)
            grads[f"{self.name}.weight"] = r["dw"]
            if self.m.bias is not None:
                grads[f"{self.name}.bias"] = r["db"]
            return r["dx"]

    class Norm:
        def __init__(self, m, name):
            self.m, self.name = m, name

        def fwd(self, t):
            self.x = t
            self.nd = dict(N=t.shape[0], H=t.shape[1], W=t.shape[2], C=t.shape[3], G=self.m.num_groups, affine=1)
            y, self.stats = nc.forward(L, B, self.nd, 1, t, npy(self.m.weight), npy(self.m.bias))
            return y

        def bwd(self, dy):
            r = nc.backward(L, B, self.nd, 1, self.x, dy, npy(self.m.weight), self.stats)
            grads[f"{self.name}.weight"], grads[f"{self.name}.bias"] = r["dgamma"], r["dbeta"]
            return r["dx"]

    class Block:
        def __init__(self, name):
            self.name, self.m = name, net.get_submodule(name)

        def fwd(self, t):
            self.x = t
            self.c = dict(N=t.shape[0], H=t.shape[1], W=t.shape[2], cin=t.shape[3], cout=2 * self.m.conv1.out_channels)
            self.params = bc.Params(L, B, self.c, self.m)
            y, self.state = bc.forward(L, B, self.c, self.params, t)
            return y

        def bwd(self, dy):
            r = bc.backward(L, B, self.c, self.params, self.x, dy, self.state)
            for key, pn in bc.param_names(self.c).items():
                grads[f"{self.name}.{pn}"] = r[key]
            return r["dx"]

    def res(t):                                          # the low grid of a high tensor t
        return dict(N=t.shape[0], h=t.shape[1] // 2, w=t.shape[2] // 2, C=t.shape[3])

    H, W = c["H"], c["W"]
    conv1 = Conv(sc, net.conv1, "conv1", dict(kind=sc.STEM7, cin=c["in_ch"], cout=c["c_stem"], N=N, H=H, W=W, bias=True))
    bn1, conv2 = Norm(net.bn1, "bn1"), Block("conv2")
    un = Conv(sc, net.unpack1.conv, "unpack1.conv", dict(kind=sc.DECONV3, cin=c["c2"], cout=c["c_hd"], N=N, H=H // 2, W=W // 2, bias=False))
    unn = Norm(net.unpack1.norm, "unpack1.norm")
    co = Conv(cc, net.conv_out, "conv_out", dict(cin=c["c_hd"], cout=c["out_ch_hd"], k=5, pad=2, N=N, H=H, W=W, bias=True))
    conv3, conv4, top = Block("conv3"), Block("conv4"), Block("top_m_0")
    cl = Conv(cc, net.conv_last0, "conv_last0", dict(cin=c["c4"], cout=c["c4"], k=1, pad=0, N=N, H=H // 4, W=W // 4, bias=True))
    bne = Norm(net.bn_end0, "bn_end0")
    l0 = Conv(cc, net.l0, "l0", dict(cin=c["c4"], cout=c["out_ch"], k=1, pad=0, N=N, H=H // 4, W=W // 4, bias=True))
    hgb = {k: {j: Block(f"m0.b{j}_{k}") for j in (1, 2, 3)} for k in range(1, depth + 1)}
    plus = Block("m0.b2_plus_1")

    def hg_fwd(level, inp):
        up1 = hgb[level][1].fwd(inp)
        low = hgb[level][2].fwd(rs.pool_forward(L, B, res(inp), inp))
        low = hg_fwd(level - 1, low) if level > 1 else plus.fwd(low)
        low = hgb[level][3].fwd(low)
        return rs.up_forward(L, B, res(up1), low, up1)

    def hg_bwd(level, dY):
        d_low = hgb[level][3].bwd(rs.up_backward(L, B, res(dY), dY))
        d_low = hg_bwd(level - 1, d_low) if level > 1 else plus.bwd(d_low)
        g_low = hgb[level][2].bwd(d_low)
        return hgb[level][1].bwd(dY) + rs.pool_backward(L, B, res(dY), g_low)            # autograd's add at the fan-out

    x2 = conv2.fwd(bn1.fwd(conv1.fwd(x.numpy())))
    x_hd = co.fwd(unn.fwd(un.fwd(x2)))
    x4 = conv4.fwd(conv3.fwd(rs.pool_forward(L, B, res(x2), x2)))
    out = l0.fwd(bne.fwd(cl.fwd(top.fwd(hg_fwd(depth, x4)))))
    parts = []
    if d_x_hd is not None:
        parts.append(un.bwd(unn.bwd(co.bwd(d_x_hd))))
    if d_out is not None:
        d_p = conv3.bwd(conv4.bwd(hg_bwd(depth, top.bwd(cl.bwd(bne.bwd(l0.bwd(d_out)))))))
        parts.append(rs.pool_backward(L, B, res(x2), d_p))
    d_x2 = parts[0] if len(parts) == 1 else parts[0] + parts[1]
    conv1.x = x.numpy()
    r = sc.backward(L, B, conv1.cd, conv1.x, bn1.bwd(conv2.bwd(d_x2)), conv1.packed, legs=("dw", "db"))
    grads["conv1.weight"], grads["conv1.bias"] = r["dw"], r["db"]
    return out, x_hd, grads


_bits = parity.bits


# ---- the properties both builds are held to (tests/test_hg_filter_cpu.py on the emulator, tests/test_gpu_hg_filter.py on the device) ----
def check_against_fp64(L, B):
    """`narrow`: both outputs, the kept tensors named in `state` and every parameter gradient within the bar"""
    c = CASES["narrow"]
    net = case("narrow")[0]
    r64, e_ref = reference()
    out, x_hd, state, grads = full_run(L, B, "narrow")
    ratios = {"out": check("narrow out", nchw(out), r64["out"], e_ref["out"]), "x_hd": check("narrow x_hd", nchw(x_hd), r64["x_hd"], e_ref["x_hd"])}
    for k, v in state_slices(c, state).items():
        ratios[k] = check(f"narrow state {k}", v, r64[k], e_ref[k])
    for n, g in zip(tensor_names(net), grads):
        ratios[n] = check(f"narrow {n}", g, r64[n], e_ref[n])
    return ratios


def check_per_layer_bits(L, B, name, d_out="g", d_x_hd="g"):
    """out, x_hd and every parameter gradient of the operator have the bits of per_layer(): same kernels, same launch geometry, the same
    fmaf in the lazily normalised loads, and one commutative fp32 add of two finished values at every fan-in"""
    net = case(name)[0]
    out, x_hd, _, grads = full_run(L, B, name) if (d_out, d_x_hd) == ("g", "g") else run(L, B, name, d_out, d_x_hd)
    want_out, want_hd, want = per_layer(L, B, name, d_out, d_x_hd)
    assert np.array_equal(_bits(out), _bits(want_out)) and np.array_equal(_bits(x_hd), _bits(want_hd))
    names = tensor_names(net)
    # what the given output gradients do not reach has no gradient on the per-layer path; the operator writes exact zeros there
    for n, g in zip(names, grads):
        if n in want:
            assert np.array_equal(_bits(g), _bits(want[n])), n
        else:
            assert (g == 0.0).all() and not np.signbit(g).any(), n
    assert set(want) <= set(names) and (len(want) == len(names)) == (d_out is not None and d_x_hd is not None)


def check_two_calls_equal_bits(L, B, name):
    """the second call on a `state` and a workspace full of NaN canaries"""
    c = CASES[name]
    a = full_run(L, B, name)
    b = run(L, B, name, ws_fill=np.nan, state=B.full(state_floats(c), np.nan))
    for u, v in zip([a[0], a[1], a[2]] + a[3], [b[0], b[1], b[2]] + b[3]):
        assert np.array_equal(_bits(u), _bits(v))
    assert all(np.isfinite(g).all() for g in a[3])


def check_image_does_not_depend_on_batch(L, B, name="deep", image=1):
    """one image of the case alone and inside its batch: the outputs and the kept tensors have equal bits"""
    c = CASES[name]
    assert c["N"] > image
    net, x, _ = case(name)
    params = Params(L, B, c, net)
    ob, hb, sb = forward(L, B, c, params, x.numpy())
    c1 = dict(c, N=1)
    o1, h1, s1 = forward(L, B, c1, params, x[image:image + 1].numpy())
    assert np.array_equal(_bits(o1), _bits(ob[image:image + 1])) and np.array_equal(_bits(h1), _bits(hb[image:image + 1]))
    one, batch = state_slices(c1, B.get(s1)), state_slices(c, B.get(sb))
    for k in one:
        assert np.array_equal(_bits(one[k]), _bits(batch[k][image:image + 1])), k


def check_null_grads_leave_buffers_alone(L, B, name):
    net = case(name)[0]
    names = tensor_names(net)
    n = len(names)
    full = full_run(L, B, name)[3]
    ix = names.index
    # the last layer alone; the stem alone (the walk goes all the way down both branches); one per branch; a norm in the middle; nothing
    subsets = [(ix("l0.weight"),), (ix("conv1.weight"),), (ix("unpack1.conv.weight"), ix("m0.b2_plus_1.conv2.weight")), (ix("m0.b3_1.bn2.bias"),), ()]
    for want in subsets:
        got = run(L, B, name, want=want)[3]
        for i in range(n):
            if i in want:
                assert np.array_equal(_bits(got[i]), _bits(full[i])), (want, names[i])     # a gradient does not depend on which others are asked for
            else:
                assert (got[i] == CANARY).all(), (want, names[i])


def check_zero_gradients_give_zeros(L, B, name):
    c = CASES[name]
    so, sh = out_shapes(c)
    grads = run(L, B, name, d_out=np.zeros(so, np.float32), d_x_hd=np.zeros(sh, np.float32))[3]
    for n, g in zip(tensor_names(case(name)[0]), grads):
        assert (g == 0.0).all(), n


def check_bad_descriptors(L, B, name="narrow"):
    c = CASES[name]
    net, x, gs = case(name)
    params = Params(L, B, c, net)
    out0, hd0, state = forward(L, B, c, params, x.numpy())
    ws, nb = workspace(L, B, c)
    so, sh = out_shapes(c)
    x_dev, go, gh = B.put(x.numpy()), B.put(nhwc(gs[0])), B.put(nhwc(gs[1]))
    out, x_hd, scratch = B.full(so, CANARY), B.full(sh, CANARY), B.full(state_floats(c), CANARY)
    bufs = [B.full(s, CANARY) for s in params.shapes]
    gptrs = pointers(B, bufs)
    gr = kl.HgFilterGrads()
    gr.tensors = ctypes.cast(gptrs, ctypes.POINTER(ctypes.c_void_p))

    def fwd(d, nb_=nb):
        return L.kpn_hg_filter_forward(ctypes.byref(d), B.ptr(x_dev), ctypes.byref(params.struct), B.ptr(out), B.ptr(x_hd), B.ptr(scratch), B.ptr(ws),
                                       nb_, B.stream)

    def bwd(d, go_=go, gh_=gh, nb_=nb):
        return L.kpn_hg_filter_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(go_), B.ptr(gh_), ctypes.byref(params.struct), B.ptr(state), ctypes.byref(gr),
                                        B.ptr(ws), nb_, B.stream)

    # odd H / 2; depth = 0; a width of 12; and more of the same kind
    for over, word in ((dict(H=c["H"] + 2), b"divisible"), (dict(W=c["W"] + 1), b"divisible"), (dict(depth=0), b"depth must"), (dict(c2=12), b"ConvBlock"),
                       (dict(c_stem=12), b"c_stem must"), (dict(c4=48), b"ConvBlock"), (dict(c_hd=12), b"c_hd must"), (dict(out_ch=6), b"out_ch must"),
                       (dict(depth=3), b"divisible"), (dict(in_ch=5), b"in_ch must"), (dict(N=0), b"N, H, W"), (dict(eps=0.0), b"eps must"),
                       (dict(H=1 << 15, W=1 << 15), b"below 2^31")):
        d = desc(c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1, over
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_hg_filter_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_hg_filter_state_floats(ctypes.byref(d)) == 0
    d = desc(c)
    assert bwd(d, go_=None, gh_=None) == -1 and b"both null" in L.kpn_last_error()
    assert fwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    bad = desc(c, c2=12)
    assert L.kpn_hg_filter_packed_floats(ctypes.byref(bad)) == 0 and L.kpn_hg_filter_tensors(ctypes.byref(bad)) == 0
    # a refused call launches nothing
    assert all((B.get(v) == CANARY).all() for v in [out, x_hd, scratch] + bufs)
    assert fwd(d) == 0 and bwd(d) == 0
    assert np.array_equal(B.get(out), out0) and np.array_equal(B.get(x_hd), hd0) and not any((B.get(v) == CANARY).all() for v in bufs)
