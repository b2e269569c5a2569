"""Test infrastructure of the single-operator ResBlkEncoder (kpn_res_encoder_*): the cases, their fp64 reference, the bar and one driver
of the C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.

Reference: tests.encoder_golden.ResBlkEncoder made with eg.seeded(..., seed).train(), a seeded normal x (seed 72) and seed gradient g
(seed 73), on the CPU in fp64: y, every parameter gradient, every convolution output c_i and every a_k (what `state` keeps).  e_ref per
tensor is the larger deviation of two CPU fp32 runs from fp64, one contiguous and one channels_last.  The bar, for every element:
|native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)) (tests/parity.py).  Every case first asserts, on the reference alone, that
the smallest |InstanceNorm output| in front of a ReLU exceeds 8x the largest fp32 deviation of those outputs: no rounding can flip a
ReLU mask (the check of tests/test_gpu_reppad.narrow_margin, over every norm of the case).
"""
import copy
import ctypes
import functools

import numpy as np
import torch
import torch.nn as nn

from keypointnerf_amd import lib as kl
from tests import encoder_golden as eg
from tests import layer_op_checks as loc
from tests import norm_cases as nc
from tests import reppad_cases as rc
from tests import strided_cases as sc
from tests import parity
from tests import test_gpu_reppad as tr
from tests.parity import CANARY, FACTOR, DeviceArrays, HostArrays, nchw, nhwc, ratio  # noqa: F401  (one bar, one pair of array kinds)

EPS = 1e-5
SEED_X, SEED_G = 72, 73
# what each case can catch:
CASES = {
    # tests/test_gpu_reppad.narrow_case: every pixel of the blocks is a ring pixel (3 x 2); two chained residual gradients; the upsample
    # reads a materialised source
    "narrow": dict(out_ch=4, ngf=4, n_down=2, n_blocks=2, n_up=1, N=2, H=12, W=8, seed=tr.NARROW_SEED),
    # the second transposed convolution's weight gradient reads R through the rhs_ss load; the 7x7 output layer reads a lazily normalised
    # source
    "up2": dict(out_ch=4, ngf=4, n_down=2, n_blocks=1, n_up=2, N=1, H=16, W=16, seed=1),
    # a_0 feeds the transposed convolution directly; no block legs
    "noblocks": dict(out_ch=8, ngf=8, n_down=1, n_blocks=0, n_up=1, N=2, H=8, W=12, seed=2),
    # 3072 stem pixels and 768 block pixels: several weight-gradient ranges and split K; a wrong range offset or image index shows here
    # (seeds 1 and 7 miss the margin condition)
    "ranges": dict(out_ch=4, ngf=4, n_down=1, n_blocks=1, n_up=1, N=3, H=32, W=32, seed=2),
}
IN_CH = 3


def layers_of(c):
    """[(kind, cin, cout, k, Ho, Wo)] in module order: include/kpnerf.h, restated"""
    out, C, h, w = [("stem", IN_CH, c["ngf"], 7, c["H"], c["W"])], c["ngf"], c["H"], c["W"]
    for _ in range(c["n_down"]):
        C, h, w = 2 * C, h // 2, w // 2
        out.append(("down", C // 2, C, 3, h, w))
    out += [("res", C, C, 3, h, w)] * (2 * c["n_blocks"])
    for _ in range(c["n_up"]):
        C, h, w = C // 2, 2 * h, 2 * w
        out.append(("up", 2 * C, C, 3, h, w))
    out.append(("out", C, c["out_ch"], 7, h, w))
    return out


def block_shape(c):
    f = 1 << c["n_down"]
    return c["N"], c["H"] // f, c["W"] // f, c["ngf"] * f


def state_floats(c):
    """sum numel(c_i) + sum numel(a_k) + 4 N sum C_norm, from the descriptor"""
    ls = layers_of(c)[:-1]
    return (sum(c["N"] * h * w * co for _, _, co, _, h, w in ls) + (c["n_blocks"] + 1) * int(np.prod(block_shape(c)))
            + 4 * c["N"] * sum(co for _, _, co, _, _, _ in ls))


def w_shape(layer):
    kind, cin, cout, k, _, _ = layer
    return (cin, cout, k, k) if kind == "up" else (cout, cin, k, k)


def encoder(c):
    return eg.seeded(eg.ResBlkEncoder(out_ch=c["out_ch"], ngf=c["ngf"], n_downsample=c["n_down"], n_blocks=c["n_blocks"],
                                      n_upsample=c["n_up"]), c["seed"]).train()


def convs_of(net):
    """the convolutions in module order: the layers of the descriptor"""
    return [m for m in net.modules() if type(m) in (nn.Conv2d, nn.ConvTranspose2d)]


def param_names(net):
    """[(weight name, bias name)] per layer"""
    return [(f"{n}.weight", f"{n}.bias") for n, m in net.named_modules() if type(m) in (nn.Conv2d, nn.ConvTranspose2d)]


def inputs(c):
    f = 1 << (c["n_down"] - c["n_up"])
    return (torch.randn(c["N"], IN_CH, c["H"], c["W"], generator=torch.Generator().manual_seed(SEED_X)),
            torch.randn(c["N"], c["out_ch"], c["H"] // f, c["W"] // f, generator=torch.Generator().manual_seed(SEED_G)))


def encoder_run(net, c, x, g, memory_format=torch.contiguous_format):
    """-> {"y", "c0" .. (every convolution output but y), "a0" .. "a{n_blocks}", parameter name: gradient}"""
    kept, hooks = {}, []
    for i, m in enumerate(convs_of(net)[:-1]):
        hooks.append(m.register_forward_hook(lambda m, i_, o, i=i: kept.__setitem__(f"c{i}", o.detach().clone())))
    a0 = net.layers[3 + 3 * c["n_down"]]                  # the ReLU behind the last stride-2 layer's norm
    assert isinstance(a0, nn.ReLU)
    hooks.append(a0.register_forward_hook(lambda m, i_, o: kept.__setitem__("a0", o.detach().clone())))
    blocks = [m for m in net.layers if type(m).__name__ == "ResBlk"]
    for k, m in enumerate(blocks):
        hooks.append(m.register_forward_hook(lambda m, i_, o, k=k: kept.__setitem__(f"a{k + 1}", o.detach().clone())))
    y = net(x.contiguous(memory_format=memory_format))
    params = dict(net.named_parameters())
    grads = torch.autograd.grad([y], list(params.values()), [g])
    for h in hooks:
        h.remove()
    out = {"y": y.detach(), **kept}
    out.update(dict(zip(params, grads)))
    return out


def margin(net, x):
    """(smallest |InstanceNorm output| in front of a ReLU of the fp64 module, largest fp32 deviation of those outputs over both memory
    formats): tests/test_gpu_reppad.narrow_margin over every norm of this encoder"""
    pre64 = loc.norm_outputs(copy.deepcopy(net).double(), x.double(), torch.contiguous_format, tr.relu_norms)
    pre32 = [loc.norm_outputs(copy.deepcopy(net), x, mf, tr.relu_norms) for mf in (torch.contiguous_format, torch.channels_last)]
    return (min(float(p.abs().min()) for p in pre64.values()), max(float((r[n].double() - p).abs().max()) for r in pre32 for n, p in pre64.items()),
            len(pre64))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (net, x, g, {tensor: fp64 array}, {tensor: e_ref}); computed once per case and shared.  The ReLU-margin condition is asserted
    here, on the reference alone."""
    c = CASES[name]
    net = tr.narrow_case()[0] if name == "narrow" else encoder(c)
    x, g = inputs(c)
    if name == "narrow":
        _, x0, g0 = tr.narrow_case()
        assert torch.equal(x, x0) and torch.equal(g, g0)
    m, e_pre, norms = margin(net, x)
    assert norms == 1 + c["n_down"] + c["n_blocks"] + c["n_up"]
    print(f"[res encoder {name}] min|InstanceNorm output| {m:.3e} against 8 e_pre = {8 * e_pre:.3e} ({m / (8 * e_pre):.1f}x, {norms} norms)")
    assert m > 8.0 * e_pre, (name, m, e_pre)
    r64 = encoder_run(copy.deepcopy(net).double(), c, x.double(), g.double())
    runs32 = [encoder_run(copy.deepcopy(net), c, x, g, mf) for mf in (torch.contiguous_format, torch.channels_last)]
    e_ref = {k: max(float((r[k].double() - v).abs().max()) for r in runs32) for k, v in r64.items()}
    r64 = {k: v.numpy() for k, v in r64.items()}
    for v in r64.values():
        v.setflags(write=False)
    return net, x, g, r64, e_ref


check = functools.partial(parity.check, tag="res encoder")


# ---- the C ABI ----
def desc(c, **over):
    d = kl.ResEncoderDesc()
    v = dict(c, eps=EPS, in_ch=IN_CH)
    v.update(over)
    for n in ("N", "H", "W", "in_ch", "ngf", "n_down", "n_blocks", "n_up", "out_ch"):
        setattr(d, n, int(v[n]))
    d.eps = float(v["eps"])
    return d


def pointers(B, tensors):
    """a host array of the tensors' addresses (None stays NULL)"""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else B.ptr(t).value for t in tensors])


def workspace(L, B, c):
    nb = L.kpn_res_encoder_workspace_bytes(ctypes.byref(desc(c)))
    assert nb > 0
    return B.full(nb // 4 + 4, 0.0), nb


class Params:
    """the packed weights (kpn_res_encoder_pack_device) and the biases of a module on the buffers of B"""

    def __init__(self, L, B, c, net):
        d = desc(c)
        convs = convs_of(net)
        assert len(convs) == L.kpn_res_encoder_layers(ctypes.byref(d)) == len(layers_of(c))
        assert [tuple(m.weight.shape) for m in convs] == [w_shape(l) for l in layers_of(c)]
        self.weights = [B.put(m.weight.detach().numpy()) for m in convs]
        self.bias = [B.put(m.bias.detach().numpy()) for m in convs]
        n = L.kpn_res_encoder_packed_floats(ctypes.byref(d))
        assert n > 0
        self.packed = B.full(n, np.nan)
        L.check(L.kpn_res_encoder_pack_device(ctypes.byref(d), pointers(B, self.weights), B.ptr(self.packed), B.stream))
        self.bias_ptrs = pointers(B, self.bias)


def y_shape(c):
    _, _, _, _, h, w = layers_of(c)[-1]
    return c["N"], h, w, c["out_ch"]


def forward(L, B, c, params, x_nchw):
    """kpn_res_encoder_forward -> (y NHWC numpy, state buffer of B)"""
    d = desc(c)
    ns = L.kpn_res_encoder_state_floats(ctypes.byref(d))
    assert ns == state_floats(c)
    y, state = B.full(y_shape(c), np.nan), B.full(ns, np.nan)
    ws, nb = workspace(L, B, c)
    x_dev = B.put(x_nchw)
    L.check(L.kpn_res_encoder_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(params.packed), params.bias_ptrs, B.ptr(y), B.ptr(state), B.ptr(ws),
                                      nb, B.stream))
    return B.get(y), state


def all_grads(c):
    return tuple((i, kind) for i in range(len(layers_of(c))) for kind in ("dw", "db"))


def backward(L, B, c, params, x_nchw, dy_nhwc, state, want=None):
    """kpn_res_encoder_backward -> {(layer, "dw" | "db"): array}: every buffer is pre-filled with CANARY and returned whether or not it
    was asked for"""
    d = desc(c)
    want = all_grads(c) if want is None else want
    ls = layers_of(c)
    bufs = {}
    for i, l in enumerate(ls):
        bufs[(i, "dw")], bufs[(i, "db")] = B.full(w_shape(l), CANARY), B.full(l[2], CANARY)
    dw = pointers(B, [bufs[(i, "dw")] if (i, "dw") in want else None for i in range(len(ls))])
    db = pointers(B, [bufs[(i, "db")] if (i, "db") in want else None for i in range(len(ls))])
    ws, nb = workspace(L, B, c)
    x_dev, dy_dev = B.put(x_nchw), B.put(dy_nhwc)
    L.check(L.kpn_res_encoder_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(dy_dev), B.ptr(params.packed), B.ptr(state), dw, db, B.ptr(ws), nb,
                                       B.stream))
    return {k: B.get(v) for k, v in bufs.items()}


def run(L, B, name, dy=None, want=None):
    """forward + backward of one case through the C ABI -> (y NHWC, state numpy, gradients)"""
    c = CASES[name]
    net, x, g, _, _ = reference(name)
    params = Params(L, B, c, net)
    y, state = forward(L, B, c, params, x.numpy())
    out = backward(L, B, c, params, x.numpy(), nhwc(g) if dy is None else dy, state, want)
    return y, B.get(state), out


def state_slices(c, state):
    """the kept tensors as `state` lays them out -> {"c0" ..: NCHW, "a0" ..: NCHW}"""
    out, o = {}, 0
    for i, (_, _, co, _, h, w) in enumerate(layers_of(c)[:-1]):
        n = c["N"] * h * w * co
        out[f"c{i}"] = nchw(state[o:o + n].reshape(c["N"], h, w, co))
        o += n
    shape = block_shape(c)
    for k in range(c["n_blocks"] + 1):
        n = int(np.prod(shape))
        out[f"a{k}"] = nchw(state[o:o + n].reshape(shape))
        o += n
    assert o + 4 * c["N"] * sum(l[2] for l in layers_of(c)[:-1]) == state.size
    return out


# ---- the properties both builds are held to (tests/test_res_encoder_cpu.py on the emulator, tests/test_gpu_res_encoder.py on the device) ----
def check_case(L, B, name):
    """y, the kept slices and every parameter gradient of one case against the fp64 reference, each within the bar; the biases in front
    of a norm get exact zeros"""
    c = CASES[name]
    net, _, _, r64, e_ref = reference(name)
    y, state, out = run(L, B, name)
    ratios = {"y": check(f"{name} y", nchw(y), r64["y"], e_ref["y"])}
    for k, v in state_slices(c, state).items():
        ratios[k] = check(f"{name} state {k}", v, r64[k], e_ref[k])
    names = param_names(net)
    for i, (wn, bn) in enumerate(names):
        ratios[wn] = check(f"{name} {wn}", out[(i, "dw")], r64[wn], e_ref[wn])
        ratios[bn] = check(f"{name} {bn}", out[(i, "db")], r64[bn], e_ref[bn])
        if i < len(names) - 1:
            assert (out[(i, "db")] == 0.0).all() and not np.signbit(out[(i, "db")]).any(), bn
    assert not (out[(len(names) - 1, "db")] == 0.0).all()
    return ratios


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_two_calls_equal_bits(L, B, name):
    runs = [run(L, B, name) for _ in range(2)]
    flat = lambda r: [r[0], r[1]] + [r[2][k] for k in all_grads(CASES[name])]  # noqa: E731
    for a, b in zip(flat(runs[0]), flat(runs[1])):
        assert np.array_equal(_bits(a), _bits(b))


def check_null_grads_leave_buffers_alone(L, B, name):
    c = CASES[name]
    n = len(layers_of(c))
    full = run(L, B, name)[2]
    every = all_grads(c)
    subsets = [((n - 1, "dw"),), ((n - 1, "db"),), ((0, "dw"),), ((1, "dw"), (n - 2, "dw")), ((1, "db"), (n - 2, "dw")), ((n // 2, "dw"), (0, "db")), ()]
    for want in subsets:
        out = run(L, B, name, want=want)[2]
        for k in every:
            if k in want:
                assert np.array_equal(_bits(out[k]), _bits(full[k])), (want, k)     # a gradient does not depend on which others are asked for
            else:
                assert (out[k] == CANARY).all(), (want, k)


def check_zero_dy_gives_zeros(L, B, name):
    c = CASES[name]
    out = run(L, B, name, dy=np.zeros(y_shape(c), np.float32))[2]
    for k in all_grads(c):
        assert (out[k] == 0.0).all(), k


def check_image_does_not_depend_on_batch(L, B, name, image=1):
    """one image of the case alone and inside its batch: y and the kept slices have equal bits"""
    c = CASES[name]
    assert c["N"] > image
    net, x, _, _, _ = reference(name)
    params = Params(L, B, c, net)
    yb, stateb = forward(L, B, c, params, x.numpy())
    c1 = dict(c, N=1)
    y1, state1 = forward(L, B, c1, params, x[image:image + 1].numpy())
    assert np.array_equal(_bits(y1), _bits(yb[image:image + 1]))
    one, batch = state_slices(c1, B.get(state1)), state_slices(c, B.get(stateb))
    for k in one:
        assert np.array_equal(_bits(one[k]), _bits(batch[k][image:image + 1])), k


def check_bad_descriptors(L, B, name="noblocks"):
    c = CASES[name]
    net, x, g, _, _ = reference(name)
    params = Params(L, B, c, net)
    y0, state = forward(L, B, c, params, x.numpy())
    ws, nb = workspace(L, B, c)
    x_dev, g_dev = B.put(x.numpy()), B.put(nhwc(g))
    y, scratch = B.full(y_shape(c), CANARY), B.full(int(state.shape[0]), CANARY)
    ls = layers_of(c)
    grads = [B.full(w_shape(l), CANARY) for l in ls] + [B.full(l[2], CANARY) for l in ls]
    dw, db = pointers(B, grads[:len(ls)]), pointers(B, grads[len(ls):])

    def off4(a):
        """the buffer's address 4 bytes on: misaligned"""
        return ctypes.c_void_p(B.ptr(a).value + 4)

    def fwd(d, y_=None, nb_=nb):
        return L.kpn_res_encoder_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(params.packed), params.bias_ptrs, B.ptr(y) if y_ is None else y_,
                                         B.ptr(scratch), B.ptr(ws), nb_, B.stream)

    def bwd(d, dy_=None, nb_=nb):
        return L.kpn_res_encoder_backward(ctypes.byref(d), B.ptr(x_dev), B.ptr(g_dev) if dy_ is None else dy_, B.ptr(params.packed), B.ptr(state),
                                          dw, db, B.ptr(ws), nb_, B.stream)

    for over, word in ((dict(ngf=12), b"ngf must"), (dict(ngf=2), b"ngf must"), (dict(n_up=0), b"n_up must be at least"), (dict(n_up=2), b"n_up must be at most"),
                       (dict(out_ch=6), b"out_ch must"), (dict(H=c["H"] + 1), b"divisible"), (dict(W=c["W"] + 1), b"divisible"),
                       (dict(ngf=1024), b"ngf << n_down"), (dict(in_ch=5), b"in_ch must"), (dict(n_blocks=-1), b"n_blocks must"),
                       (dict(N=0), b"N, H, W"), (dict(N=1 << 16), b"N must"), (dict(eps=0.0), b"eps must"), (dict(H=1 << 15, W=1 << 15), b"below 2^31")):
        d = desc(c, **over)
        for call in (fwd, bwd):
            assert call(d) == -1, over
            assert word in L.kpn_last_error(), (over, L.kpn_last_error())
        assert L.kpn_res_encoder_workspace_bytes(ctypes.byref(d)) == 0 and L.kpn_res_encoder_state_floats(ctypes.byref(d)) == 0
    d = desc(c)
    assert fwd(d, y_=off4(y)) == -1 and b"aligned" in L.kpn_last_error()
    assert bwd(d, dy_=off4(g_dev)) == -1 and b"aligned" in L.kpn_last_error()
    assert fwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    assert bwd(d, nb_=nb - 1) == -1 and b"workspace" in L.kpn_last_error()
    hole = pointers(B, params.bias[:-1] + [None])
    assert L.kpn_res_encoder_forward(ctypes.byref(d), B.ptr(x_dev), B.ptr(params.packed), hole, B.ptr(y), B.ptr(scratch), B.ptr(ws), nb, B.stream) == -1
    assert b"null" in L.kpn_last_error()
    bad = desc(c, ngf=12)
    assert L.kpn_res_encoder_packed_floats(ctypes.byref(bad)) == 0 and L.kpn_res_encoder_layers(ctypes.byref(bad)) == 0
    assert L.kpn_res_encoder_pack_device(ctypes.byref(bad), pointers(B, params.weights), B.ptr(scratch), B.stream) == -1 and b"ngf must" in L.kpn_last_error()
    # a refused call launches nothing
    assert all((B.get(v) == CANARY).all() for v in [y, scratch] + grads)
    assert fwd(d) == 0 and bwd(d) == 0
    assert np.array_equal(B.get(y), y0) and not any((B.get(v) == CANARY).all() for v in grads)


def check_pack_is_the_single_layers_packs(L, B, name):
    """kpn_res_encoder_pack_device writes, byte for byte, what kpn_conv2d_rp_pack_device / kpn_conv2d_s2_pack_device write for each layer's
    weight, in layer order; kpn_res_encoder_packed_floats is the sum of the single layers' counts"""
    c = CASES[name]
    net = reference(name)[0]
    params = Params(L, B, c, net)
    parts, floats = [], 0
    for (kind, cin, cout, k, _, _), m in zip(layers_of(c), convs_of(net)):
        w = m.weight.detach().numpy()
        if kind in ("down", "up"):
            cd = dict(kind=sc.CONV3 if kind == "down" else sc.DECONV3, cin=cin, cout=cout, N=1, H=2, W=2, bias=True)
            parts.append(B.get(sc.pack(L, B, cd, w)))
            floats += L.kpn_conv2d_s2_packed_floats(ctypes.byref(sc.desc(cd)))
        else:
            cd = dict(kind=rc.STEM7 if kind == "stem" else (rc.CONV3 if k == 3 else rc.CONV7), cin=cin, cout=cout, N=1, H=1, W=1, bias=True)
            parts.append(B.get(rc.pack(L, B, cd, w)))
            floats += L.kpn_conv2d_rp_packed_floats(ctypes.byref(rc.desc(cd)))
    assert sorted({l[0] for l in layers_of(c)}) == ["down", "out", "res", "stem", "up"]          # every layer kind
    want = np.concatenate([p.reshape(-1) for p in parts])
    assert L.kpn_res_encoder_packed_floats(ctypes.byref(desc(c))) == floats == want.size
    assert np.array_equal(_bits(B.get(params.packed)), _bits(want))


def layer_by_layer(L, B, name):
    """the forward of one case through the single layers of the C ABI (kpn_conv2d_rp_forward / kpn_conv2d_s2_forward /
    kpn_group_norm_forward per layer, one fp32 add per ResBlk): the dataflow of install_native_tex() -> (y NHWC, {"c0" .., "a0" ..: NHWC})"""
    c = CASES[name]
    net, x, _, _, _ = reference(name)
    convs, ls = convs_of(net), layers_of(c)

    def conv(i, t):
        kind, cin, cout, k, _, _ = ls[i]
        w, b = convs[i].weight.detach().numpy(), convs[i].bias.detach().numpy()
        if kind in ("down", "up"):
            cd = dict(kind=sc.CONV3 if kind == "down" else sc.DECONV3, cin=cin, cout=cout, N=t.shape[0], H=t.shape[1], W=t.shape[2], bias=True)
            return sc.forward(L, B, cd, t, sc.pack(L, B, cd, w), b)
        rk = rc.STEM7 if kind == "stem" else (rc.CONV3 if k == 3 else rc.CONV7)
        H, W = (t.shape[2], t.shape[3]) if kind == "stem" else (t.shape[1], t.shape[2])
        cd = dict(kind=rk, cin=cin, cout=cout, N=t.shape[0], H=H, W=W, bias=True)
        return rc.forward(L, B, cd, t, rc.pack(L, B, cd, w), b)

    def inorm(t, relu):
        nd = dict(N=t.shape[0], C=t.shape[3], H=t.shape[1], W=t.shape[2], G=t.shape[3], affine=0)
        return nc.forward(L, B, nd, relu, t, None, None)[0]

    got, t, i = {}, x.numpy(), 0
    for i in range(1 + c["n_down"]):
        got[f"c{i}"] = conv(i, t)
        t = inorm(got[f"c{i}"], 1)
    got["a0"] = t
    i += 1
    for k in range(c["n_blocks"]):
        got[f"c{i}"] = conv(i, t)
        got[f"c{i + 1}"] = conv(i + 1, inorm(got[f"c{i}"], 1))
        t = t + inorm(got[f"c{i + 1}"], 0)
        got[f"a{k + 1}"] = t
        i += 2
    for _ in range(c["n_up"]):
        got[f"c{i}"] = conv(i, t)
        t = inorm(got[f"c{i}"], 1)
        i += 1
    return conv(i, t), got


def check_layer_by_layer_bits(L, B, name):
    """y and every kept tensor of kpn_res_encoder_forward have the bits of layer_by_layer: same kernels, same launch geometry, the same
    fmaf, one commutative add"""
    c = CASES[name]
    y, state, _ = run(L, B, name, want=())
    kept = state_slices(c, state)
    want_y, got = layer_by_layer(L, B, name)
    assert np.array_equal(_bits(y), _bits(want_y))
    assert sorted(got) == sorted(kept)
    for k, v in got.items():
        assert np.array_equal(_bits(kept[k]), _bits(nchw(v))), k
    return want_y
