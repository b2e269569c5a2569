"""Test infrastructure of the native convolution (kpn_conv2d_*): the cases, their Family and what only this family checks.  The fp64
reference, the driver of the C ABI and the properties shared with the stride-2 and replication-padded families: tests/layer_cases.py,
bound to the Family below under the names the test files use.  The bar and the buffers: tests/parity.py.

Reference: seeded normal x, w, b and seed gradient g give y, dX, dW, db from torch.nn.functional.conv2d and torch.autograd.grad
on the CPU in fp64.  e_ref is the max deviation of the same computation in CPU fp32 from that, per tensor.  The bar, for every
element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)).
"""
import ctypes
import functools

import torch
import torch.nn.functional as F

from keypointnerf_amd import lib as kl
from tests import layer_cases as lc
from tests.parity import CANARY, FACTOR, DeviceArrays, HostArrays, check, nchw, nhwc, ratio  # noqa: F401  (the test files take them from here)

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


def out_hw(c):
    return c["H"] + 2 * c["pad"] - c["k"] + 1, c["W"] + 2 * c["pad"] - c["k"] + 1


FAMILY = lc.Family(
    cases=CASES, Desc=kl.Conv2dDesc, fields=("N", "H", "W", "cin", "cout", "k", "pad", "has_bias"), prefix="kpn_conv2d_", seed=1000,
    k_of=lambda c: c["k"], w_shape=lambda c: (c["cout"], c["cin"], c["k"], c["k"]), out_hw=out_hw,
    torch_layer=lambda c, x, w, b: F.conv2d(x, w, b, stride=1, padding=c["pad"]),
    has_dx=lambda c: True, x_is_nchw=lambda c: False,
    wgrad_gemm=lambda c: (c["cin"], c["cout"], c["N"] * out_hw(c)[0] * out_hw(c)[1]))
_of = lambda f: functools.partial(f, FAMILY)  # noqa: E731
desc, inputs, reference, reference_of, expected_ranges = _of(lc.desc), _of(lc.inputs), _of(lc.reference), _of(lc.reference_of), _of(lc.expected_ranges)
pack, workspace, forward, backward, legs_of = _of(lc.pack), _of(lc.workspace), _of(lc.forward), _of(lc.backward), _of(lc.legs_of)
check_case, check_two_calls_equal_bits = _of(lc.check_case), _of(lc.check_two_calls_equal_bits)
check_null_legs_leave_buffers_alone, check_zero_dy_gives_zeros = _of(lc.check_null_legs_leave_buffers_alone), _of(lc.check_zero_dy_gives_zeros)


def check_bad_descriptors(L, B):
    # the stems (k = 7, the only stride-2 / 7 x 7 layers), p >= k, channels that are no multiple of 4: each names its field
    lc.check_refusals(FAMILY, L, B, "k3_4to8", ((dict(k=7, pad=3), b"k must"), (dict(pad=3), b"pad must"), (dict(cin=6), b"cin must"),
                                                (dict(cout=10), b"cout must"), (dict(H=0), b"N, H, W")), bad_pack=(dict(k=7), b"k must"))


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
