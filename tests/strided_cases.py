"""Test infrastructure of the native stride-2, stem and transposed convolutions (kpn_conv2d_s2_*): the cases, their Family and what only
this family checks.  The fp64 reference, the driver of the C ABI and the properties shared with the other single-layer families:
tests/layer_cases.py, bound to the Family below under the names the test files use.  The bar and the buffers: tests/parity.py.

Reference: seeded normal x, w, b and seed gradient g give y, dX, dW, db from torch.nn.functional.conv2d / conv_transpose2d and
torch.autograd.grad on the CPU in fp64.  e_ref is the max deviation of the same computation in CPU fp32 from that, per tensor.
The bar, for every element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)).
"""
import ctypes
import functools

import torch.nn.functional as F

from keypointnerf_amd import lib as kl
from tests import layer_cases as lc
from tests.parity import CANARY, DeviceArrays, HostArrays, check, nchw, nhwc, ratio  # noqa: F401  (the test files take them from here)

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


def torch_layer(c, x, w, b):
    if c["kind"] == DECONV3:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    return F.conv2d(x, w, b, stride=2, padding=3 if c["kind"] == STEM7 else 1)


def wgrad_gemm(c):
    """the transposed layer's weight gradient is that of a convolution cout -> cin over the source pixels"""
    if c["kind"] == DECONV3:
        return c["cout"], c["cin"], c["N"] * c["H"] * c["W"]
    Ho, Wo = out_hw(c)
    return c["cin"], c["cout"], c["N"] * Ho * Wo


FAMILY = lc.Family(
    cases=CASES, Desc=kl.Conv2dS2Desc, fields=("N", "H", "W", "cin", "cout", "kind", "has_bias"), prefix="kpn_conv2d_s2_", seed=2000,
    k_of=k_of, w_shape=w_shape, out_hw=out_hw, torch_layer=torch_layer, has_dx=lambda c: c["kind"] != STEM7,
    x_is_nchw=lambda c: c["kind"] == STEM7, wgrad_gemm=wgrad_gemm)
_of = lambda f: functools.partial(f, FAMILY)  # noqa: E731
desc, inputs, reference, expected_ranges, x_layout = _of(lc.desc), _of(lc.inputs), _of(lc.reference), _of(lc.expected_ranges), _of(lc.x_layout)
pack, workspace, forward, backward, legs_of = _of(lc.pack), _of(lc.workspace), _of(lc.forward), _of(lc.backward), _of(lc.legs_of)
check_case, check_two_calls_equal_bits = _of(lc.check_case), _of(lc.check_two_calls_equal_bits)
check_null_legs_leave_buffers_alone, check_zero_dy_gives_zeros = _of(lc.check_null_legs_leave_buffers_alone), _of(lc.check_zero_dy_gives_zeros)
check_padded_stem_channel = functools.partial(lc.check_padded_stem_channel, FAMILY, name="stem_3to64")


def check_range_counts(L):
    for name in ("s2_ranges", "stem_ranges", "up_ranges"):
        c = CASES[name]
        n, chunks, cpr = expected_ranges(c)
        assert (n, chunks, cpr) == (3, 48, 20)                                  # 20 / 20 / 8: a ragged last range
        assert L.kpn_conv2d_s2_wgrad_ranges(ctypes.byref(desc(c))) == n
    for name in ("s2_4to8", "stem_odd", "up_1x1"):
        assert L.kpn_conv2d_s2_wgrad_ranges(ctypes.byref(desc(CASES[name]))) == expected_ranges(CASES[name])[0] == 1


def check_refusals(L, B):
    lc.check_refusals(FAMILY, L, B, "s2_4to8",
                      ((dict(H=5), b"H, W must be even"), (dict(cin=6), b"cin must"), (dict(cout=10), b"cout must"), (dict(kind=3), b"kind must"),
                       (dict(kind=-1), b"kind must"), (dict(N=0), b"N, H, W"), (dict(has_bias=2), b"has_bias")),
                      bad_pack=(dict(cin=6), b"cin must"), stem_name="stem_3to64")
    assert L.kpn_abi_version() == 10
