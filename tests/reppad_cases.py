"""Test infrastructure of the native replication-padded convolutions (kpn_conv2d_rp_*): the cases, their Family and what only this
family checks.  The fp64 reference, the driver of the C ABI and the properties shared with the other single-layer families:
tests/layer_cases.py, bound to the Family below under the names the test files use.  The bar and the buffers: tests/parity.py.

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
from tests import layer_cases as lc
from tests.parity import CANARY, DeviceArrays, HostArrays, check, nchw, nhwc, ratio  # noqa: F401  (the test files take them from here)

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


def torch_layer(c, x, w, b):
    p = k_of(c) // 2
    return F.conv2d(F.pad(x, (p,) * 4, mode="replicate"), w, b)


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


FAMILY = lc.Family(
    cases=CASES, Desc=kl.Conv2dRpDesc, fields=("N", "H", "W", "cin", "cout", "kind", "has_bias"), prefix="kpn_conv2d_rp_", seed=3000,
    k_of=k_of, w_shape=w_shape, out_hw=lambda c: (c["H"], c["W"]), torch_layer=torch_layer, has_dx=lambda c: c["kind"] != STEM7,
    x_is_nchw=lambda c: c["kind"] == STEM7, wgrad_gemm=lambda c: (c["cin"], c["cout"], c["N"] * c["H"] * c["W"]),
    closed_form_dx={name: closed_form_dx for name in CLOSED_FORM})
_of = lambda f: functools.partial(f, FAMILY)  # noqa: E731
desc, inputs, reference, expected_ranges, x_layout = _of(lc.desc), _of(lc.inputs), _of(lc.reference), _of(lc.expected_ranges), _of(lc.x_layout)
pack, workspace, forward, backward, legs_of = _of(lc.pack), _of(lc.workspace), _of(lc.forward), _of(lc.backward), _of(lc.legs_of)
check_case, check_two_calls_equal_bits = _of(lc.check_case), _of(lc.check_two_calls_equal_bits)
check_null_legs_leave_buffers_alone, check_zero_dy_gives_zeros = _of(lc.check_null_legs_leave_buffers_alone), _of(lc.check_zero_dy_gives_zeros)
check_padded_stem_channel = functools.partial(lc.check_padded_stem_channel, FAMILY, name="rp7stem_3to16")


def check_a_wrong_ring_fails(name="rp3_4to8"):
    """the case a wrong ring fails: the zero-padded input gradient, which is right on every interior pixel, misses the bar of this case
    by orders of magnitude - on the ring"""
    c = CASES[name]
    (x, w, b, g), r64, e_ref = reference(name)
    xz = x.double().requires_grad_(True)
    zero = torch.autograd.grad(F.conv2d(xz, w.double(), padding=k_of(c) // 2), xz, g.double())[0].numpy()
    assert ratio(zero, r64["dx"], e_ref["dx"]) > 1e3
    assert ratio(zero[:, :, 1:-1, 1:-1], r64["dx"][:, :, 1:-1, 1:-1], e_ref["dx"]) <= 4.0


def check_range_counts(L):
    for name in ("rp3_ranges", "rp7stem_ranges"):
        c = CASES[name]
        n, chunks, cpr = expected_ranges(c)
        assert (n, chunks, cpr) == (3, 48, 20)                                  # 20 / 20 / 8: a ragged last range
        assert L.kpn_conv2d_rp_wgrad_ranges(ctypes.byref(desc(c))) == n
    for name in ("rp3_4to8", "rp3_1x1", "rp7_2x2", "rp7_16to8", "rp7stem_3to16"):
        assert L.kpn_conv2d_rp_wgrad_ranges(ctypes.byref(desc(CASES[name]))) == expected_ranges(CASES[name])[0] == 1


def check_refusals(L, B):
    lc.check_refusals(FAMILY, L, B, "rp3_4to8",
                      ((dict(cin=6), b"cin must"), (dict(cout=10), b"cout must"), (dict(kind=3), b"kind must"), (dict(kind=-1), b"kind must"),
                       (dict(N=0), b"N, H, W"), (dict(has_bias=2), b"has_bias")), bad_pack=(dict(cin=6), b"cin must"), stem_name="rp7stem_3to16")
    assert L.kpn_abi_version() == 10
