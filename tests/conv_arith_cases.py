"""Test infrastructure of the arithmetic selector of the native convolution (kpn_conv2d_ex_*, kpn_conv_block_ex_*): the cases the
bf16 x 3 kernels' own rules need beside tests/conv_cases.py's, and one driver for host arrays (the emulator build) and device tensors
(the product library).

The driver is tests/conv_cases.py's and tests/block_cases.py's own: ArithLib presents kpn_conv2d_<f> and kpn_conv_block_<f> of a library
as their _ex forms with one fixed arith, so every property written there is asked of the other arithmetic unchanged - reference, e_ref
and bar included: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)).
"""
import ctypes
import functools

import numpy as np
import torch

from keypointnerf_amd import lib as kl
from tests import block_cases as bc
from tests import conv_cases as cc
from tests.parity import CANARY, DeviceArrays, HostArrays, bits, check, nchw, nhwc  # noqa: F401

F32, B3 = kl.CONV_F32, kl.CONV_BF16X3
_FAMILIES = ("kpn_conv2d_", "kpn_conv_block_")
_OTHER = ("kpn_conv2d_s2_", "kpn_conv2d_rp_", "kpn_conv2d_ex_", "kpn_conv_block_ex_")


class ArithLib:
    """a library whose kpn_conv2d_* / kpn_conv_block_* are the _ex entry points with this arith; everything else is the library's"""

    def __init__(self, L, arith):
        self._L, self.arith = L, arith

    def __getattr__(self, name):
        if not name.startswith(_OTHER):
            for fam in _FAMILIES:
                if name.startswith(fam):
                    fn = getattr(self._L, fam + "ex_" + name[len(fam):])
                    return lambda desc, *a: fn(desc, self.arith, *a)
        return getattr(self._L, name)


# ---- the rules of KPN_CONV_BF16X3 as include/kpnerf.h states them, restated ----
def tile(cout):
    """(BM, BN) of a GEMM with `cout` output channels: pixels (or K rows of a weight gradient) x channels"""
    return (128, 64) if cout > 32 else (256, 32)


def expected_ksplit(Ho, Wo, K, cout):
    """K ranges of one k_enc_conv_b3 launch: from the per-image geometry alone; fewer than 128 tiles per image split K towards 256
    workgroups, at most 16 ranges and at most one per chunk of 32"""
    bm, bn = tile(cout)
    tiles = -(-Ho * Wo // bm) * -(-cout // bn)
    nk = -(-K // 32)
    return 1 if tiles >= 128 else max(1, min(nk, 16, -(-256 // tiles)))


def fwd_ksplit(c):
    Ho, Wo = cc.out_hw(c)
    return expected_ksplit(Ho, Wo, c["k"] ** 2 * c["cin"], c["cout"])


def dx_ksplit(c):
    return expected_ksplit(c["H"], c["W"], c["k"] ** 2 * c["cout"], c["cin"])


# the range rule of kpn_conv2d_wgrad_ranges over the bf16 x 3 tile -> (ranges, chunks, chunks per range)
expected_ranges = functools.partial(cc.expected_ranges, tile=tile)


# ---- the cases the new kernels' own rules need; each is stated from its rule and asserted against it in check_own_rules ----
OWN_CASES = {
    # split K, both sides of the threshold of 128 tiles per image (BM 128, two channel tiles): 96 x 96 pixels are 72 x 2 = 144 tiles,
    # unsplit although K = 36 has two chunks; 84 x 96 are 63 x 2 = 126 tiles and split in two.  y only: dX of 128 channels at these
    # sizes is minutes of emulator time and runs the same kernel
    "unsplit_144": dict(N=1, H=96, W=96, cin=4, cout=128, k=3, pad=1, bias=False, only=("y",)),
    "split_126": dict(N=1, H=84, W=96, cin=4, cout=128, k=3, pad=1, bias=True, only=("y",)),
    # 90 pixels on the 128 x 64 tile: wavefront row 1 owns pixels 64 .. 127, its first accumulator is ragged (64 .. 89), its last empty
    "acc_empty": dict(N=1, H=9, W=10, cin=8, cout=64, k=3, pad=1, bias=False),
    # K = 72 for y and dX: two chunks of 32 and 8 entries, ending inside the first 16-wide slab of the third chunk
    "k_first_half": dict(N=1, H=6, W=6, cin=8, cout=8, k=3, pad=1, bias=True),
    # 340 output pixels = 22 chunks of 16: one past the boundary of conv_cases' range1 (20 chunks, exactly one range): two ranges
    "range2": dict(N=1, H=17, W=20, cin=8, cout=8, k=3, pad=1, bias=True),
}
CASES = dict(cc.CASES, **OWN_CASES)


def check_own_rules(L3):
    """every own case is where its comment says, by the restated rules and, where the ABI reports it, by the library"""
    assert fwd_ksplit(CASES["unsplit_144"]) == 1 and -(-96 * 96 // 128) * 2 == 144
    assert fwd_ksplit(CASES["split_126"]) == 2 and -(-84 * 96 // 128) * 2 == 126
    assert all(fwd_ksplit(c) > 1 or dx_ksplit(c) > 1 for c in cc.CASES.values())         # the inherited cases split K somewhere
    c = CASES["acc_empty"]
    assert tile(c["cout"]) == (128, 64) and 64 < c["H"] * c["W"] <= 96
    assert (9 * CASES["k_first_half"]["cin"]) % 32 in range(1, 17) and (9 * CASES["k_first_half"]["cout"]) % 32 in range(1, 17)
    assert (9 * cc.CASES["k3_4to8"]["cin"]) % 32 in range(1, 17)                          # K = 36: so does the inherited case
    for name, want in (("ranges3", 3), ("range1", 1), ("range2", 2)):
        n, chunks, cpr = expected_ranges(CASES[name])
        assert n == want and L3.kpn_conv2d_wgrad_ranges(ctypes.byref(cc.desc(CASES[name]))) == want, name
    assert expected_ranges(CASES["range1"])[1:] == (20, 20) and expected_ranges(CASES["range2"])[1:] == (22, 20)


@functools.lru_cache(maxsize=None)
def reference(name, seed=0):
    """conv_cases.reference for its cases and, computed in the same way, for the own ones"""
    if name in cc.CASES:
        return cc.reference(name, seed)
    return cc.reference_of(OWN_CASES[name], seed)


def run(L, B, name, scale_x=1.0, scale_g=1.0):
    """pack, forward and (unless the case is y only) backward of one case -> (packed buffer of B, {y, dx, dw, db} as NCHW / OIHW numpy)"""
    c = CASES[name]
    (x, w, b, g), _, _ = reference(name)
    packed = cc.pack(L, B, c, w.numpy())
    x_nhwc, g_nhwc = nhwc(x) * np.float32(scale_x), nhwc(g) * np.float32(scale_g)
    out = {"y": nchw(cc.forward(L, B, c, x_nhwc, packed, None if b is None else b.numpy()))}
    if c.get("only") != ("y",):
        bw = cc.backward(L, B, c, x_nhwc, g_nhwc, packed, cc.legs_of(c))
        out.update(dx=nchw(bw["dx"]), dw=bw["dw"], db=bw["db"])
    return packed, out


def check_case(L, B, name):
    """y, dX, dW, db of one case against the fp64 reference, each within the standing bar; -> {tensor: ratio}"""
    c = CASES[name]
    _, r64, e_ref = reference(name)
    _, out = run(L, B, name)
    ratios = {}
    for k in ("y", "dx", "dw", "db"):
        if k not in out:
            continue
        if k == "db" and not c["bias"]:
            assert (out["db"] == CANARY).all()
            continue
        ratios[k] = check(f"{name} arith {L.arith} {k}", out[k], r64[k], e_ref[k])
    return ratios


def check_f32_through_ex_has_the_bits_of_the_plain_entry_points(L, B, name):
    c = CASES[name]
    L0 = ArithLib(L, F32)
    d = ctypes.byref(cc.desc(c))
    assert L0.kpn_conv2d_packed_floats(d) == L.kpn_conv2d_packed_floats(d) and L0.kpn_conv2d_workspace_bytes(d) == L.kpn_conv2d_workspace_bytes(d)
    assert L0.kpn_conv2d_wgrad_ranges(d) == L.kpn_conv2d_wgrad_ranges(d)
    (pa, a), (pb, b) = run(L, B, name), run(L0, B, name)
    assert np.array_equal(bits(B.get(pa)), bits(B.get(pb)))
    for k in ("y", "dx", "dw", "db"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def check_two_calls_equal_bits(L, B, name):
    (pa, a), (pb, b) = run(L, B, name), run(L, B, name)
    assert np.array_equal(bits(B.get(pa)), bits(B.get(pb)))
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def check_image_does_not_depend_on_batch(L, B, name, image=1):
    """y and dX of one image alone (N = 1) and inside its batch have equal bits"""
    c = CASES[name]
    assert c["N"] > image
    (x, w, b, g), _, _ = reference(name)
    packed = cc.pack(L, B, c, w.numpy())
    bias = None if b is None else b.numpy()
    yb = cc.forward(L, B, c, nhwc(x), packed, bias)
    dxb = cc.backward(L, B, c, nhwc(x), nhwc(g), packed, ("dx",))["dx"]
    c1 = dict(c, N=1)
    x1, g1 = nhwc(x[image:image + 1]), nhwc(g[image:image + 1])
    y1 = cc.forward(L, B, c1, x1, packed, bias)
    dx1 = cc.backward(L, B, c1, x1, g1, packed, ("dx",))["dx"]
    assert np.array_equal(bits(y1), bits(yb[image:image + 1])) and np.array_equal(bits(dx1), bits(dxb[image:image + 1]))


def check_exponent_range(L, B, name):
    """x scaled by 2^20 and dy by 2^-40 (both exact): y, dX and dW are the unscaled results times the same powers of two, bit for bit -
    three bf16 pieces keep fp32's exponent range, which two fp16 pieces do not"""
    c = CASES[name]
    assert not c["bias"]                                     # a bias would not scale with x
    _, a = run(L, B, name)
    _, s = run(L, B, name, scale_x=2.0 ** 20, scale_g=2.0 ** -40)
    for k, f in (("y", 2.0 ** 20), ("dx", 2.0 ** -40), ("dw", 2.0 ** -20)):
        want = a[k] * np.float32(f)
        assert np.isfinite(want).all() and (np.abs(want[want != 0]) > 1e-30).all()       # the scaling itself is exact: nothing subnormal
        assert np.array_equal(bits(s[k]), bits(want)), k


def unpack_b3(packed, K, cout):
    """the first packed copy of a bf16 x 3 pack -> the pieces [3][chunks * 32][cout_p] as fp32"""
    bn = tile(cout)[1]
    nk, cout_p = -(-K // 32), -(-cout // bn) * bn
    u = np.ascontiguousarray(packed[:nk * cout_p * 48]).view(np.uint16).reshape(nk, 3, 4, cout_p, 8)
    f = (u.astype(np.uint32) << 16).view(np.float32)
    return f.transpose(1, 0, 2, 4, 3).reshape(3, nk * 32, cout_p), nk * cout_p * 48


def check_packed_pieces(L3, B, name):
    """both copies: [chunk of 32][piece][K octet][cout_p][8 bf16]; h + m + l gives the weight back to 2^-24 relative, h is its bf16
    rounding, and padded taps and channels are zero in all three pieces"""
    c = CASES[name]
    w = reference(name)[0][1].numpy()
    cin, cout, k = c["cin"], c["cout"], c["k"]
    packed = B.get(cc.pack(L3, B, c, w))
    fwd, n_f = unpack_b3(packed, k * k * cin, cout)
    bwd, n_b = unpack_b3(packed[n_f:], k * k * cout, cin)
    assert packed.size == n_f + n_b
    for pieces, K, C, want in ((fwd, k * k * cin, cout, w.transpose(2, 3, 1, 0).reshape(k * k * cin, cout)),
                               (bwd, k * k * cout, cin, w[:, :, ::-1, ::-1].transpose(2, 3, 0, 1).reshape(k * k * cout, cin))):
        assert not pieces[:, K:].any() and not pieces[:, :, C:].any()
        h, m, lo = (pieces[i, :K, :C].astype(np.float64) for i in range(3))
        assert np.array_equal(pieces[0, :K, :C], torch.from_numpy(np.ascontiguousarray(want)).bfloat16().float().numpy())
        assert (np.abs(h + m + lo - want) <= 2.0 ** -24 * np.abs(want)).all()


def check_packs_of_the_two_arithmetics_differ_in_size(L):
    for c in CASES.values():
        d = ctypes.byref(cc.desc(c))
        n0, n3 = L.kpn_conv2d_ex_packed_floats(d, F32), L.kpn_conv2d_ex_packed_floats(d, B3)
        assert n0 == L.kpn_conv2d_packed_floats(d) and n0 > 0 and n3 > n0


def check_bad_arith(L, B):
    """an unknown arith: the size queries return 0, the calls return KPN_EINVAL with a message that names arith, and nothing is launched"""
    c = CASES["k3_4to8"]
    (x, w, b, g), _, _ = reference("k3_4to8")
    L3 = ArithLib(L, B3)
    packed = cc.pack(L3, B, c, w.numpy())
    ws, nb = cc.workspace(L3, B, c)
    d = ctypes.byref(cc.desc(c))
    Ho, Wo = cc.out_hw(c)
    x_dev, g_dev, b_dev, w_dev = B.put(nhwc(x)), B.put(nhwc(g)), B.put(b.numpy()), B.put(w.numpy())
    y, dx = B.full((c["N"], Ho, Wo, c["cout"]), CANARY), B.full((c["N"], c["H"], c["W"], c["cin"]), CANARY)
    out = B.full(int(B.get(packed).size), CANARY)
    for bad in (2, -1, 7):
        assert L.kpn_conv2d_ex_packed_floats(d, bad) == 0 and L.kpn_conv2d_ex_workspace_bytes(d, bad) == 0
        assert L.kpn_conv2d_ex_wgrad_ranges(d, bad) == 0
        calls = (lambda: L.kpn_conv2d_ex_pack_device(d, bad, B.ptr(w_dev), B.ptr(out), B.stream),
                 lambda: L.kpn_conv2d_ex_forward(d, bad, B.ptr(x_dev), B.ptr(packed), B.ptr(b_dev), B.ptr(y), B.ptr(ws), nb, B.stream),
                 lambda: L.kpn_conv2d_ex_backward(d, bad, B.ptr(x_dev), B.ptr(g_dev), B.ptr(packed), B.ptr(dx), None, None, B.ptr(ws), nb, B.stream))
        for call in calls:
            assert call() == -1 and b"arith must" in L.kpn_last_error(), L.kpn_last_error()
    assert all((B.get(v) == CANARY).all() for v in (y, dx, out))
    # the block
    name = "d4to16"
    cb = bc.CASES[name]
    net, xb, gb, _, _ = bc.reference(name)
    params = bc.Params(L3, B, cb, net)
    yb0, state = bc.forward(L3, B, cb, params, nhwc(xb))
    wsb, nbb = bc.workspace(L3, B, cb)
    db_ = ctypes.byref(bc.desc(cb))
    xb_dev, gb_dev = B.put(nhwc(xb)), B.put(nhwc(gb))
    yb, dxb = B.full((cb["N"], cb["H"], cb["W"], cb["cout"]), CANARY), B.full((cb["N"], cb["H"], cb["W"], cb["cin"]), CANARY)
    scratch, gr = B.full(int(state.shape[0]), CANARY), kl.ConvBlockGrads()
    assert L.kpn_conv_block_ex_workspace_bytes(db_, 2) == 0 and L.kpn_conv_block_ex_state_floats(db_, 2) == 0
    assert L.kpn_conv_block_ex_forward(db_, 2, B.ptr(xb_dev), ctypes.byref(params.struct), B.ptr(yb), B.ptr(scratch), B.ptr(wsb), nbb, B.stream) == -1
    assert b"arith must" in L.kpn_last_error()
    assert L.kpn_conv_block_ex_backward(db_, 2, B.ptr(xb_dev), B.ptr(gb_dev), ctypes.byref(params.struct), B.ptr(state), B.ptr(dxb),
                                        ctypes.byref(gr), B.ptr(wsb), nbb, B.stream) == -1
    assert b"arith must" in L.kpn_last_error()
    assert all((B.get(v) == CANARY).all() for v in (yb, dxb, scratch))


# ---- the fused block ----
BLOCKS = ("d4to16", "i32")       # the two smallest shapes of tests/block_cases.py: the downsample leg, and cin == cout


def check_block_has_the_bits_of_its_legs(L, B, name):
    """y and the kept slices of kpn_conv_block_ex_forward against kpn_group_norm_forward(relu = 1) + kpn_conv2d_ex_forward per leg with the
    same arith, a concatenation and one fp32 add - the property the fp32 block has (tests/test_block_cpu.py)"""
    from tests import norm_cases as nc
    c = bc.CASES[name]
    net, x, _, _, _ = bc.reference(name)
    y, state, _ = bc.run(L, B, name, legs=())
    win, wout, ks = bc.widths(c)

    def leg(i, t):
        bn, conv = bc.leg_modules(net)[i]
        nd = dict(N=c["N"], C=win[i], H=c["H"], W=c["W"], G=min(32, win[i]), affine=1)
        n, _ = nc.forward(L, B, nd, 1, t, bn.weight.detach().numpy(), bn.bias.detach().numpy())
        cd = dict(N=c["N"], H=c["H"], W=c["W"], cin=win[i], cout=wout[i], k=ks[i], pad=ks[i] // 2, bias=False)
        return cc.forward(L, B, cd, n, cc.pack(L, B, cd, conv.weight.detach().numpy()), None)

    x_nhwc = nhwc(x)
    o1 = leg(0, x_nhwc)
    o2 = leg(1, o1)
    o3 = leg(2, o2)
    want = np.concatenate((o1, o2, o3), -1) + (leg(3, x_nhwc) if bc.legs_of(c) == 4 else x_nhwc)
    assert np.array_equal(bits(y), bits(want))
    s1, s2 = bc.state_slices(c, state)
    assert np.array_equal(bits(s1), bits(nchw(o1))) and np.array_equal(bits(s2), bits(nchw(o2)))
