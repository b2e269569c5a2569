"""The native replication-padded convolutions (kpn_conv2d_rp_forward / kpn_conv2d_rp_backward) on the host SIMT emulator: the very
kernel sources, with numpy buffers through the C ABI.  Cases, reference and bar: tests/reppad_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import reppad_cases as rc
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


B = rc.HostArrays()


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_forward_and_gradients_against_fp64(L, name):
    rc.check_case(L, B, name)


def test_one_case_fails_a_wrong_ring():
    rc.check_a_wrong_ring_fails()


def test_no_case_needs_more_than_the_factor_for_sums_taken_before_the_product():
    """The native dx adds the ring's dy values, then multiplies; torch multiplies, then adds.  Emulate the native order in CPU fp32
    (the rectangle sums in fp32, oy outer and ox inner, then one fp32 contraction with the weight) and hold it to the bar: the factor 4
    over torch's own fp32 error covers the other order in every case."""
    for name, c in rc.CASES.items():
        if c["kind"] == rc.STEM7:
            continue
        (x, w, b, g), r64, e_ref = rc.reference(name)
        k, H, W = rc.k_of(c), c["H"], c["W"]
        p = k // 2
        dx = torch.zeros(c["N"], c["cin"], H, W, dtype=torch.float32)
        for ky in range(k):
            for kx in range(k):
                s = torch.zeros(c["N"], c["cout"], H, W, dtype=torch.float32)
                for oy in range(H):
                    for ox in range(W):
                        s[:, :, min(max(oy + ky - p, 0), H - 1), min(max(ox + kx - p, 0), W - 1)] += g[:, :, oy, ox]
                dx += torch.einsum("oi,nohw->nihw", w[:, :, ky, kx], s)
        r = rc.ratio(dx.numpy(), r64["dx"], e_ref["dx"])
        print(f"[reppad] {name}: sums before the product, CPU fp32: ratio {r:.3f}")
        assert r <= 4.0, (name, r)


@pytest.mark.parametrize("name", rc.ONE_PER_KIND)
def test_two_calls_give_equal_bits(L, name):
    rc.check_two_calls_equal_bits(L, B, name)


@pytest.mark.parametrize("name", ("rp3_4to8", "rp7_8to4", "rp7stem_3to16"))
def test_null_legs_leave_their_buffers_untouched(L, name):
    rc.check_null_legs_leave_buffers_alone(L, B, name)


@pytest.mark.parametrize("name", rc.ONE_PER_KIND)
def test_zero_dy_gives_exact_zeros(L, name):
    rc.check_zero_dy_gives_zeros(L, B, name)


def test_wgrad_range_counts_follow_the_stated_rule(L):
    rc.check_range_counts(L)


def test_the_padded_stem_channel_is_never_read(L):
    rc.check_padded_stem_channel(L, B)


def test_bad_calls_are_refused_with_a_message_and_launch_nothing(L):
    rc.check_refusals(L, B)


def test_packed_copies_per_kind(L):
    """forward copy, then the flipped input-gradient copy; the stem has the forward copy alone"""
    for name, copies in (("rp3_12to36", 2), ("rp7_16to8", 2), ("rp7stem_3to16", 1)):
        c = rc.CASES[name]
        n = L.kpn_conv2d_rp_packed_floats(ctypes.byref(rc.desc(c)))
        k2, cin_p = rc.k_of(c) ** 2, -(-c["cin"] // 4) * 4
        pad = lambda v, t: -(-v // t) * t  # noqa: E731
        fwd = -(-k2 * cin_p // 16) * pad(c["cout"], 64 if c["cout"] > 32 else 32) * 16
        dx = -(-k2 * c["cout"] // 16) * pad(c["cin"], 64 if c["cin"] > 32 else 32) * 16
        assert n == fwd + (dx if copies == 2 else 0)


def test_workspace_covers_the_range_partials(L):
    for name in ("rp3_ranges", "rp7stem_ranges"):
        c = rc.CASES[name]
        n = rc.expected_ranges(c)[0]
        assert L.kpn_conv2d_rp_workspace_bytes(ctypes.byref(rc.desc(c))) >= n * int(np.prod(rc.w_shape(c))) * 4


def test_fake_kernels_give_channels_last_shapes():
    import keypointnerf_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 12, 5, 7, device="cuda").contiguous(memory_format=torch.channels_last)
        for k, kind in ((3, rc.CONV3), (7, rc.CONV7)):
            w = torch.empty(36, 12, k, k, device="cuda")
            y = torch.ops.kpnerf.conv2d_replicate(x, w, None)
            assert tuple(y.shape) == (2, 36, 5, 7) and y.is_contiguous(memory_format=torch.channels_last)
            dx, dw, db = torch.ops.kpnerf.conv2d_rp_backward(x, w, y, kind, False, [True, True, False])
            assert dx.shape == x.shape and dx.is_contiguous(memory_format=torch.channels_last) and dw.shape == w.shape and db.numel() == 0
        im, ws, bs = torch.empty(1, 3, 9, 7, device="cuda"), torch.empty(8, 3, 7, 7, device="cuda"), torch.empty(8, device="cuda")
        ys = torch.ops.kpnerf.conv2d_replicate(im, ws, bs)
        assert tuple(ys.shape) == (1, 8, 9, 7) and ys.is_contiguous(memory_format=torch.channels_last)
        dx, dw, db = torch.ops.kpnerf.conv2d_rp_backward(im, ws, ys, rc.STEM7, True, [False, True, True])
        assert dx.numel() == 0 and dw.shape == ws.shape and tuple(db.shape) == (8,)
    with pytest.raises((NotImplementedError, RuntimeError)):             # no CPU kernel
        torch.ops.kpnerf.conv2d_replicate(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3), None)
