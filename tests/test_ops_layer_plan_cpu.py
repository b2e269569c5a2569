"""The cached layer plan behind ops.conv2d_*, conv2d_s2_* and conv2d_rp_* (ops._layer_plan), on the emulator library: its sizes against
fresh answers of the C ABI, its shapes and flags against the Family of tests/layer_cases.py, its cache, its refusal, and the
signatures of the thirteen public functions that sit on it."""
import ctypes
import inspect

import pytest

from keypointnerf_amd import lib as kl
from keypointnerf_amd import ops
from tests import conv_cases, reppad_cases, strided_cases
from tests import layer_cases as lc
from tests.simt_harness import simt_lib

FAMILIES = {"conv2d": conv_cases.FAMILY, "conv2d_s2": strided_cases.FAMILY, "conv2d_rp": reppad_cases.FAMILY}
CASES = [(name, case) for name, fam in FAMILIES.items() for case in sorted(fam.cases)]


@pytest.fixture(scope="module")
def L():
    return simt_lib()


def _what(name, c):
    return (c["k"], c["pad"]) if name == "conv2d" else c["kind"]


def _plan(L, name, c, **over):
    c = dict(c, **over)
    return ops._layer_plan(L, name, _what(name, c), c["cin"], c["cout"], c["N"], c["H"], c["W"], bool(c["bias"]))


def _check_plan(plan, fam, c, workspace_bytes, packed_floats):
    ref, forward, backward, pack, nb, pf, Ho, Wo, dw_shape, nchw, has_dx, d = plan
    assert nb == workspace_bytes > 0 and pf == packed_floats > 0
    assert (Ho, Wo) == tuple(fam.out_hw(c)) and dw_shape == tuple(fam.w_shape(c))
    assert nchw is bool(fam.x_is_nchw(c)) and has_dx is bool(fam.has_dx(c))
    assert all(getattr(d, f) == getattr(lc.desc(fam, c), f) for f in fam.fields)


@pytest.mark.parametrize("name,case", CASES)
def test_the_plan_has_the_librarys_sizes_and_the_familys_shapes(L, name, case):
    fam = FAMILIES[name]
    c = fam.cases[case]
    d = lc.desc(fam, c)
    plan = _plan(L, name, c)
    _check_plan(plan, fam, c, fam.fn(L, "workspace_bytes")(ctypes.byref(d)), fam.fn(L, "packed_floats")(ctypes.byref(d)))
    assert plan[1:4] == (fam.fn(L, "forward"), fam.fn(L, "backward"), fam.fn(L, "pack_device"))
    assert _plan(L, name, c) is plan                                    # a second lookup of the same key


@pytest.mark.parametrize("case", sorted(conv_cases.CASES))
def test_the_plan_of_the_other_arithmetic_has_that_arithmetics_sizes(L, case):
    c = conv_cases.CASES[case]
    d, B3 = conv_cases.desc(c), kl.CONV_BF16X3
    L3 = ops._ArithLibrary(L, B3)                                       # what ops._conv_library(CONV_BF16X3) hands to the plan
    plan = _plan(L3, "conv2d", c)
    _check_plan(plan, conv_cases.FAMILY, c, L.kpn_conv2d_ex_workspace_bytes(ctypes.byref(d), B3), L.kpn_conv2d_ex_packed_floats(ctypes.byref(d), B3))
    assert _plan(L3, "conv2d", c) is plan and _plan(L, "conv2d", c) is not plan     # the library is part of the key


@pytest.mark.parametrize("name,case", [("conv2d", "k3_4to8"), ("conv2d_s2", "up_8to4"), ("conv2d_rp", "rp7_8to4")])
def test_the_packers_plan_depends_on_the_weight_alone(L, name, case):
    fam = FAMILIES[name]
    c = fam.cases[case]
    plan = ops._layer_plan(L, name, _what(name, c), c["cin"], c["cout"])
    assert plan[5] == fam.fn(L, "packed_floats")(ctypes.byref(lc.desc(fam, c))) and plan[8] == tuple(fam.w_shape(c))
    assert plan[4] == 0 and ops._layer_plan(L, name, _what(name, c), c["cin"], c["cout"]) is plan


@pytest.mark.parametrize("name,case", [("conv2d", "k3_4to8"), ("conv2d_s2", "s2_4to8"), ("conv2d_rp", "rp3_4to8")])
def test_an_unserved_descriptor_raises_the_librarys_reason_every_time(L, name, case):
    c = FAMILIES[name].cases[case]
    before = ops._layer_plan.cache_info().currsize
    for _ in range(2):                                                  # nothing is kept of a refusal
        with pytest.raises(ValueError, match=f"^{name}: unsupported convolution: .*cin must be a multiple of 4"):
            _plan(L, name, c, cin=6)
        with pytest.raises(ValueError, match=f"^{name}: unsupported weight .*cin must be a multiple of 4"):
            ops._layer_plan(L, name, _what(name, c), 6, c["cout"])
    assert ops._layer_plan.cache_info().currsize == before
    assert ops._layer_plan.cache_info().maxsize == 4096


# inspect.signature of the public functions on the commit before the plan
SIGNATURES = {
    "conv2d_supported": "(cin, cout, k, arith=0)",
    "conv2d_pack": "(weight, arith=0)",
    "conv2d_forward": "(x, packed, bias, cout, k, padding, arith=0)",
    "conv2d_backward": "(x, dy, packed, cin, k, padding, has_bias, want_dx=True, want_dw=True, want_db=True, arith=0)",
    "conv2d_s2_supported": "(kind, cin, cout)",
    "conv2d_s2_pack": "(weight, kind)",
    "conv2d_s2_forward": "(x, packed, bias, cout, kind)",
    "conv2d_s2_backward": "(x, dy, packed, x_shape, kind, has_bias, want_dx=True, want_dw=True, want_db=True)",
    "conv2d_rp_kind": "(weight_shape)",
    "conv2d_rp_supported": "(kind, cin, cout)",
    "conv2d_rp_pack": "(weight, kind)",
    "conv2d_rp_forward": "(x, packed, bias, cout, kind)",
    "conv2d_rp_backward": "(x, dy, packed, x_shape, kind, has_bias, want_dx=True, want_dw=True, want_db=True)",
}


def test_the_public_functions_keep_their_signatures():
    assert len(SIGNATURES) == 13
    assert {n: str(inspect.signature(getattr(ops, n))) for n in SIGNATURES} == SIGNATURES
