"""Pins the workspace and kept-state sizes of the field, backward and render entry points: callers allocate by these numbers and
the layouts behind them are shared by several entry points, so a refactor of the host code must not move them.  CPU only: the size
functions make no HIP call, so the device library answers without a GPU (as in test_library_abi.py).

EXPECTED was read from the two libraries of the commit before the layouts were composed from shared blocks ("Give the field, backward
and render host path named arguments and one layout"), at each library's default row-scratch cap and rows mode 3."""
import ctypes

import pytest

from keypointnerf_amd import lib as kl

# V, N points (the four per-point-count functions), nx x ny rays at Sc + Sf samples, fine, chunk_rays (the three per-render functions)
CASES = [
    dict(V=1, N=1, nx=5, ny=1, Sc=3, Sf=1, fine=1, chunk_rays=0),                  # the smallest of everything
    dict(V=3, N=1000, nx=64, ny=64, Sc=64, Sf=64, fine=1, chunk_rays=0),           # the shipped shape, one chunk
    dict(V=3, N=1000, nx=64, ny=64, Sc=64, Sf=64, fine=0, chunk_rays=0),           # coarse only: no train layouts
    dict(V=4, N=4097, nx=100, ny=7, Sc=128, Sf=128, fine=1, chunk_rays=48),        # 14 chunks of 48 rays and a last one of 28
    dict(V=3, N=100000, nx=333, ny=3, Sc=70, Sf=66, fine=1, chunk_rays=100),       # the emulator's 1 MiB cap: 49 batches per query
    dict(V=3, N=20000000, nx=512, ny=512, Sc=64, Sf=64, fine=1, chunk_rays=0),     # the device build's 3 GiB cap: several batches
    dict(V=4, N=2000000000, nx=2048, ny=1, Sc=128, Sf=128, fine=0, chunk_rays=0),  # more tiles than 60 batches of the cap hold
    dict(V=1, N=262145, nx=300, ny=300, Sc=128, Sf=128, fine=1, chunk_rays=0),     # one point beyond a backward pass; chunk capped by it
]
FUNCTIONS = ["kpn_query_workspace_bytes", "kpn_geo_rows_backward_workspace_bytes", "kpn_query_backward_geometry_workspace_bytes",
             "kpn_query_backward_workspace_bytes", "kpn_render_workspace_bytes", "kpn_render_rays_train_backward_workspace_bytes",
             "kpn_render_rays_train_state_bytes"]
DEFAULT_CAP = {"emulator": 1 << 20, "device": 3072 << 20}
# per library and case: the seven sizes in FUNCTIONS order
EXPECTED = {
    "emulator": [
        [20992, 1968640, 2036480, 2132992, 25088, 2150912, 28416],
        [993280, 15008000, 18358528, 27427072, 27509504, 6578206464, 36917504],
        [993280, 15008000, 18358528, 27427072, 14370560, 0, 0],
        [2648320, 72651264, 88535808, 137147136, 3090176, 408190208, 87443456],
        [2376448, 1288631296, 1615831296, 2501431296, 2491392, 344795904, 45867520],
        [401345792, 3375100160, 4232835328, 6554382592, 1758627072, 6583367424, 2362704128],
        [50800015872, 4499173632, 5507903744, 8594911488, 15683328, 0, 0],
        [3593728, 1126953216, 1682698496, 2473324800, 1056123648, 2496004096, 1281391104],
    ],
    "device": [
        [20992, 312613376, 312681216, 312777728, 25088, 312795648, 28416],
        [993280, 325652736, 329003264, 338071808, 524470784, 7137331712, 782328064],
        [993280, 325652736, 329003264, 338071808, 262851072, 0, 0],
        [5319168, 383296000, 399180544, 447791872, 16238336, 731983104, 363554816],
        [96802304, 1599276032, 1926476032, 2812076032, 13627648, 666576896, 205045760],
        [3319515648, 3685744896, 4543480064, 6865027328, 4459010048, 7142492672, 50068979968],
        [50800015872, 4809818368, 5818548480, 8905556224, 346647040, 0, 0],
        [153113088, 1437597952, 1993343232, 2783969536, 4094886144, 2890162944, 12274694656],
    ],
}


def _library(kind):
    if kind == "emulator":
        from tests import simt_harness as sh
        return sh.simt_lib()
    from keypointnerf_amd import build as kb
    kb.build(verbose=False)
    return kl.get_library()


def sizes(L, case):
    keep = (ctypes.c_float * 16)()   # stands for every tensor: the size functions check pointers for null and never follow them
    d = kl.SceneDesc()
    d.n_views, d.src_h, d.src_w, d.geo0_h, d.geo0_w, d.geo1_h, d.geo1_w, d.tex_h, d.tex_w = case["V"], 64, 64, 32, 32, 64, 64, 32, 32
    d.znear, d.zfar, d.nml_scale, d.sigma = 1.0, 2.0, 1.0, 0.1
    for k in ("KRT", "extrin", "kpt3d", "img", "fg_mask", "geo0", "geo1", "tex"):
        setattr(d, k, ctypes.addressof(keep))
    a = kl.RenderArgs()
    a.K = a.RT = a.bounds = ctypes.addressof(keep)
    a.step, a.nx, a.ny, a.n_coarse, a.n_fine, a.fine, a.chunk_rays = 1, case["nx"], case["ny"], case["Sc"], case["Sf"], case["fine"], case["chunk_rays"]
    out = [int(getattr(L, f)(case["N"], case["V"])) for f in FUNCTIONS[:4]]
    return out + [int(getattr(L, f)(ctypes.byref(d), ctypes.byref(a))) for f in FUNCTIONS[4:]]


@pytest.mark.parametrize("kind", ["emulator", "device"])
def test_workspace_and_state_sizes_are_pinned(kind):
    L = _library(kind)
    cap, rows_mode = L.kpn_row_scratch_cap_bytes(), L.kpn_get_geo_rows_mode()
    try:   # the process-wide settings the layouts depend on, at their defaults whatever an earlier test left
        L.check(L.kpn_set_row_scratch_cap_bytes(DEFAULT_CAP[kind]))
        L.check(L.kpn_set_geo_rows_mode(3))
        got = [sizes(L, case) for case in CASES]
    finally:
        L.check(L.kpn_set_row_scratch_cap_bytes(cap))
        L.check(L.kpn_set_geo_rows_mode(rows_mode))
    for case, g, e in zip(CASES, got, EXPECTED[kind]):
        assert g == e, (kind, case, dict(zip(FUNCTIONS, zip(g, e))))
    # every branch the cases are there for was taken: the train layouts exist exactly where the call is coarse + fine
    assert all((g[5] > 0 and g[6] > 0) == bool(case["fine"]) and min(g[:5]) > 0 for case, g in zip(CASES, got))
