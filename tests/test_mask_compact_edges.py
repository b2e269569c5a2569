"""k_mask_compact at its edges: point counts around a wavefront, a workgroup and the multi-point loop (1, 255, 257, 2049, 6149)
through kpn_query with `valid` in both modes, and ray-ordered points with 1, 3, 64 and 65 samples per ray (the ray index at sizes
that are no power of two) through a render with stages, at 1 and 3 source views.

Against the oracle: the validity bits are equal; a masked point's row is the reference's constant pair exactly, with the plain
average of the sampled source colours behind it in kpn_query (within the bar of the valid rows: it is an average of bilinear
taps, no constant) and zeros in a render pass, which never looks at a masked point's colour; valid rows stay within the 1e-5 the
stage tests use.
Every output is pre-filled with NaN, so a row that nobody wrote fails the comparison.  The same cases on the emulator build and,
under the gpu marker, on the device."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle

BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
BAR = 1e-5                                       # tests/test_kernels_simt.py test_field_kernels_vs_golden_and_oracle
COUNTS = [1, 255, 257, 2049, 6149]
# (Sc, Sf, lattice on the 16 x 16 target): the coarse pass has Sc samples per ray, the fine pass evaluates the Sf new ones
RENDERS = [(3, 1, (0, 0, 1, 16, 16)), (64, 65, (5, 5, 6, 2, 2)), (65, 64, (5, 5, 6, 2, 2))]


@functools.lru_cache(maxsize=None)
def world(V):
    from keypointnerf_amd.synthetic import make_scene
    from tests.golden_io import load_weights
    sd = load_weights()                          # the weights the bar was set with
    scene = make_scene(n_views=V, src_hw=(64, 64), tar_hw=(16, 16), mask="ellipsoid", seed=1, tar_focal_at_512=800.0)
    return scene, sd, oracle.OracleScene(scene), oracle.flat_weights(sd)


@functools.lru_cache(maxsize=None)
def backend_scene(backend, V):
    scene, sd, _, _ = world(V)
    if backend == "emu":
        from tests import simt_harness as sh
        L = sh.simt_lib()
        return sh, L, sh.HostScene(L, scene), sh.pack_weights(L, sd)
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from keypointnerf_amd import ops
    from keypointnerf_amd.synthetic import to_device
    s = to_device(scene, "cuda")
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    return ops, s, ps, ops.PackedWeights(sd)


def query(backend, V, pts, view, mode):
    """-> out (N, 5) pre-filled with NaN, valid (N,) bool"""
    if backend == "emu":
        sh, L, hs, packed = backend_scene(backend, V)
        return sh.query(L, hs, packed, pts, view, mode=mode)
    ops, _, ps, w = backend_scene(backend, V)
    out, valid = ops.query(ps, w, torch.from_numpy(pts).cuda()[None], torch.from_numpy(view).cuda()[None], mode=mode)
    return out[0].cpu().numpy(), valid.reshape(-1).cpu().numpy()


def render_stages(backend, V, grid, Sc, Sf):
    scene = world(V)[0]
    if backend == "emu":
        sh, L, hs, packed = backend_scene(backend, V)
        return sh.render(L, hs, packed, scene["cam_tar"], scene["bounds"], grid, Sc, Sf, stages=True)[1]
    ops, s, ps, w = backend_scene(backend, V)
    _, st = ops.render_rays(ps, w, s["cam_tar"], s["bounds"], grid=grid, n_coarse=Sc, n_fine=Sf, stages=True)
    return {k: v.cpu().numpy() for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def points(V, N):
    """seeded points in the scene's box blown up 2.2 times about its centre (most fall outside a view or off the foreground), random
    unit view directions, and the oracle's results in both modes"""
    scene, _, osc, wflat = world(V)
    rng = np.random.default_rng(6000 + 10 * N + V)
    b = np.asarray(scene["bounds"], np.float32).reshape(2, 3)
    c, h = 0.5 * (b[0] + b[1]), 0.5 * (b[1] - b[0])
    pts = (c + 2.2 * h * (2.0 * rng.random((N, 3), dtype=np.float32) - 1.0)).astype(np.float32)
    if N == 1:
        pts[0] = c
    view = rng.standard_normal((N, 3)).astype(np.float32)
    view /= np.linalg.norm(view, axis=-1, keepdims=True)
    refs = {mode: oracle.query(osc, wflat, pts, view, apply_eval_func=bool(mode)) for mode in (0, 1)}
    return pts, np.ascontiguousarray(view), refs


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", COUNTS)
def test_query_counts_against_the_oracle(backend, V, mode, N):
    pts, view, refs = points(V, N)
    ref, rvalid = refs[mode]
    out, valid = query(backend, V, pts, view, mode)
    assert np.array_equal(valid, rvalid)
    if N >= 255:
        assert rvalid.any() and (~rvalid).sum() > 64       # whole wavefronts of masked rows, and pieces next to valid ones
    m = ~rvalid
    assert np.array_equal(bits(out[m][:, :2]), bits(ref[m][:, :2]))
    d_rgb = float(np.abs(out[m][:, 2:] - ref[m][:, 2:]).max()) if m.any() else 0.0
    d_valid = float(np.abs(out - ref)[rvalid].max()) if rvalid.any() else 0.0
    print(f"[mask compact] N={N} V={V} mode={mode}: {int(rvalid.sum())} valid; masked rgb max diff {d_rgb:.2e}, valid rows {d_valid:.2e} (bar {BAR:g})")
    assert d_rgb < BAR and d_valid < BAR                  # (NaN where a row was not written: not < BAR)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("Sc,Sf,grid", RENDERS)
def test_ray_ordered_points_against_the_oracle(backend, V, Sc, Sf, grid):
    scene, _, osc, wflat = world(V)
    st = render_stages(backend, V, grid, Sc, Sf)
    const = np.array([0.0, np.float32(0.1) / np.float32(scene["cam"]["nml_scale"])], np.float32)
    n_masked = n_valid = 0
    for zk, qk in (("z_coarse", "rgba_coarse"), ("z_fine", "rgba_fine")):
        z, q = st[zk], st[qk].reshape(-1, 5)
        dirs = np.repeat(st["dirs"][:, None, :], z.shape[1], 1)
        pts = (st["cam_pos"][None, None, :] + dirs * z[..., None]).astype(np.float32)       # fp32: one product, one sum, as the kernel
        ref, rvalid = oracle.query(osc, wflat, pts.reshape(-1, 3), dirs.reshape(-1, 3), apply_eval_func=True)
        m = ~rvalid
        assert np.array_equal(bits(ref[m][:, :2]), bits(np.broadcast_to(const, (int(m.sum()), 2))))
        assert np.array_equal(bits(q[m][:, :2]), bits(ref[m][:, :2])) and (bits(q[m][:, 2:]) == 0).all(), qk
        assert np.abs(q - ref)[rvalid][:, :2].max(initial=0.0) < BAR, qk
        lit = rvalid & (ref[:, 0] > 0) & (q[:, 0] > 0)       # a point of zero density contributes 0 * rgb: its colour may be skipped
        assert np.abs(q - ref)[lit].max(initial=0.0) < BAR, qk
        assert not np.isnan(q[rvalid]).any()
        n_masked, n_valid = n_masked + int(m.sum()), n_valid + int(rvalid.sum())
    assert n_masked > 0 and n_valid > 0
