"""Test infrastructure of the fp16 range guard (keypointnerf_amd/csrc/api_field.hip run_field, kpn_field_shared.h kpn_batch_gate /
kpn_batch_range, the three atomicOr(batch.bad, 1) sites of field_kernels.hip): the inputs and the checks, written once against a small
driver that the emulator build (tests/test_range_guard_cpu.py) and the product library (tests/test_gpu_range_guard.py) both provide.

The default field kernels (rows mode 3, fuse mode 1) carry every operand as two fp16 pieces.  They stand aside when a weight or a map
is beyond fp16's range, the per-point kernel flags a batch that produced a non-finite value, and either way the fp32-range kernels
launched behind them evaluate that batch again.  A redo that did not happen, or one that read stale scratch, gives a finite but wrong
frame: every check here compares bits with the SAFE run (the same call with rows mode 2 + fuse mode 0 selected: the very launches of a
redo) and looks at kpn_range_guard_count; the RAW run (kpn_set_range_guard(0)) shows that the input does overflow.

Which branch of run_field (api_field.hip) each check pins:
  check_density_first      282 `split`, 297 launch_density_first, 305 `if (split) launch_records(r_rows)`, 304 / 306 the redo on
                           `slots + 4` over the latents pass A left in slabs 0..3; pass A's flag (field_kernels.hip 651) for the
                           activation input, pass B's alone (799) for the colour input
  check_one_flagged_batch  284-286 the per-batch flag `slots + 6`, 303 / 306 the redo of batch b under the SAME flag and the same
                           kpn_batch_range as the first launches (kpn_query: not lean, 817)
  check_batched_render     284-308 with L.nbatch > 1 in a render pass, fused and density first (the live list of ONE batch)
  check_query              kpn_query (api_field.hip 393-406): modes 0 and 1, `valid` written, no zero-density short path (278)
  check_per_call_kernels   256 / 257 selected_rows_mode / selected_fuse_mode, 262 the ROWS layout under a process-wide rows mode 0,
                           273-276 `guard` / `guarded` for the mixed pairs, 275 safe_rmode
  check_train              api_render.hip 176 (allow_pool = false) and 334 (keep_rows): the forward, and the rows the backward reads

A driver has: lib (the C ABI: settings and counters), emulated, batch_points (kUncappedPoints of the build), stream(), scene(dict),
weights(state dict), render(...), query(...), train_forward(...), train_backward(...); arrays in and out are numpy, images as
(3, ny, nx) / (ny, nx), train outputs as (3, R) / (R,).
"""
import contextlib
import ctypes
import functools

import numpy as np

from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict

SC, SF = 12, 8                     # samples of every render here: coarse + fine
OVERFLOWS = ("map", "weight", "activation", "colour")
DEFAULTS = (3, 1, 2, 1)            # rows mode, fuse mode, density first (auto), range guard
ORACLE_SANITY = 2e-3               # tests/test_kernels_simt.py::test_range_guard_of_the_fp16_kernels: deliberately ill-scaled networks
GRAD_RTOL, GRAD_ATOL = 2e-4, 1e-6  # test_backward_multi_pass_and_chunking: two backward runs whose row order differs
# the density head's bias of the worlds whose redone batch must hold dead AND live points (tests/test_gpu_soak.py's use of it): measured
# on the emulator, 10 x 10 rays at 12 + 8 samples, (listed, live) points of the safe frame: bias 0: base and colour (616, 616), map
# (605, 401), activation (611, 491); bias -20: base and colour (620, 313), map and activation as before
DENSITY_BIAS = -20.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# inputs
def _scaled(sd, key, f):
    out = {k: v.clone() for k, v in sd.items()}
    out[key] = sd[key] * f
    return out


@functools.lru_cache(maxsize=None)
def inputs(tar_hw=(10, 10), mask="ellipsoid", density_bias=0.0):
    """name -> (scene, state dict): the in-range base, the four overflow inputs of the emulator guard test, and the base scene with ONE
    hot pixel in feat_geo[0] (every channel x 1e3: points that project near it overflow an activation, nothing stands aside)"""
    scene = make_scene(n_views=3, src_hw=(64, 64), tar_hw=tar_hw, mask=mask, seed=2, tar_focal_at_512=800.0)
    sd = random_hotpath_state_dict(seed=3, density_bias=density_bias)
    big, hot = dict(scene), dict(scene)
    g0 = scene["feat_geo"][0].clone(); g0[:, 5] *= 1.0e5
    big["feat_geo"] = [g0, scene["feat_geo"][1]]
    h0 = scene["feat_geo"][0].clone()
    H, W = h0.shape[-2:]
    h0[:, :, H // 2 - 2, W // 2] *= 1.0e3
    hot["feat_geo"] = [h0, scene["feat_geo"][1]]
    return {"base": (scene, sd), "map": (big, sd), "hot pixel": (hot, sd),
            "weight": (scene, _scaled(sd, "mlp_geo.layers1.layers.1.linear.weight_g", 2048.0)),
            "activation": (scene, _scaled(sd, "mlp_geo.layers1.layers.0.linear.weight_g", 300.0)),
            "colour": (scene, _scaled(sd, "mlp_tex.ray_encoder.2.weight", 3.0e3))}


class World:
    """The inputs on one backend: scene and weight handles made once, the safe frames computed once and handed out unchanged."""

    def __init__(self, drv, **kw):
        self.drv, self.inp = drv, inputs(**kw)
        self._scenes, self._weights, self._safe = {}, {}, {}

    def get(self, name):
        """-> (scene handle, weights handle, scene dict)"""
        scene, sd = self.inp[name]
        if id(scene) not in self._scenes:
            self._scenes[id(scene)] = self.drv.scene(scene)
        if id(sd) not in self._weights:
            self._weights[id(sd)] = self.drv.weights(sd)
        return self._scenes[id(scene)], self._weights[id(sd)], scene

    def render(self, name, fine=True, **kw):
        hs, w, scene = self.get(name)
        nx, ny = scene["cam_tar"]["width"], scene["cam_tar"]["height"]
        return self.drv.render(hs, w, scene, (0, 0, 1, nx, ny), SC, SF, fine=fine, **kw)

    def safe_frame(self, name, fine=True):
        """-> (the frame in rows mode 2 + fuse mode 0, (listed, live) points its per-point kernel looked at)"""
        if (name, fine) not in self._safe:
            with settings(self.drv.lib, rows=2, fuse=0):
                density_stats(self.drv)
                frame = self.render(name, fine=fine)
                self._safe[name, fine] = (frame, density_stats(self.drv))
        frame, stats = self._safe[name, fine]
        return {k: v.copy() for k, v in frame.items()}, stats


# ------------------------------------------------------------------------------------------------
# settings and counters of the C ABI
def assert_defaults(lib):
    assert (lib.kpn_get_geo_rows_mode(), lib.kpn_get_fuse_mode(), lib.kpn_get_density_first(), lib.kpn_get_range_guard()) == DEFAULTS


@contextlib.contextmanager
def settings(lib, rows=None, fuse=None, density_first=None, guard=None, cap=None):
    """process-wide settings for the block, whatever was set before restored behind it"""
    setters = (lib.kpn_set_geo_rows_mode, lib.kpn_set_fuse_mode, lib.kpn_set_density_first, lib.kpn_set_range_guard,
               lib.kpn_set_row_scratch_cap_bytes)
    old = (lib.kpn_get_geo_rows_mode(), lib.kpn_get_fuse_mode(), lib.kpn_get_density_first(), lib.kpn_get_range_guard(),
           lib.kpn_row_scratch_cap_bytes())
    try:
        for setter, v in zip(setters, (rows, fuse, density_first, guard, cap)):
            if v is not None:
                lib.check(setter(v))
        yield
    finally:
        for setter, v in zip(setters, old):
            lib.check(setter(v))


def guard_count(drv):
    n = ctypes.c_int64(-1)
    drv.lib.check(drv.lib.kpn_range_guard_count(drv.stream(), ctypes.byref(n)))
    return int(n.value)


def density_stats(drv):
    """(listed, live) points the render passes' per-point kernels looked at since the last call; resets"""
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    drv.lib.check(drv.lib.kpn_density_stats(drv.stream(), ctypes.byref(a), ctypes.byref(b), 1))
    return int(a.value), int(b.value)


def pass_forms(lib):
    """(density first, fused) eligible render passes since the last call; resets"""
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    lib.check(lib.kpn_density_first_passes(ctypes.byref(a), ctypes.byref(b), 1))
    return int(a.value), int(b.value)


def assert_same_frame(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.isfinite(got[k]).all(), (what, k)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, int((bits(got[k]) != bits(want[k])).sum()))


def all_finite(frame):
    return all(np.isfinite(v).all() for v in frame.values())


# ------------------------------------------------------------------------------------------------
# 1. density first and the guard
def check_density_first(world, name, mode):
    """An overflow input rendered with kpn_set_density_first(mode): the passes took that form, the frame is the safe frame bit for bit,
    the counter moved — and the redone batch held dead and live points, so that "gather records for the live points only" matters."""
    drv = world.drv
    assert_defaults(drv.lib)
    want, (listed, live) = world.safe_frame(name)
    print(f"[{name}] safe frame: {listed} listed, {live} live points")
    assert listed > live > 0, (name, listed, live)
    with settings(drv.lib, density_first=mode):
        pass_forms(drv.lib)
        c0 = guard_count(drv)
        got = world.render(name)
        moved = guard_count(drv) - c0
        forms = pass_forms(drv.lib)
    assert forms == ((2, 0) if mode == 1 else (0, 2)), (name, mode, forms)   # the coarse pass and the fine pass's new samples
    assert_same_frame(got, want, (name, mode))
    assert moved > 0, (name, mode)
    assert_defaults(drv.lib)


def check_colour_overflows_in_pass_b_only(world):
    """what makes the colour input a test of pass B's flag: with density first on and the guard off the densities are finite (pass A
    saw nothing) and the colours are not"""
    drv = world.drv
    with settings(drv.lib, density_first=1, guard=0):
        pass_forms(drv.lib)
        raw = world.render("colour")
        assert pass_forms(drv.lib) == (2, 0)
    assert np.isfinite(raw["alpha"]).all() and np.isfinite(raw["alpha_fine"]).all()
    assert not (np.isfinite(raw["tex_fg"]).all() and np.isfinite(raw["tex_fg_fine"]).all())
    assert_defaults(drv.lib)


def check_base_frame(world):
    """in range: the counter stays put in both forms, and both give the same bits"""
    drv = world.drv
    assert_defaults(drv.lib)
    frames = []
    for mode in (0, 1):
        with settings(drv.lib, density_first=mode):
            pass_forms(drv.lib)
            c0 = guard_count(drv)
            frames.append(world.render("base"))
            assert guard_count(drv) == c0, mode
            assert pass_forms(drv.lib) == ((2, 0) if mode == 1 else (0, 2)), mode
    assert_same_frame(frames[1], frames[0], "base")
    assert_defaults(drv.lib)


# ------------------------------------------------------------------------------------------------
# 2. several batches, one of them flagged (kpn_query, mode 1)
def _random_points(scene, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = scene["bounds"].reshape(2, 3).numpy().astype(np.float32)
    pts = (lo + (hi - lo) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
    view = rng.standard_normal((n, 3)).astype(np.float32)
    view /= np.linalg.norm(view, axis=-1, keepdims=True)
    return pts, view


def check_one_flagged_batch(world, n_candidates, n_valid, cap=None):
    """Points of which at most 150 overflow, all among the first 256 (one workgroup of k_mask_compact: contiguous in the valid list),
    in a pass of several batches: only the flagged batch is evaluated again, the others keep the two-fp16-piece kernels' bits.
    n_candidates random points are classified with a raw query, n_valid valid ones kept; cap: the row scratch cap of the calls."""
    drv = world.drv
    assert_defaults(drv.lib)
    hs, w, scene = world.get("hot pixel")
    hs_map, w_map, _ = world.get("map")
    cand, cview = _random_points(scene, n_candidates, seed=7)
    with settings(drv.lib, guard=0, cap=cap):
        raw0, valid0 = drv.query(hs, w, cand, cview, 1)
    hot0 = valid0 & ~np.isfinite(raw0).all(-1)
    cool0 = valid0 & ~hot0
    print(f"candidates: {n_candidates}, valid {int(valid0.sum())}, hot {int(hot0.sum())}")
    assert hot0.sum() >= 150 and cool0.sum() >= n_valid - 150 and (~valid0).sum() >= 64
    order = np.concatenate([np.nonzero(hot0)[0][:150], np.nonzero(cool0)[0][:n_valid - 150], np.nonzero(~valid0)[0][:64]])
    pts, view = cand[order], cview[order]
    with settings(drv.lib, cap=cap):
        c0 = guard_count(drv)
        got, v_got = drv.query(hs, w, pts, view, 1)
        d = guard_count(drv) - c0
        _, v_map = drv.query(hs_map, w_map, pts, view, 1)      # every batch stands aside: the number of batches of this pass
        nb = guard_count(drv) - c0 - d
        with settings(drv.lib, guard=0):
            raw, v_raw = drv.query(hs, w, pts, view, 1)
        with settings(drv.lib, rows=2, fuse=0):
            safe, v_safe = drv.query(hs, w, pts, view, 1)
    print(f"valid {int(v_got.sum())} of {len(pts)}: {nb} batches, {d} evaluated again")
    assert np.isfinite(got).all()
    assert np.array_equal(v_got, v_raw) and np.array_equal(v_got, v_safe) and np.array_equal(v_got, v_map)
    assert np.array_equal(v_got, valid0[order])
    eq_raw, eq_safe = (bits(got) == bits(raw)).all(-1), (bits(got) == bits(safe)).all(-1)
    assert (eq_raw | eq_safe).all(), int((~(eq_raw | eq_safe)).sum())
    bad_raw = ~np.isfinite(raw).all(-1)
    assert eq_safe[bad_raw].all()
    assert bad_raw.any() and np.nonzero(bad_raw)[0].max() < 256          # the construction
    took_raw, took_safe = v_got & eq_raw & ~eq_safe, v_got & eq_safe & ~eq_raw
    print(f"rows with the fp16 kernels' bits only: {int(took_raw.sum())}, with the fp32-range kernels' only: {int(took_safe.sum())}")
    assert took_raw.any() and took_safe.any()
    assert 1 <= d < nb, (d, nb)
    assert took_safe.sum() <= d * drv.batch_points                       # d * tiles_cap * 32
    assert_defaults(drv.lib)


# ------------------------------------------------------------------------------------------------
# 3. several batches in a render pass, fused and density first
def check_batched_render(world, cap=None, oracle_stride=1):
    """A coarse-only render whose pass is cut into T >= 2 batches (the map input moves the counter by T).  map: the safe frame bit for
    bit in both forms.  activation: finite, at least one batch evaluated again, near the oracle (the batches that were not flagged
    keep the two-fp16-piece kernels' bits: no bit claim).  oracle_stride: the oracle renders every n-th ray (rays are independent).
    Measured on the MI355X, dense mask, every 17th ray: the worst ray is 8.0e-4 from the oracle at 256 x 256 and 8.2e-4 at 224 x 224
    (plain fp32 kernels, rows mode 0 + fuse mode 0: 1.4e-3 and 3.0e-4).  At 320 x 320 ONE ray of 6024 is 4.2e-3 off with every batch
    evaluated again and the frame bit-equal to the safe frame, and 2.5e-3 off with the plain fp32 kernels: that ray under a layer 300 x
    its size, not the guard — the bound is a sanity bound on an ill-scaled network, so the device frame is the smallest one whose pass
    is sure to need two batches, not a larger one."""
    from oracle import oracle
    drv = world.drv
    assert_defaults(drv.lib)
    scene_a, sd_a = world.inp["activation"]
    nx, ny = scene_a["cam_tar"]["width"], scene_a["cam_tar"]["height"]
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    pix = np.stack([xx.reshape(-1), yy.reshape(-1)], -1).astype(np.int32)[::oracle_stride]
    ref = oracle.render_rays(oracle.OracleScene(scene_a), oracle.flat_weights(sd_a), scene_a["cam_tar"], scene_a["bounds"], pix, SC, SF,
                             fine=False)
    with settings(drv.lib, cap=cap):
        want, _ = world.safe_frame("map", fine=False)
        for mode in (0, 1):
            with settings(drv.lib, density_first=mode):
                pass_forms(drv.lib)
                c0 = guard_count(drv)
                got = world.render("map", fine=False)
                T = guard_count(drv) - c0
                assert pass_forms(drv.lib) == ((1, 0) if mode == 1 else (0, 1)), mode
                print(f"density first {mode}: the pass ran in {T} batches")
                assert T >= 2, (mode, T)
                assert_same_frame(got, want, ("map", mode))
                c0 = guard_count(drv)
                act = world.render("activation", fine=False)
                d = guard_count(drv) - c0
                print(f"density first {mode}: activation input, {d} of {T} batches evaluated again")
                assert all_finite(act) and 1 <= d <= T, (mode, d, T)
                e_rgb = np.abs(act["tex_fg"].transpose(1, 2, 0).reshape(-1, 3)[::oracle_stride] - ref["tex_fg"]).max()
                e_a = np.abs(act["alpha"].reshape(-1)[::oracle_stride] - ref["alpha"]).max()
                print(f"density first {mode}: |rgb - oracle| {e_rgb:.2e}, |alpha - oracle| {e_a:.2e}")
                assert e_rgb < ORACLE_SANITY and e_a < ORACLE_SANITY, (mode, e_rgb, e_a)
    assert_defaults(drv.lib)


# ------------------------------------------------------------------------------------------------
# 4. kpn_query
QUERY_POINTS = 2049    # one more than a multi-point loop of k_mask_compact covers


def check_query(world, name, mode):
    drv = world.drv
    assert_defaults(drv.lib)
    hs, w, scene = world.get(name)
    pts, view = _random_points(scene, QUERY_POINTS, seed=11)
    c0 = guard_count(drv)
    got, v_got = drv.query(hs, w, pts, view, mode)
    assert guard_count(drv) > c0, (name, mode)
    with settings(drv.lib, rows=2, fuse=0):
        safe, v_safe = drv.query(hs, w, pts, view, mode)
    with settings(drv.lib, guard=0):
        raw, _ = drv.query(hs, w, pts, view, mode)
    assert np.isfinite(got).all(), (name, mode)
    assert 0 < v_got.sum() < QUERY_POINTS and np.array_equal(v_got, v_safe)
    assert np.array_equal(bits(got), bits(safe)), (name, mode, int((bits(got) != bits(safe)).any(-1).sum()))
    assert not np.isfinite(raw).all(), (name, mode)
    assert_defaults(drv.lib)


# ------------------------------------------------------------------------------------------------
# 5. per-call kernel selection under a process-wide rows mode 0 + fuse mode 0
COMPARATOR = ("bf16x3", "f32")
PLAN_CASES = (("map", ("f16x2", "f16x2")), ("map", ("f16x2", "f32")), ("map", ("bf16x3", "f16x2")),
              ("activation", ("f16x2", "f32")), ("colour", ("bf16x3", "f16x2")))


def check_per_call_kernels(world, name, plan):
    drv = world.drv
    assert_defaults(drv.lib)
    with settings(drv.lib, rows=0, fuse=0):
        c0 = guard_count(drv)
        want = world.render(name, rows_kernel=COMPARATOR[0], fuse_kernel=COMPARATOR[1])
        assert guard_count(drv) == c0, name                    # nothing of this plan stands under the guard
        got = world.render(name, rows_kernel=plan[0], fuse_kernel=plan[1])
        moved = guard_count(drv) - c0
    assert_same_frame(got, want, (name, plan))
    assert moved > 0, (name, plan)
    assert_defaults(drv.lib)


# ------------------------------------------------------------------------------------------------
# 6. train branch
class TrainDraws:
    """36 rays (a 6 x 6 patch of the 10 x 10 target), 8 + 8 samples, recorded draws, view dropout, density noise"""

    def __init__(self):
        rng = np.random.default_rng(21)
        self.Sc = self.Sf = 8
        yy, xx = np.meshgrid(np.arange(6) + 2, np.arange(6) + 2, indexing="ij")
        self.pix = np.stack([xx.reshape(-1), yy.reshape(-1)], -1).astype(np.int32)
        R = self.R = self.pix.shape[0]
        self.u_c, self.u_f = rng.random((R, self.Sc), dtype=np.float32), rng.random((R, self.Sf), dtype=np.float32)
        self.n_c = rng.standard_normal(R * self.Sc).astype(np.float32)
        self.n_f = rng.standard_normal(R * (self.Sc + self.Sf)).astype(np.float32)
        self.keep_c, self.keep_f, self.std = 0b111, 0b101, 0.01
        self.grads = {k: (rng.standard_normal((3, R)) if k.startswith("tex") else rng.standard_normal(R)).astype(np.float32) / R
                      for k in ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf")}


def check_train(world, name, keep_state=False):
    """render_rays_train under the default modes: the safe forward bit for bit, the counter moved, NaN without the guard; then the
    backward, whose forward recompute (or kept state) must hold the fp32-range rows: finite and within the bar of two backward runs
    whose row order differs of the backward in the safe modes.  keep_state: forward with a kept state + the kept-state backward too,
    the kept and the not-kept forward bit-equal."""
    drv = world.drv
    assert_defaults(drv.lib)
    hs, w, scene = world.get(name)
    d = TrainDraws()
    c0 = guard_count(drv)
    got, _ = drv.train_forward(hs, w, scene, d)
    assert guard_count(drv) > c0, name
    with settings(drv.lib, rows=2, fuse=0):
        want, _ = drv.train_forward(hs, w, scene, d)
        ref = drv.train_backward(hs, w, scene, d)
    with settings(drv.lib, guard=0):
        raw, _ = drv.train_forward(hs, w, scene, d)
    assert_same_frame(got, want, name)
    assert not all_finite(raw), name
    print(f"[{name}] max |gradient| of the safe backward, per block: " + ", ".join(f"{float(np.abs(r).max()):.2e}" for r in ref))
    assert np.abs(ref[0]).max() > 0                   # (a saturated density leaves the texture map's gradient at zero)
    runs = [("repeating the forward", drv.train_backward(hs, w, scene, d))]
    if keep_state:
        c0 = guard_count(drv)
        kept, state = drv.train_forward(hs, w, scene, d, keep_state=True)
        assert guard_count(drv) > c0, name
        assert_same_frame(kept, got, (name, "kept state"))
        runs.append(("kept state", drv.train_backward(hs, w, scene, d, state=state)))
    for what, grads in runs:
        for i, (g, r) in enumerate(zip(grads, ref)):
            err, bar = float(np.abs(g - r).max()) if np.isfinite(g).all() else float("inf"), GRAD_RTOL * float(np.abs(r).max()) + GRAD_ATOL
            print(f"[{name}, {what}] gradient block {i}: |got - safe| {err:.2e}, bar {bar:.2e}")
            assert np.isfinite(g).all(), (name, what, i)
            assert err <= bar, (name, what, i, err, bar)
    assert_defaults(drv.lib)
