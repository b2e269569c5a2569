"""Test infrastructure of the ray-stage kernels (keypointnerf_amd/csrc/ray_kernels.hip): the cases, their references, the bars and
one driver of the C ABI that runs on host arrays (the emulator build) and on device tensors (the product library) alike.

1. kpn_rgba2out_backward at every specialisation (<1>, <2>, <4>, <8> samples per lane, one thread per ray beyond 512 samples)
   against a division-free restatement of the compositor differentiated by torch.autograd in fp64 on the CPU.  e_ref is the same
   restatement in fp32; the bar, per call and column group: ratio(native, fp64, e_ref) <= 4 (the project's standing rule).
2. k_fine_samples_w, the sampler inside kpn_render_rays / kpn_render_rays_train, against the stand-alone kpn_importance_sample on
   the render's own stage outputs: sort(cat(z_coarse, samples)) is bit-equal to the stage output z_fine.
3. kpn_importance_sample, kpn_ray_bbox_intersection and kpn_make_rays at their edges against the oracle.
4. the grid-stride loops of k_rgba2out and k_fine_samples_w (more rays than 4 x 8192 workgroup slots).
"""
import ctypes
import functools

import numpy as np
import torch

from keypointnerf_amd import lib as kl
from oracle import oracle
from tests.parity import CANARY, DeviceArrays, HostArrays, bits, ratio  # noqa: F401  (the runners take the array classes from here)
from tests.test_oracle_vs_golden import assert_samples_close

# e_ref is torch's fp32 on the host of the run and so moves with its torch, SIMD path and libm (measured: 9.1e-8 on one host, 2.3e-8 on
# another, same case), while the kernel's result does not: a case near the bar can flip on another host with no change to the kernel.
# The closest measured: S = 257, colour call, d sigma on the device, 3.96 (profiles/ray_stage_tests.md).
FACTOR = 4.0
CASE_C = "case_c_v3_offaxis"


def put_raw(B, a):
    """an array of any dtype (pixels are int32) on the build's side of the ABI"""
    a = np.ascontiguousarray(a)
    return a.copy() if isinstance(B, HostArrays) else torch.from_numpy(a.copy()).cuda()


# ------------------------------------------------------------------------------------------------
# 1. compositor backward
# samples per ray -> rays: 7 rays leave the last workgroup of a wavefront-per-ray kernel with three of four waves, 67 rays the
# thread-per-ray kernel with one full 64-thread block plus three
BWD_CASES = {1: 7, 2: 7, 63: 7, 64: 7,        # <1>
             65: 7, 128: 7,                   # <2>: per = 2, lanes >= 33 idle; full
             130: 7, 256: 7,                  # <4>: per = 3 under PER = 4; full
             257: 7, 512: 7,                  # <8>: per = 5 under PER = 8; full
             513: 67, 700: 67}                # one thread per ray
BWD_CALLS = {"all": ("color", "depth", "alpha", "sdf"), "color": ("color",), "alpha": ("alpha",), "depth_sdf": ("depth", "sdf")}
MIN_ALPHA = 0.5      # d_depth and d_sdf go through 1 / (alpha + 1e-8)^2: ill-conditioned on thin rays (depth_legs_conditioned)


def _exclusive_cumsum(x):
    """sum_{j<i} x_j along the last axis, one addition per sample in x's own dtype.  torch.cumsum is not used: on the CPU it accumulates
    fp32 input in fp64 (measured: 200 times closer to the fp64 sum than sequential fp32 additions over 1e5 terms), so the fp32 run of
    the restatement would not be an fp32 computation and e_ref would not hold what fp32 costs"""
    acc = torch.zeros_like(x[..., 0])
    cols = [acc]
    for i in range(x.shape[-1] - 1):
        acc = acc + x[..., i]
        cols.append(acc)
    return torch.stack(cols, -1)


def _composite(rgba, z, dtype):
    """the compositor (reference src/model.py:1162-1174) without its cumprod: T_i = exp(-exclusive_cumsum(sigma dist)), so a sample
    with a = 1 is harmless.  dist is formed in fp32 as the kernel and the reference form it, then promoted.
    -> (leaf rgba, {color, depth, alpha, sdf})"""
    zt = torch.from_numpy(z)
    dist = torch.cat([zt[:, 1:] - zt[:, :-1], torch.full_like(zt[:, :1], 1e10)], -1).to(dtype)
    q = torch.from_numpy(rgba).to(dtype).requires_grad_(True)
    tau = q[..., 0] * dist
    T = torch.exp(-_exclusive_cumsum(tau))
    w = (1.0 - torch.exp(-tau)) * T
    alpha = w.sum(-1)
    out = {"color": (q[..., 2:] * w[..., None]).sum(-2), "alpha": alpha, "sdf": (q[..., 1] * w).sum(-1) / (alpha + 1e-8),
           "depth": (zt.to(dtype) * w).sum(-1) / (alpha + 1e-8)}
    return q, out


def composite_backward(rgba, z, grads, dtype=torch.float64):
    """d rgba of the restatement by autograd; grads: {output name: upstream gradient} (a missing one is NULL) -> (R, S, 5) array"""
    if not grads:
        return np.zeros(rgba.shape, np.float64)
    q, out = _composite(rgba, z, dtype)
    names = sorted(grads)
    (d,) = torch.autograd.grad([out[k] for k in names], q, [torch.from_numpy(grads[k]).to(dtype).reshape(out[k].shape) for k in names])
    return d.numpy()


def reference_weights(rgba, z):
    """the restatement's weights w_i = a_i T_i and e_i = 1 - a_i in fp64, for the input conditions -> (w, e), both (R, S)"""
    tau = rgba[..., 0].astype(np.float64) * np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], 1e10)], -1).astype(np.float64)
    e = np.exp(-tau)
    return (1.0 - e) * np.exp(-(np.cumsum(tau, -1) - tau)), e


def depth_legs_conditioned(rgba, z):
    """The input condition of every call that passes d_depth or d_sdf, per ray, on the fp64 reference alone.
    (a) alpha >= MIN_ALPHA: the two gradients go through 1 / (alpha + 1e-8)^2.
    (b) the ray is not seen through a single partially transparent sample: a second sample holds at least 1 % of the ray's weight,
        or the heaviest sample is opaque (e <= 1e-6, nothing behind it is seen).  Where one sample holds the whole weight, depth and
        sdf are that sample's own values and d depth / d w_i = (z_i - depth) / alpha vanishes identically: what any fp32 evaluation
        returns for it is the rounding of d_depth z_i / alpha (1e-7), carried to d sigma by T_i dist_i e_i, while the fp32
        restatement is exact there because its operands are (measured at S = 2: e_ref 3.8e-9 on a gradient of 1.5, 1.8e-8 on one of
        2.8e-3), so the bar would sit at one ulp of a difference of numbers of size 3."""
    w, e = reference_weights(rgba, z)
    alpha = w.sum(-1)
    heaviest = w.argmax(-1)
    second = np.sort(w, -1)[:, -2] if w.shape[1] > 1 else np.zeros_like(alpha)
    return (alpha >= MIN_ALPHA) & ((second >= 0.01 * alpha) | (e[np.arange(len(w)), heaviest] <= 1e-6))


@functools.lru_cache(maxsize=None)
def bwd_inputs(S, well_conditioned):
    """seeded rgba (R, S, 5), z (R, S) and the four upstream gradients, built as in test_rgba2out_sample_counts_vs_oracle: densities
    from thin to opaque, 30 % exact zeros, sorted depths in [2, 5]; the last sample's density is 0 on the even rays and > 0 on the odd
    ones; ray 1 has a saturating early sample (sigma dist > 100).  The mixed set (the colour and alpha calls) also has a ray of zero
    density (2) and a thin one (3).  The well-conditioned set (every call that passes d_depth or d_sdf) meets depth_legs_conditioned
    on every ray: a ray that does not gets sigma dist = 1 on its first sample (a = 0.63) and a positive last density, so two samples
    share its weight (at S = 2 that leaves no ray with a last density of 0)."""
    R = BWD_CASES[S]
    rng = np.random.default_rng(7000 + 2 * S + int(well_conditioned))
    rgba = rng.random((R, S, 5), dtype=np.float32)
    scale = rng.random((R, 1), dtype=np.float32) * 40.0
    rgba[..., 0] *= scale
    rgba[rng.random((R, S)) < 0.3, 0] = 0.0
    z = np.ascontiguousarray(np.sort(2.0 + 3.0 * rng.random((R, S), dtype=np.float32), axis=-1))
    rgba[0::2, -1, 0] = 0.0
    rgba[1::2, -1, 0] = 0.5 + rng.random(len(rgba[1::2]), dtype=np.float32)
    if S >= 3:
        i = int(np.argmax(np.diff(z[1])[:max(1, S // 2)]))
        rgba[1, i, 0] = np.float32(150.0) / (z[1, i + 1] - z[1, i])
        assert rgba[1, i, 0] * (z[1, i + 1] - z[1, i]) > 100.0
    if not well_conditioned:
        rgba[2, :, 0] = 0.0
        rgba[3, :, 0] *= np.float32(0.01)
    else:
        bad = ~depth_legs_conditioned(rgba, z)
        rgba[bad, -1, 0] = 1.0
        if S > 1:
            rgba[bad, 0, 0] = np.float32(1.0) / (z[bad, 1] - z[bad, 0])
    grads = {"color": rng.standard_normal((R, 3), dtype=np.float32), "depth": rng.standard_normal(R, dtype=np.float32),
             "alpha": rng.standard_normal(R, dtype=np.float32), "sdf": rng.standard_normal(R, dtype=np.float32)}
    return rgba, z, grads


@functools.lru_cache(maxsize=None)
def bwd_reference(S, call):
    """-> (rgba, z, {name: upstream gradient}, fp64 d_rgba, fp32 d_rgba of the same restatement); computed once and shared"""
    legs = BWD_CALLS[call]
    rgba, z, grads = bwd_inputs(S, bool({"depth", "sdf"} & set(legs)))
    if {"depth", "sdf"} & set(legs):
        assert depth_legs_conditioned(rgba, z).all()              # the input condition, on the reference alone
    g = {k: grads[k] for k in legs}
    r64, r32 = composite_backward(rgba, z, g, torch.float64), composite_backward(rgba, z, g, torch.float32)
    r64.setflags(write=False)
    return rgba, z, g, r64, r32


def bwd_groups(d):
    """the column groups a bar is taken over: the last sample's d sigma carries the 1e10 and is compared against its own maximum"""
    return {"dsigma": d[:, :-1, 0], "dsigma_last": d[:, -1, 0], "dsdf": d[..., 1], "drgb": d[..., 2:]}


def rgba2out_backward(L, B, rgba, z, grads):
    """kpn_rgba2out_backward -> d_rgba (R, S, 5) (numpy); the output is pre-filled with NaN"""
    R, S = z.shape
    out = B.full((R, S, 5), np.nan)
    dev = {k: B.put(v) for k, v in grads.items()}
    q, zz = B.put(rgba), B.put(z)
    L.check(L.kpn_rgba2out_backward(B.ptr(q), B.ptr(zz), R, S, *[B.ptr(dev.get(k)) for k in ("color", "depth", "alpha", "sdf")], B.ptr(out),
                                    B.stream))
    return B.get(out)


def check_backward_case(L, B, S):
    """every call of one sample count against the fp64 restatement, each column group within the bar; -> {(call, group): ratio}"""
    ratios = {}
    for call in BWD_CALLS:
        rgba, z, g, r64, r32 = bwd_reference(S, call)
        got = rgba2out_backward(L, B, rgba, z, g)
        assert np.isfinite(got).all(), (S, call)
        for (name, a), f64, f32 in zip(bwd_groups(got).items(), bwd_groups(r64).values(), bwd_groups(r32).values()):
            if a.size == 0:      # S = 1 has no interior sample
                continue
            e_ref = float(np.abs(f32.astype(np.float64) - f64).max())
            r = ratio(a, f64, e_ref)
            print(f"[ray stages] backward S={S} {call} {name}: ratio {r:.3f} (e_ref {e_ref:.3e}, bar {FACTOR:g})")
            ratios[(call, name)] = r
    worst = {k: v for k, v in ratios.items() if not v <= FACTOR}
    assert not worst, (S, worst)
    return ratios


def check_backward_null_and_repeat(L, B, S):
    """all four upstream gradients NULL: exact zeros; two calls give equal bits"""
    rgba, z, g, _, _ = bwd_reference(S, "all")
    assert (rgba2out_backward(L, B, *bwd_inputs(S, False)[:2], {}) == 0.0).all()
    a, b = rgba2out_backward(L, B, rgba, z, g), rgba2out_backward(L, B, rgba, z, g)
    assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------
# 2. the render's sampler against the stand-alone one
# (Sc, Sf, lattice step) on the 24 x 24 target of case_c: 9 rays at step 8, 4 at step 12
EVAL_CASES = [(3, 1, 8), (8, 4, 8), (64, 64, 12),
              (65, 64, 12), (64, 65, 12),      # the first sizes on k_fine_samples_w<false>
              (70, 66, 12), (128, 128, 12)]
TRAIN_CASES = [(16, 16), (70, 66)]
U_ROWS = ("descending", "duplicated", "ends", "sorted", "iid")


def train_draws(Sc, Sf, seed=0):
    """pix (10, 2), u_coarse (10, Sc), u_fine (10, Sf) for case_c's 24 x 24 target; rows k and 5 + k of u_fine are of kind U_ROWS[k]:
    strictly descending (every new sample out of order: the rank-counting branch), duplicated values (equal new samples: the j < k
    tie-break), zeros and 1 - 2^-24, sorted random, iid random"""
    rng = np.random.default_rng(4100 + 100 * seed + Sc + Sf)
    pix = np.array([(x, y) for y in (0, 8, 16) for x in (0, 8, 16)] + [(12, 12)], np.int32)
    R = len(pix)
    u_c = rng.random((R, Sc), dtype=np.float32)
    u_f = rng.random((R, Sf), dtype=np.float32)
    top = np.float32(1.0) - np.float32(2.0 ** -24)
    for r in range(R):
        kind = U_ROWS[r % 5]
        if kind == "descending":
            u_f[r] = np.linspace(0.97, 0.02, Sf, dtype=np.float32)
            assert Sf == 1 or (np.diff(u_f[r]) < 0).all()
        elif kind == "duplicated":
            u_f[r] = np.repeat(u_f[r, :(Sf + 2) // 3], 3)[:Sf][rng.permutation(Sf)]
        elif kind == "ends":
            u_f[r, 0::2], u_f[r, 1::2] = 0.0, top
        elif kind == "sorted":
            u_f[r] = np.sort(u_f[r])
    return pix, u_c, u_f


def render_train_device(L, B, scene, weights, cam_tar, bounds, pix, Sc, Sf, u_c, u_f):
    """kpn_render_rays_train with kpn_render_args.stages on device tensors (keypointnerf_amd.ops does not expose the stages of the
    train call): scene an ops.PreparedScene, weights an ops.PackedWeights -> the stage arrays (numpy), every view kept, no noise"""
    R = len(pix)
    K, RT, b = (B.put(np.asarray(t, np.float32).reshape(s)) for t, s in ((cam_tar["K"], (4, 4)), (cam_tar["RT"], (4, 4)), (bounds, (2, 3))))
    o = {k: B.full((3, R), np.nan) for k in ("tex_fg", "tex_fg_fine")}
    o.update({k: B.full(R, np.nan) for k in ("depth", "alpha", "depth_fine", "alpha_fine", "sdf")})
    a = kl.RenderArgs()
    a.K, a.RT, a.bounds = K.data_ptr(), RT.data_ptr(), b.data_ptr()
    a.znear, a.zfar = float(cam_tar["znear"]), float(cam_tar["zfar"])
    a.x0, a.y0, a.step, a.nx, a.ny = 0, 0, 1, R, 1
    a.n_coarse, a.n_fine, a.fine = Sc, Sf, 1
    for k, v in o.items():
        setattr(a, k, v.data_ptr())
    st = {"z_coarse": B.full((R, Sc), np.nan), "rgba_coarse": B.full((R, Sc, 5), np.nan), "dirs": B.full((R, 3), np.nan),
          "cam_pos": B.full(3, np.nan), "z_fine": B.full((R, Sc + Sf), np.nan), "rgba_fine": B.full((R, Sc + Sf, 5), np.nan)}
    cst = kl.RenderStages()
    for k, v in st.items():
        setattr(cst, k, v.data_ptr())
    a.stages = ctypes.pointer(cst)
    draws = (put_raw(B, pix), B.put(u_c), B.put(u_f))
    t = kl.TrainArgs()
    t.pix, t.u_coarse, t.u_fine = (v.data_ptr() for v in draws)
    t.keep_coarse = t.keep_fine = (1 << scene.n_views) - 1
    nb = L.kpn_render_workspace_bytes(ctypes.byref(scene.desc), ctypes.byref(a))
    assert nb > 0, L.kpn_last_error()
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    L.check(L.kpn_render_rays_train(ctypes.byref(scene.desc), B.ptr(scene.ws), B.ptr(weights.tensor), ctypes.byref(a), ctypes.byref(t),
                                    B.ptr(ws), nb, B.stream))
    return {k: B.get(v) for k, v in st.items()}


def rgba2out(L, B, rgba, z, canary=np.nan):
    """kpn_rgba2out -> (color, depth, alpha, contrib, sdf) (numpy); every output is pre-filled with `canary`"""
    R, S = z.shape
    outs = [B.full(s, canary) for s in ((R, 3), R, R, (R, S), R)]
    q, zz = B.put(rgba), B.put(z)
    L.check(L.kpn_rgba2out(B.ptr(q), B.ptr(zz), R, S, *[B.ptr(v) for v in outs], B.stream))
    return [B.get(v) for v in outs]


def importance_sample(L, B, contrib, z, n, u=None, canary=np.nan):
    """kpn_importance_sample -> (return code, out (R, n) numpy)"""
    R, Dm2 = contrib.shape
    out = B.full((R, n), canary)
    c, zz, uu = B.put(contrib), B.put(z), (None if u is None else B.put(u))
    rc = L.kpn_importance_sample(B.ptr(c), B.ptr(zz), B.ptr(uu), R, Dm2, n, B.ptr(out), B.stream)
    return rc, B.get(out)


def check_sampler_agrees(L, B, st, Sf, u=None, min_hit_rays=2):
    """st: the stage arrays of one render (numpy).  contrib from kpn_rgba2out (the kernel and call the render makes), z_mid in fp32,
    kpn_importance_sample with the same u, sort(cat) in NumPy: bit-equal to the stage output z_fine.  Both kernels perform the same
    fp32 operations in the same order (contraction-proof KADD / KMUL, plain division).  -> the samples"""
    zc, rc = np.asarray(st["z_coarse"], np.float32), np.asarray(st["rgba_coarse"], np.float32)
    assert np.isfinite(zc).all() and np.isfinite(rc).all() and np.isfinite(st["z_fine"]).all()
    _, _, alpha, contrib, _ = rgba2out(L, B, rc, zc)
    assert (alpha > 1e-3).sum() >= min_hit_rays, alpha          # contrib is non-trivial
    z_mid = np.float32(0.5) * (zc[:, 1:] + zc[:, :-1])
    assert z_mid.dtype == np.float32
    code, znew = importance_sample(L, B, np.ascontiguousarray(contrib[:, 1:-1]), z_mid, Sf, u)
    assert code == 0
    want = np.sort(np.concatenate([zc, znew], -1), axis=-1)
    diff = bits(want) != bits(st["z_fine"])
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    return znew


def check_coarse_records_kept(st, znew):
    """z_fine is sorted, and the rgba_fine stage holds rgba_coarse's records at the positions of the coarse depths (equal depths are
    ordered coarse first)"""
    zc, zf = st["z_coarse"], st["z_fine"]
    assert (np.diff(zf, axis=-1) >= 0).all()
    pos = np.arange(zc.shape[1])[None] + (znew[:, None, :] < zc[:, :, None]).sum(-1)
    rows = np.arange(zc.shape[0])[:, None]
    assert np.array_equal(bits(zf[rows, pos]), bits(zc))
    assert np.array_equal(bits(st["rgba_fine"][rows, pos]), bits(st["rgba_coarse"]))


# ------------------------------------------------------------------------------------------------
# 3. kpn_importance_sample, kpn_ray_bbox_intersection, kpn_make_rays
IS_BINS = (1, 2, 14, 63, 128)
IS_SAMPLES = (1, 16, 65, 200)
IS_RAYS = 67                                     # one full 64-thread workgroup plus three
IS_CONTRIB = ("random", "zero", "spike", "tiny")
IS_U = ("linspace", "random", "edges")


@functools.lru_cache(maxsize=None)
def sampler_inputs(Dm2, n, ckind, ukind):
    rng = np.random.default_rng(5000 + 1000 * IS_CONTRIB.index(ckind) + 300 * IS_U.index(ukind) + 7 * Dm2 + n)
    R = IS_RAYS
    c = rng.random((R, Dm2), dtype=np.float32)
    if ckind == "zero":
        c[:] = 0.0
    elif ckind == "spike":                        # the bins beside the spike are narrower than 1e-5: the den < 1e-5 branch
        c[:] = 0.0
        c[np.arange(R), rng.integers(0, Dm2, R)] = 1.0
    elif ckind == "tiny":
        c *= np.float32(1e-7)
    z = np.ascontiguousarray(np.sort(2.0 + 3.0 * rng.random((R, Dm2 + 1), dtype=np.float32), axis=-1))
    u = None
    if ukind != "linspace":
        u = rng.random((R, n), dtype=np.float32)
    if ukind == "edges":
        for r in range(R):
            u[r, rng.integers(0, n)] = (0.0, 1.0, np.float32(1.0) - np.float32(2.0 ** -24))[r % 3]
    ref = oracle.importance_sample(c, z, n, u=u)
    ref.setflags(write=False)
    return c, z, u, ref


def check_sampler_grid(L, B, Dm2, exact):
    """every (n, contrib, u) of one bin count against the oracle: bit-equal on the emulator; on the device the bin-flip-aware rule
    the golden test uses (assert_samples_close with its committed defaults).  Both: every sample within [z[0], z[-1]].
    -> (samples that differ from the oracle, samples)"""
    differ = total = 0
    for n in IS_SAMPLES:
        for ckind in IS_CONTRIB:
            for ukind in IS_U:
                c, z, u, ref = sampler_inputs(Dm2, n, ckind, ukind)
                code, out = importance_sample(L, B, c, z, n, u)
                assert code == 0
                assert (out >= z[:, :1]).all() and (out <= z[:, -1:]).all(), (Dm2, n, ckind, ukind)
                if exact:
                    assert np.array_equal(bits(out), bits(ref)), (Dm2, n, ckind, ukind)
                else:
                    assert_samples_close(out, ref, z)
                differ += int((bits(out) != bits(ref)).sum())
                total += out.size
    print(f"[ray stages] importance_sample Dm2={Dm2}: {differ} of {total} samples differ from the oracle")
    return differ, total


def check_sampler_refuses_129_bins(L, B):
    rng = np.random.default_rng(3)
    c, z = rng.random((3, 129), dtype=np.float32), np.sort(rng.random((3, 130), dtype=np.float32), -1)
    code, out = importance_sample(L, B, c, z, 5, canary=CANARY)
    assert code != 0 and b"bin count" in L.kpn_last_error()
    assert (out == CANARY).all()                 # a refused call launches nothing


BOX_BOUNDS = np.array([[-0.4, -0.9, -0.3], [0.35, 0.85, 0.25]], np.float32)       # three different extents
BOX_ORIGINS = {"outside": np.array([0.1, -0.2, 3.0], np.float32), "inside": np.array([0.05, 0.3, -0.1], np.float32),
               "on_face": np.array([0.1, -0.2, np.float32(0.25) + np.float32(0.01)], np.float32)}


@functools.lru_cache(maxsize=None)
def box_directions():
    """500 seeded unit directions and the planted rows: axis-parallel ones and components under the |d| < 1e-5 clamp"""
    d = np.random.default_rng(11).standard_normal((500, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    planted = np.array([(0, 0, -1), (0, 0, 1), (1, 0, 0), (1e-6, -1e-6, -1), (0, 1e-5, -1)], np.float32)
    return np.ascontiguousarray(np.concatenate([planted, d]).astype(np.float32))


def box_corner_directions(orig):
    """unit directions from `orig` at the corners and the edge mid-points of the padded box: decisions on the 1e-6 test by design"""
    lo, hi = BOX_BOUNDS[0] - np.float32(0.01), BOX_BOUNDS[1] + np.float32(0.01)
    pts = [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    mid = 0.5 * (lo + hi)
    for ax in range(3):
        o1, o2 = [a for a in range(3) if a != ax]
        for v1 in (lo[o1], hi[o1]):
            for v2 in (lo[o2], hi[o2]):
                p = [0.0, 0.0, 0.0]
                p[ax], p[o1], p[o2] = mid[ax], v1, v2
                pts.append(tuple(p))
    d = np.array(pts, np.float32) - orig
    return np.ascontiguousarray((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))


def ray_bbox(L, B, orig, dirs):
    R = len(dirs)
    near, far, hit = B.full(R, np.nan), B.full(R, np.nan), B.full(R, 7, np.uint8)
    b, o, d = B.put(BOX_BOUNDS), B.put(orig), B.put(dirs)
    L.check(L.kpn_ray_bbox_intersection(B.ptr(b), B.ptr(o), B.ptr(d), R, B.ptr(near), B.ptr(far), B.ptr(hit), B.stream))
    return B.get(near), B.get(far), B.get(hit)


def check_ray_bbox(L, B, where, exact):
    """near, far and hit against the oracle: bit-equal on the emulator (the corner- and edge-aimed set included); on the device the hit
    bits exact and near / far within 2e-6 (the bars of test_stage_ops_vs_golden)"""
    orig = BOX_ORIGINS[where]
    sets = [box_directions()] + ([box_corner_directions(orig)] if exact else [])
    for dirs in sets:
        near, far, hit = ray_bbox(L, B, orig, dirs)
        on, of, oh = oracle.ray_bbox_intersection(BOX_BOUNDS, orig, dirs)
        assert set(np.unique(hit)) <= {0, 1} and np.isfinite(near).all() and np.isfinite(far).all()
        if exact:
            assert np.array_equal(hit.astype(bool), oh) and np.array_equal(bits(near), bits(on)) and np.array_equal(bits(far), bits(of))
        else:
            assert np.array_equal(hit.astype(bool), oh)
            np.testing.assert_allclose(near, on, rtol=0, atol=2e-6)
            np.testing.assert_allclose(far, of, rtol=0, atol=2e-6)
    hits = oracle.ray_bbox_intersection(BOX_BOUNDS, orig, box_directions())[2]
    assert 0 < hits.sum() and (where != "outside" or hits.sum() < hits.size)      # the case decides something


MAKE_RAYS_GRID = (1, 2, 3, 7, 6)                 # x0, y0 != 0, step 3 on case_c's 24 x 24 target


def check_make_rays(L, B, cam_tar, bounds, stages):
    """the exported kpn_make_rays over MAKE_RAYS_GRID: dirs and cam_pos bit-equal to the `dirs` / `cam_pos` stages of a kpn_render_rays
    call over the same grid (the same kernel); near / far against the oracle within 2e-6"""
    x0, y0, step, nx, ny = MAKE_RAYS_GRID
    R = nx * ny
    K, RT, b = (B.put(np.asarray(t, np.float32).reshape(s)) for t, s in ((cam_tar["K"], (4, 4)), (cam_tar["RT"], (4, 4)), (bounds, (2, 3))))
    dirs, cam_pos, near, far = B.full((R, 3), np.nan), B.full(3, np.nan), B.full(R, np.nan), B.full(R, np.nan)
    L.check(L.kpn_make_rays(B.ptr(K), B.ptr(RT), float(cam_tar["znear"]), float(cam_tar["zfar"]), B.ptr(b), x0, y0, step, nx, ny,
                            B.ptr(dirs), B.ptr(cam_pos), B.ptr(near), B.ptr(far), B.stream))
    dirs, cam_pos, near, far = (B.get(v) for v in (dirs, cam_pos, near, far))
    assert np.array_equal(bits(dirs), bits(stages["dirs"])) and np.array_equal(bits(cam_pos), bits(stages["cam_pos"]))
    ys, xs = np.meshgrid(y0 + step * np.arange(ny), x0 + step * np.arange(nx), indexing="ij")
    pix = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32)
    od, oc, on, of = oracle.make_rays(cam_tar, bounds, pix)
    np.testing.assert_allclose(near, on, rtol=0, atol=2e-6)
    np.testing.assert_allclose(far, of, rtol=0, atol=2e-6)
    assert (on < of).any()                       # some rays cross the box: the hit branch of near / far ran


# ------------------------------------------------------------------------------------------------
# 4. grid-stride paths: the compositor's and the sampler's grids cap at 8192 workgroups of four rays
STRIDE_RAYS = 4 * 8192 + 5


STRIDE_MIN_ALPHA = 0.05


@functools.lru_cache(maxsize=None)
def stride_inputs(S):
    """Built as in test_rgba2out_sample_counts_vs_oracle, with one input condition, on the oracle's alpha: every ray has
    alpha >= STRIDE_MIN_ALPHA or alpha == 0.  depth and sdf are ratios of sums of a_i = 1 - exp(-sigma dist), and on a thin ray each a_i
    carries the exp's rounding, 6e-8, whole: two exps that differ by one ulp on half the samples move depth by up to
    sqrt(S) 6e-8 (z spread) / alpha, measured on the unconditioned draw at S = 65 as 4.2e-5 at alpha = 6.7e-3 (two of the 32,773 rays
    lay below 0.01) and 6.8e-6 from 0.05 on; 1,237 rays hold no ray that thin.  A ray below the threshold has its density scale lifted to an optical depth of
    0.2 (alpha 0.18); the five rays that the stride loop alone reaches have the scale 20."""
    rng = np.random.default_rng(900 + S)
    R = STRIDE_RAYS
    rgba = rng.random((R, S, 5), dtype=np.float32)
    scale = rng.random((R, 1), dtype=np.float32) * 40.0
    scale[4 * 8192:] = 20.0
    unit = rgba[..., 0].copy()
    unit[rng.random((R, S)) < 0.3] = 0.0
    z = np.ascontiguousarray(np.sort(2.0 + 3.0 * rng.random((R, S), dtype=np.float32), axis=-1))
    for _ in range(4):
        rgba[..., 0] = unit * scale
        ref = oracle.rgba2out(rgba, z)
        thin = (ref[2] < STRIDE_MIN_ALPHA) & (ref[2] != 0.0)
        if not thin.any():
            break
        scale[thin] *= (0.2 / -np.log1p(-ref[2][thin].astype(np.float64)))[:, None].astype(np.float32)   # optical depth 0.2: alpha 0.18
    assert ((ref[2] >= STRIDE_MIN_ALPHA) | (ref[2] == 0.0)).all()       # the input condition, on the oracle alone
    return rgba, z, ref


def check_rgba2out_stride(L, B, S):
    """kpn_rgba2out over STRIDE_RAYS rays: the stride loop and the one-ray-ahead prefetch carry the last five rays.  Every ray against
    the oracle with the tolerances of test_rgba2out_sample_counts_vs_oracle; the canary fill of every output is overwritten for all
    rays."""
    rgba, z, ref = stride_inputs(S)
    got = rgba2out(L, B, rgba, z, canary=CANARY)
    for name, a, b, tol in zip(("color", "depth", "alpha", "contrib", "sdf"), got, ref, (5e-6, 3e-5, 5e-6, 3e-6, 3e-5)):
        assert (a != CANARY).all(), name
        err = np.abs(a.reshape(b.shape) - b)
        assert err.max() <= tol, (name, float(err.max()))
