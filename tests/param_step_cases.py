"""Shared by the emulator and the GPU tests of the parameter step (kpn_fold_params, kpn_fold_params_backward, kpn_adam_step;
csrc/param_kernels.hip): seeded inputs over the layer table, the formulas restated in fp64, the bars, and a driver that calls the
C ABI on buffers of either kind (numpy for the emulator build, device tensors for the product library).

The shape is the layer table itself (19 layers, 864 rows, 4 to 232 wide, 1 / 2 / 33-row layers, normed beside plain ones).

Bars.  They follow from the number formats, not from the kernels (u = 2^-24, one fp32 rounding):
  fold        W = fl(v * fl(g / n)): two roundings of an otherwise exact value          |W - W64|  <= 2^-23 |W64|
  dg          fl(dot / n)                                                              |dg - dg64| <= 2^-23 |dg64|
  dv          fl(fl(s dW) - fl(c v)), s and c one rounding each: at most 3 u on either
              product and u on the difference, which is at most u (|s dW| + |c v|)     |dv - dv64| <= 2^-22 (|s dW| + |c v|)
  copies      bit-exact; accumulate = fl(old + new) bit for bit
  Adam m, v   one rounding of the fp64 formula's value (bar 2^-22 relative)
  Adam p      |p - p64| <= 2^-24 |p64| + 2^-20 |update64|
  trajectory  50 steps: the native distance from the fp64 trajectory is at most twice torch.optim.Adam's (fp32, CPU,
              foreach=False) on the same gradients — both are fp32 states with different rounding sequences
"""
import ctypes
import functools

import numpy as np
import torch

from keypointnerf_amd import lib as kl
from keypointnerf_amd.synthetic import HOTPATH_LAYERS

N_PLAIN = sum(o * i + o for _, _, (o, i), _ in HOTPATH_LAYERS) + 1
N_NORM_ROWS = sum(o for _, _, (o, i), wn in HOTPATH_LAYERS if wn)
SENTINEL = np.float32(-777.25)


def slots():
    """(kpn_param_table field, layer, shape) per tensor, in weights.hot_tensor_names order"""
    out = []
    for l, (_, _, (o, i), wn) in enumerate(HOTPATH_LAYERS):
        if wn:
            out.append(("g", l, (o, 1)))
        out += [("v_or_w", l, (o, i)), ("b", l, (o,))]
    return out + [("ani_al", None, (1,))]


@functools.lru_cache(maxsize=None)
def inputs(seed=0):
    """the 44 tensors and a d_plain: every row of every layer scaled by its own power of two in 2^-12 .. 2^12, g of both signs.
    Cached: shared, read-only."""
    r = np.random.default_rng(4200 + seed)
    tensors = []
    for field, l, shape in slots():
        x = r.standard_normal(shape).astype(np.float32)
        if field in ("g", "v_or_w"):
            x = (x * np.exp2(r.integers(-12, 13, (shape[0], 1)))).astype(np.float32)
        if field == "g":
            x = np.where(np.abs(x) < 1e-6, np.float32(0.5), x).astype(np.float32)
            assert (x > 0).any() and (x < 0).any()
        x.setflags(write=False)
        tensors.append(x)
    d_plain = r.standard_normal(N_PLAIN).astype(np.float32)
    o = 0
    for _, _, (rows, cols), _ in HOTPATH_LAYERS:                      # the rows of dW spread like the rows of v
        d_plain[o:o + rows * cols] *= np.repeat(np.exp2(r.integers(-12, 13, rows)), cols).astype(np.float32)
        o += rows * cols + rows
    d_plain.setflags(write=False)
    return tuple(tensors), d_plain


def fold64(tensors):
    """the fold restated in fp64 numpy -> (plain64, is_copy mask)"""
    parts, copy = [], []
    it = iter(tensors)
    for _, _, (o, i), wn in HOTPATH_LAYERS:
        if wn:
            g, v = next(it).astype(np.float64), next(it).astype(np.float64)
            w = v * (g.reshape(-1, 1) / np.sqrt((v * v).sum(1, keepdims=True)))
        else:
            w = next(it).astype(np.float64)
        b = next(it).astype(np.float64)
        parts += [w.reshape(-1), b]
        copy += [np.full(o * i, not wn), np.full(o, True)]
    parts.append(next(it).astype(np.float64).reshape(1))
    copy.append(np.full(1, True))
    return np.concatenate(parts), np.concatenate(copy)


def backward64(tensors, d_plain):
    """per tensor: (fp64 gradient by torch autograd of the restated fold, per-element bar scale or None for a copy).  The scale
    of dg is |dg64|, of dv |s dW| + |c v|."""
    out, o = [], 0
    it = iter(tensors)
    for _, _, (rows, cols), wn in HOTPATH_LAYERS:
        dW = torch.from_numpy(d_plain[o:o + rows * cols].astype(np.float64)).reshape(rows, cols)
        db = d_plain[o + rows * cols:o + rows * cols + rows].astype(np.float64)
        o += rows * cols + rows
        if wn:
            g = torch.from_numpy(next(it).astype(np.float64)).requires_grad_(True)
            v = torch.from_numpy(next(it).astype(np.float64)).requires_grad_(True)
            n = v.pow(2).sum(1, keepdim=True).sqrt()
            dg, dv = torch.autograd.grad(v * (g / n), [g, v], dW)
            with torch.no_grad():
                dot = (dW * v).sum(1, keepdim=True)
                scale = ((g / n) * dW).abs() + (g * dot / n ** 3 * v).abs()
            out += [(dg.numpy(), np.abs(dg.numpy())), (dv.numpy(), scale.numpy())]
        else:
            next(it)
            out.append((dW.numpy(), None))
        next(it)
        out.append((db, None))
    out.append((d_plain[o:o + 1].astype(np.float64), None))
    return out


class Driver:
    """The three entry points on numpy inputs.  to_dev(np array) -> buffer, ptr(buffer) -> c_void_p, to_host(buffer) -> np array,
    stream: what the C ABI gets."""

    def __init__(self, L, to_dev, ptr, to_host, stream=None):
        self.L, self.to_dev, self.ptr, self.to_host, self.stream = L, to_dev, ptr, to_host, stream

    def table(self, bufs):
        t = kl.ParamTable()
        for b, (field, l, _) in zip(bufs, slots()):
            if b is None:
                continue
            if l is None:
                t.ani_al = self.ptr(b)
            else:
                getattr(t, field)[l] = self.ptr(b)
        return t

    def fold(self, tensors):
        """-> (plain, norms buffer kept on the device side, the device buffers of the tensors)"""
        dev = [self.to_dev(np.ascontiguousarray(x, np.float32).reshape(-1)) for x in tensors]
        plain = self.to_dev(np.full(N_PLAIN, SENTINEL, np.float32))
        assert self.L.kpn_fold_norm_floats() == 3 * N_NORM_ROWS
        norms = self.to_dev(np.zeros(3 * N_NORM_ROWS // 2, np.float64))
        t = self.table(dev)
        self.L.check(self.L.kpn_fold_params(ctypes.byref(t), self.ptr(plain), self.ptr(norms), self.stream))
        return self.to_host(plain), norms, dev

    def backward(self, dev, norms, d_plain, old=None):
        """old=None: overwrite into sentinel-filled buffers; else accumulate into copies of `old` (a list of arrays)"""
        dp = self.to_dev(np.ascontiguousarray(d_plain, np.float32))
        dst = [self.to_dev(np.full(int(np.prod(s)), SENTINEL, np.float32) if old is None else np.array(old[k], np.float32).reshape(-1))
               for k, (_, _, s) in enumerate(slots())]
        t, g = self.table(dev), self.table(dst)
        self.L.check(self.L.kpn_fold_params_backward(ctypes.byref(t), self.ptr(norms), self.ptr(dp), ctypes.byref(g), int(old is not None),
                                                     self.stream))
        return [self.to_host(b).reshape(s) for b, (_, _, s) in zip(dst, slots())]

    def adam(self, p, g, m, v, step, lr, b1, b2, eps, wd):
        """lists of arrays -> (p, m, v) after one kpn_adam_step"""
        bufs = [[self.to_dev(np.ascontiguousarray(x, np.float32).reshape(-1)) for x in lst] for lst in (p, g, m, v)]
        segs = (kl.AdamSegment * len(p))()
        for i in range(len(p)):
            segs[i].param, segs[i].grad, segs[i].exp_avg, segs[i].exp_avg_sq = (self.ptr(bufs[k][i]).value for k in range(4))
            segs[i].count = p[i].size
        a = kl.AdamArgs(segments_host=segs, n_segments=len(p), step=step, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd)
        self.L.check(self.L.kpn_adam_step(ctypes.byref(a), self.stream))
        return tuple([self.to_host(b).reshape(x.shape) for b, x in zip(bufs[k], p)] for k in (0, 2, 3))


# ---- the checks both builds run -------------------------------------------------------------------------------------------
def check_fold(drv):
    tensors, _ = inputs()
    plain, _, _ = drv.fold(tensors)
    ref, copy = fold64(tensors)
    assert plain[copy].tobytes() == ref[copy].astype(np.float32).tobytes()                     # copies: bit-exact
    err = np.abs(plain.astype(np.float64) - ref)
    rel = (err[~copy] / np.abs(ref[~copy])).max()
    print(f"fold: max |W - W64| / |W64| = {rel:.3e} (bar {2.0 ** -23:.3e}), {int((~copy).sum())} folded elements")
    assert (err[~copy] <= 2.0 ** -23 * np.abs(ref[~copy])).all()
    # and torch's own fold of the same inputs: the same bar plus torch's own distance from fp64
    eager = torch.cat([torch._weight_norm(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(g)), 0).reshape(-1)
                       for g, v in _normed_pairs(tensors)]).numpy().astype(np.float64)
    mine, r64 = plain[~copy].astype(np.float64), ref[~copy]
    assert (np.abs(mine - eager) <= 2.0 ** -23 * np.abs(r64) + np.abs(eager - r64)).all()


def _normed_pairs(tensors):
    it = iter(tensors)
    for _, _, _, wn in HOTPATH_LAYERS:
        if wn:
            yield next(it), next(it)
        else:
            next(it)
        next(it)


def check_backward(drv):
    tensors, d_plain = inputs()
    _, norms, dev = drv.fold(tensors)
    got = drv.backward(dev, norms, d_plain)
    ref = backward64(tensors, d_plain)
    worst = {"g": 0.0, "v_or_w": 0.0}
    for k, ((field, l, shape), (r, scale)) in enumerate(zip(slots(), ref)):
        assert not (got[k] == SENTINEL).any(), (field, l)
        if scale is None:
            assert got[k].tobytes() == r.astype(np.float32).tobytes(), (field, l)              # copies: bit-exact
            continue
        err = np.abs(got[k].astype(np.float64) - r.reshape(shape))
        bar = (2.0 ** -23 if field == "g" else 2.0 ** -22) * scale.reshape(shape)
        worst[field] = max(worst[field], float((err / scale.reshape(shape)).max()))
        assert (err <= bar).all(), (field, l, float((err / scale.reshape(shape)).max()))
    print(f"fold backward: max |dg - dg64| / |dg64| = {worst['g']:.3e} (bar {2.0 ** -23:.3e}); "
          f"max |dv - dv64| / (|s dW| + |c v|) = {worst['v_or_w']:.3e} (bar {2.0 ** -22:.3e})")
    # accumulate: pre-filled destinations, result = fl(old + new)
    r = np.random.default_rng(7)
    old = [(r.standard_normal(s) * np.abs(g).mean()).astype(np.float32) for g, (_, _, s) in zip(got, slots())]
    acc = drv.backward(dev, norms, d_plain, old=old)
    for k, (field, l, _) in enumerate(slots()):
        assert acc[k].tobytes() == (old[k] + got[k]).astype(np.float32).tobytes(), (field, l)
    # NULL destinations are skipped, the others are written as before
    dp = drv.to_dev(np.ascontiguousarray(d_plain, np.float32))
    dst = [None if k % 3 == 0 else drv.to_dev(np.full(int(np.prod(s)), SENTINEL, np.float32)) for k, (_, _, s) in enumerate(slots())]
    t, g = drv.table(dev), drv.table(dst)
    drv.L.check(drv.L.kpn_fold_params_backward(ctypes.byref(t), drv.ptr(norms), drv.ptr(dp), ctypes.byref(g), 0, drv.stream))
    for k, (_, _, s) in enumerate(slots()):
        if dst[k] is not None:
            assert drv.to_host(dst[k]).tobytes() == got[k].tobytes()


ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam64(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam's formulas in fp64 numpy -> (p, m, v, update)"""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    upd = (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps)
    return p - upd, m, v, upd


@functools.lru_cache(maxsize=None)
def adam_state(fresh):
    """p, g, m, v over the 44 shapes of the layer table; the gradient of tensor 5 is all zeros; fresh: m = v = 0 (step 1)"""
    r = np.random.default_rng(99)
    p, g, m, v = [], [], [], []
    for k, (_, _, s) in enumerate(slots()):
        p.append(r.standard_normal(s).astype(np.float32))
        g.append((r.standard_normal(s) * 10.0 ** r.uniform(-4, 0)).astype(np.float32) if k != 5 else np.zeros(s, np.float32))
        m.append(np.zeros(s, np.float32) if fresh else (r.standard_normal(s) * 1e-2).astype(np.float32))
        v.append(np.zeros(s, np.float32) if fresh else (r.standard_normal(s) * 1e-2).astype(np.float32) ** 2)
    return p, g, m, v


def check_adam_one_step(drv, step, wd):
    p, g, m, v = adam_state(step == 1)
    gp, gm, gv = drv.adam(p, g, m, v, step, wd=wd, **ADAM)
    worst = [0.0, 0.0, 0.0]
    for k in range(len(p)):
        p64, m64, v64, upd = adam64(p[k], g[k], m[k], v[k], step, wd=wd, **ADAM)
        em, ev, ep = (np.abs(a.astype(np.float64) - b) for a, b in ((gm[k], m64), (gv[k], v64), (gp[k], p64)))
        assert (em <= 2.0 ** -22 * np.abs(m64)).all() and (ev <= 2.0 ** -22 * np.abs(v64)).all(), k
        bar = 2.0 ** -24 * np.abs(p64) + 2.0 ** -20 * np.abs(upd)
        assert (ep <= bar).all(), (k, float((ep / bar).max()))
        nz = lambda e, r: float((e[r != 0] / np.abs(r[r != 0])).max()) if (r != 0).any() else 0.0
        worst = [max(worst[0], nz(em, m64)), max(worst[1], nz(ev, v64)), max(worst[2], float((ep / np.maximum(bar, 1e-300)).max()))]
    if wd == 0.0:                                                     # the zero gradient: from a fresh state nothing moves
        assert step != 1 or (gp[5].tobytes() == p[5].tobytes() and not gm[5].any() and not gv[5].any())
    print(f"adam t={step} wd={wd}: max rel err m = {worst[0]:.3e}, v = {worst[1]:.3e} (bar {2.0 ** -22:.3e}); max |p - p64| / bar = {worst[2]:.3f}")


TRAJ_SHAPES = ((33, 32), (16, 4), (1, 8), (1,))
TRAJ_STEPS = 50


def check_adam_trajectory(drv):
    """50 steps on a seeded gradient sequence: native, torch.optim.Adam (fp32, CPU, foreach=False) and the fp64 formulas from the
    same start; distance = max |p - p64| over every element after the last step"""
    r = np.random.default_rng(123)
    p0 = [r.standard_normal(s).astype(np.float32) for s in TRAJ_SHAPES]
    grads = [[(r.standard_normal(s) * 0.1).astype(np.float32) for s in TRAJ_SHAPES] for _ in range(TRAJ_STEPS)]
    p64, m64, v64 = [x.astype(np.float64) for x in p0], [np.zeros(s) for s in TRAJ_SHAPES], [np.zeros(s) for s in TRAJ_SHAPES]
    pn, mn, vn = list(p0), [np.zeros(s, np.float32) for s in TRAJ_SHAPES], [np.zeros(s, np.float32) for s in TRAJ_SHAPES]
    pt = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p0]
    opt = torch.optim.Adam(pt, lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"], foreach=False)
    for t in range(1, TRAJ_STEPS + 1):
        g = grads[t - 1]
        for k in range(len(p0)):
            p64[k], m64[k], v64[k], _ = adam64(p64[k], g[k], m64[k], v64[k], t, wd=0.0, **ADAM)
            pt[k].grad = torch.from_numpy(g[k].copy())
        opt.step()
        pn, mn, vn = drv.adam(pn, g, mn, vn, t, wd=0.0, **ADAM)
    d_native = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pn, p64))
    d_torch = max(float(np.abs(a.detach().numpy().astype(np.float64) - b).max()) for a, b in zip(pt, p64))
    print(f"adam trajectory, {TRAJ_STEPS} steps: max |native - fp64| = {d_native:.3e}, max |torch.optim.Adam - fp64| = {d_torch:.3e}")
    assert d_torch > 0.0 and d_native <= 2.0 * d_torch, (d_native, d_torch)


def check_determinism(drv):
    """fold, backward and step run twice from the same bytes give the same bytes"""
    tensors, d_plain = inputs()
    runs = []
    for _ in range(2):
        plain, norms, dev = drv.fold(tensors)
        grads = drv.backward(dev, norms, d_plain)
        p, g, m, v = adam_state(False)
        stepped = drv.adam(p, g, m, v, 7, wd=0.01, **ADAM)
        runs.append(plain.tobytes() + drv.to_host(norms).tobytes() + b"".join(x.tobytes() for x in grads)
                    + b"".join(x.tobytes() for lst in stepped for x in lst))
    assert runs[0] == runs[1]


def check_bad_tables(drv):
    """null or inconsistent tables are KPN_EINVAL with a message, before any launch"""
    L = drv.L
    tensors, d_plain = inputs()
    dev = [drv.to_dev(np.ascontiguousarray(x, np.float32).reshape(-1)) for x in tensors]
    plain, norms = drv.to_dev(np.zeros(N_PLAIN, np.float32)), drv.to_dev(np.zeros(3 * N_NORM_ROWS // 2, np.float64))
    ok = drv.table(dev)
    assert L.kpn_fold_params(None, drv.ptr(plain), drv.ptr(norms), drv.stream) == -1 and b"null" in L.kpn_last_error()
    assert L.kpn_fold_params(ctypes.byref(ok), None, drv.ptr(norms), drv.stream) == -1 and b"null" in L.kpn_last_error()
    t = drv.table(dev)
    t.g[0] = None                                                     # a weight-normed layer without its g
    assert L.kpn_fold_params(ctypes.byref(t), drv.ptr(plain), drv.ptr(norms), drv.stream) == -1 and b"inconsistent" in L.kpn_last_error()
    t = drv.table(dev)
    t.g[3] = t.b[3]                                                   # g on a plain layer
    assert L.kpn_fold_params(ctypes.byref(t), drv.ptr(plain), drv.ptr(norms), drv.stream) == -1 and b"inconsistent" in L.kpn_last_error()
    t = drv.table(dev)
    t.b[18] = None
    assert L.kpn_fold_params(ctypes.byref(t), drv.ptr(plain), drv.ptr(norms), drv.stream) == -1 and b"null" in L.kpn_last_error()
    dp = drv.to_dev(np.ascontiguousarray(d_plain, np.float32))
    g = drv.table(dev)
    g.g[3] = g.b[3]
    assert L.kpn_fold_params_backward(ctypes.byref(ok), drv.ptr(norms), drv.ptr(dp), ctypes.byref(g), 0, drv.stream) == -1
    assert b"inconsistent" in L.kpn_last_error()
    assert L.kpn_fold_params_backward(ctypes.byref(ok), None, drv.ptr(dp), ctypes.byref(ok), 0, drv.stream) == -1
    seg = (kl.AdamSegment * 1)()
    seg[0].param = seg[0].grad = seg[0].exp_avg = seg[0].exp_avg_sq = drv.ptr(plain).value
    seg[0].count = 4
    bad = lambda **kw: L.kpn_adam_step(ctypes.byref(kl.AdamArgs(**dict(dict(segments_host=seg, n_segments=1, step=1, lr=1e-3, beta1=0.9,
                                                                           beta2=0.999, eps=1e-8, weight_decay=0.0), **kw))), drv.stream)
    assert bad(step=0) == -1 and b"step" in L.kpn_last_error()
    assert bad(beta1=1.0) == -1 and b"betas" in L.kpn_last_error()
    assert bad(n_segments=0) == -1
    seg[0].count = 0
    assert bad() == -1 and b"segment" in L.kpn_last_error()
    seg[0].count, seg[0].grad = 4, None
    assert bad() == -1 and b"null" in L.kpn_last_error()
