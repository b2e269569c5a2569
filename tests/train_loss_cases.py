"""Shared by the emulator and the GPU tests of kpn_train_loss: seeded inputs, the reference's formulas (src/utils.py:108-183) in
torch on the CPU at a chosen precision (values and what autograd derives), the bar, and a driver that calls the C ABI on
buffers of either kind (numpy for the emulator build, device tensors for the product library).

Bar (per term and per gradient tensor, every element): |native - fp64| <= 4 * max|eager fp32 - fp64| + one fp32 ulp of the
tensor's largest fp64 magnitude — the rule of tests/test_encoders_cpu.py.  The eager fp32 error is measured here, on the same
inputs, from torch's own fp32 evaluation of the same formulas; never from the kernel."""
import ctypes
import functools

import numpy as np
import torch

from keypointnerf_amd import lib as kl

FACTOR = 4.0
WEIGHTS = (1.0, 10.0, 3.0, 0.5, 4.0)               # l1_c, l1, l2, lp, mloss: every term on
TERMS = ("e_pix_c", "e_pix_l1", "e_pix_l2", "e_pix_lp", "mask_loss_c", "mask_loss_f")
# 1, 63, 64, 65, 4096: around a wave and the shipped patch; 3 N is no multiple of 4 at 1, 63 and 65; 171: 3 N = 2 * 256 + 1, a
# third block with a single element; 174,764: 3 N = 2048 * 256 + 4, the first size at which the grid is capped and a thread
# takes a second element
SHAPES = (1, 63, 64, 65, 171, 4096, 174764)
GRADS = ("d_tex", "d_tex_fine", "d_alpha", "d_alpha_fine")


@functools.lru_cache(maxsize=None)
def inputs(n, seed=0):
    """tex, tex_fine, tar (3n), alpha, alpha_fine, tar_alpha (n); |src - tar| >= 2e-3 (no sign decision near a tie), alphas on both
    sides of the clamp's band.  Cached: shared, treat as read-only."""
    r = np.random.default_rng(1000 * seed + n)
    tar = r.random(3 * n, dtype=np.float32)
    d = {}
    for k in ("tex", "tex_fine"):
        step = (r.uniform(2e-3, 0.6, 3 * n) * r.choice([-1.0, 1.0], 3 * n)).astype(np.float32)
        src = (tar + step).astype(np.float32)
        assert (np.abs(src.astype(np.float64) - tar) >= 1e-3).all()
        d[k] = src
    d["tar"] = tar
    for k in ("alpha", "alpha_fine"):
        d[k] = r.uniform(-0.15, 1.15, n).astype(np.float32)
    d["tar_alpha"] = (r.random(n) > 0.5).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


def formulas(inp, weights, dtype):
    """the reference's terms (float64 numpy, 6) and autograd's gradients of each term alone, evaluated by torch on the CPU in
    `dtype`: {"d_tex", "d_tex_fine" (3, 3n), "d_alpha", "d_alpha_fine"}; a missing input or weight <= 0 gives 0 / None"""
    t = {k: (None if v is None else torch.from_numpy(np.array(v)).to(dtype)) for k, v in inp.items()}
    for k in ("tex", "tex_fine", "alpha", "alpha_fine"):
        if t[k] is not None:
            t[k].requires_grad_(True)
    l1_c, l1, l2, lp, ml = weights
    terms = np.zeros(6, np.float64)
    grads = {"d_tex": None, "d_tex_fine": [None, None, None], "d_alpha": None, "d_alpha_fine": None}

    def take(slot, value, wrt):
        terms[slot] = float(value.detach().double())
        return torch.autograd.grad(value, wrt)[0].detach().double().numpy()

    if t["tex"] is not None and l1_c > 0:
        grads["d_tex"] = take(0, l1_c * (t["tex"] - t["tar"]).abs().mean(), t["tex"])
    if t["tex_fine"] is not None:
        s, tar = t["tex_fine"], t["tar"]
        if l1 > 0:
            grads["d_tex_fine"][0] = take(1, l1 * (s - tar).abs().mean(), s)
        if l2 > 0:
            grads["d_tex_fine"][1] = take(2, l2 * (s - tar).pow(2.0).mean(), s)
        if lp > 0:
            grads["d_tex_fine"][2] = take(3, lp * ((s - tar).abs() + 1e-4).pow(0.4).mean(), s)
    if t["tar_alpha"] is not None and ml > 0:
        for slot, k in ((4, "alpha"), (5, "alpha_fine")):
            if t[k] is not None:
                grads["d_" + k] = take(slot, ml * torch.nn.functional.mse_loss(t[k].clip(1e-3, 1.0), t["tar_alpha"]), t[k])
    return terms, grads


def bar(eager, ref):
    e = float(np.abs(np.asarray(eager, np.float64) - ref).max())
    return FACTOR * e + float(np.spacing(np.float32(np.abs(ref).max()))), e


def check_against_fp64(got_terms, got_grads, inp, weights, report=None):
    """every term and every gradient element against the fp64 formulas, bar from torch's fp32 run of the same formulas"""
    ref_t, ref_g = formulas(inp, weights, torch.float64)
    eag_t, eag_g = formulas(inp, weights, torch.float32)
    rows = []
    for q, name in enumerate(TERMS):
        b, e = bar(eag_t[q], ref_t[q:q + 1])
        err = abs(float(got_terms[q]) - ref_t[q])
        rows.append((name, err, e, b))
    pairs = [("d_tex", got_grads["d_tex"], ref_g["d_tex"], eag_g["d_tex"]), ("d_alpha", got_grads["d_alpha"], ref_g["d_alpha"], eag_g["d_alpha"]),
             ("d_alpha_fine", got_grads["d_alpha_fine"], ref_g["d_alpha_fine"], eag_g["d_alpha_fine"])]
    for k, nm in enumerate(("l1", "l2", "lp")):
        pairs.append((f"d_tex_fine[{nm}]", None if got_grads["d_tex_fine"] is None else got_grads["d_tex_fine"][k], ref_g["d_tex_fine"][k],
                      eag_g["d_tex_fine"][k]))
    for name, got, ref, eag in pairs:
        if ref is None:
            continue
        b, e = bar(eag, ref)
        rows.append((name, float(np.abs(got.astype(np.float64).reshape(ref.shape) - ref).max()), e, b))
    for name, err, e, b in rows:
        line = f"n={inp['tar'].size // 3} {name}: |native - fp64| = {err:.3e}, eager fp32 = {e:.3e}, bar = {b:.3e}"
        print(line)
        if report is not None:
            report.append(line)
    for name, err, e, b in rows:
        assert err <= b, (name, err, e, b)


SENTINEL = np.float32(-777.25)


class Driver:
    """kpn_train_loss / kpn_pix_l1_loss on numpy inputs.  to_dev(np array) -> buffer, ptr(buffer) -> c_void_p, to_host(buffer) -> np
    array, stream: what the C ABI gets.  Gradient buffers are pre-filled with SENTINEL, the workspace with 0xFF bytes."""

    def __init__(self, L, to_dev, ptr, to_host, stream=None):
        self.L, self.to_dev, self.ptr, self.to_host, self.stream = L, to_dev, ptr, to_host, stream

    def workspace(self, n):
        return self.to_dev(np.full(self.L.kpn_train_loss_workspace_bytes(n), 0xFF, np.uint8))

    def run(self, inp, weights, ws=None, reset=1, want=GRADS):
        n = inp["tar"].size // 3
        if ws is None:
            ws = self.workspace(n)
        dev = {k: (None if v is None else self.to_dev(np.ascontiguousarray(v, np.float32))) for k, v in inp.items()}
        sizes = {"d_tex": 3 * n, "d_tex_fine": 9 * n, "d_alpha": n, "d_alpha_fine": n}
        out = {k: self.to_dev(np.full(sizes[k], SENTINEL, np.float32)) for k in want}
        terms = self.to_dev(np.full(6, SENTINEL, np.float32))
        p = lambda b: None if b is None else self.ptr(b)
        args = kl.TrainLossArgs(tex=p(dev["tex"]), tex_fine=p(dev["tex_fine"]), tar=p(dev["tar"]), alpha=p(dev["alpha"]),
                                alpha_fine=p(dev["alpha_fine"]), tar_alpha=p(dev["tar_alpha"]), n=n, l1_c=weights[0], l1=weights[1],
                                l2=weights[2], lp=weights[3], mloss=weights[4], reset_ticket=reset, terms=p(terms),
                                **{k: p(out.get(k)) for k in GRADS})
        self.L.check(self.L.kpn_train_loss(ctypes.byref(args), self.ptr(ws), self.stream))
        g = {k: (self.to_host(out[k]) if k in out else None) for k in GRADS}
        if g["d_tex_fine"] is not None:
            g["d_tex_fine"] = g["d_tex_fine"].reshape(3, 3 * n)
        return self.to_host(terms), g

    def pix_l1(self, src, tar, lam):
        a, b = self.to_dev(np.ascontiguousarray(src, np.float32)), self.to_dev(np.ascontiguousarray(tar, np.float32))
        loss, d = self.to_dev(np.zeros(1, np.float32)), self.to_dev(np.full(a.shape[0], SENTINEL, np.float32))
        scratch = self.to_dev(np.zeros(2048 * 8 + 8, np.uint8))
        self.L.check(self.L.kpn_pix_l1_loss(self.ptr(a), self.ptr(b), src.size, lam, self.ptr(loss), self.ptr(d), self.ptr(scratch), self.stream))
        return self.to_host(loss)[0], self.to_host(d)


# ---- the checks both builds run -------------------------------------------------------------------------------------------
def check_values_and_gradients(drv, n, report=None):
    inp = inputs(n)
    terms, g = drv.run(inp, WEIGHTS)
    check_against_fp64(terms, g, inp, WEIGHTS, report)


def check_l1_bit_identical_and_rerun(drv, n):
    """L1 slots and gradients = two kpn_pix_l1_loss calls, bit for bit; a second launch on the SAME workspace without a reset
    (the kernel left its ticket at zero) repeats every bit"""
    inp = inputs(n)
    ws = drv.workspace(n)
    terms, g = drv.run(inp, WEIGHTS, ws=ws, reset=1)
    for slot, src, lam, got in ((0, "tex", WEIGHTS[0], g["d_tex"]), (1, "tex_fine", WEIGHTS[1], g["d_tex_fine"][0])):
        loss, d = drv.pix_l1(inp[src], inp["tar"], lam)
        assert np.float32(loss).tobytes() == np.float32(terms[slot]).tobytes(), (slot, loss, terms[slot])
        assert np.array_equal(d, got)
    terms2, g2 = drv.run(inp, WEIGHTS, ws=ws, reset=0)
    assert terms.tobytes() == terms2.tobytes()
    for k in GRADS:
        assert g[k].tobytes() == g2[k].tobytes(), k


def check_ties(drv):
    """src == tar: the l1, l2 AND lp gradients are exactly 0 (sign(0) = 0, although (1e-4)^-0.6 is finite)"""
    n = 65
    inp = dict(inputs(n))
    inp["tex"] = inp["tex_fine"] = inp["tar"]
    terms, g = drv.run(inp, WEIGHTS)
    assert not g["d_tex"].any() and not g["d_tex_fine"].any()
    assert terms[0] == 0.0 and terms[1] == 0.0 and terms[2] == 0.0
    want_lp = WEIGHTS[3] * 1e-4 ** 0.4
    assert abs(float(terms[3]) - want_lp) <= float(np.spacing(np.float32(want_lp)))
    # ties among ordinary elements: exactly those are 0, their neighbours keep the formula's value
    inp2 = dict(inputs(n))
    src = np.array(inp2["tex_fine"])
    src[::7] = inp2["tar"][::7]
    inp2["tex_fine"] = src
    _, g2 = drv.run(inp2, WEIGHTS)
    tie = np.zeros(3 * n, bool)
    tie[::7] = True
    assert not g2["d_tex_fine"][:, tie].any() and (g2["d_tex_fine"][:, ~tie] != 0).all()


def check_clamp_band(drv):
    """alpha exactly 1e-3 and exactly 1: the gradient passes; one ulp outside: exactly 0, the value takes the clipped number"""
    lo, hi = np.float32(1e-3), np.float32(1.0)
    alpha = np.array([lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(2)), 0.5], np.float32)
    t = np.array([1, 0, 1, 0, 1], np.float32)
    n, lam = alpha.size, WEIGHTS[4]
    inp = {"tex": None, "tex_fine": None, "tar": np.zeros(3 * n, np.float32), "alpha": alpha, "alpha_fine": alpha[::-1].copy(), "tar_alpha": t}
    terms, g = drv.run(inp, WEIGHTS)
    for got, a, tt, slot in ((g["d_alpha"], alpha, t, 4), (g["d_alpha_fine"], alpha[::-1], t, 5)):
        c = np.clip(a, lo, hi).astype(np.float64)
        inside = (a >= lo) & (a <= hi)
        want = np.where(inside, 2.0 * lam * (c - tt) / n, 0.0)
        assert (got[~inside] == 0.0).all() and (got[inside] != 0.0).all()
        assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
        value = lam * np.mean((c - tt) ** 2)
        assert abs(float(terms[slot]) - value) <= float(np.spacing(np.float32(value)))
    assert terms[0] == 0.0 and terms[1] == 0.0 and terms[2] == 0.0 and terms[3] == 0.0      # NULL tex / tex_fine
    # a NaN alpha: what torch does (the term is NaN, the element's gradient is clamp backward's 0, the others are NaN-free)
    a_nan = np.array([0.25, np.nan, 0.75, 2.0], np.float32)
    t4 = np.array([1, 1, 0, 0], np.float32)
    inp = {"tex": None, "tex_fine": None, "tar": np.zeros(12, np.float32), "alpha": a_nan, "alpha_fine": None, "tar_alpha": t4}
    terms, g = drv.run(inp, WEIGHTS)
    ta = torch.from_numpy(a_nan).requires_grad_(True)
    ref = lam * torch.nn.functional.mse_loss(ta.clip(1e-3, 1.0), torch.from_numpy(t4))
    ref.backward()
    assert np.isnan(float(ref.detach())) and np.isnan(terms[4]) and terms[5] == 0.0
    assert np.array_equal(np.isnan(g["d_alpha"]), np.isnan(ta.grad.numpy()))
    ok = ~np.isnan(ta.grad.numpy())
    assert np.allclose(g["d_alpha"][ok], ta.grad.numpy()[ok], rtol=3e-7, atol=0) and g["d_alpha"][1] == ta.grad.numpy()[1]
    assert (g["d_alpha_fine"] == SENTINEL).all()


def check_skipped_terms_leave_their_buffers(drv):
    """weight 0 or a NULL input: slot 0, gradient buffer untouched (the sentinel survives)"""
    n = 64
    inp = inputs(n)
    # weights of 0 for l1_c, l2 and mloss
    terms, g = drv.run(inp, (0.0, 10.0, 0.0, 0.5, 0.0))
    assert terms[0] == 0.0 and terms[2] == 0.0 and terms[4] == 0.0 and terms[5] == 0.0 and terms[1] > 0.0 and terms[3] > 0.0
    assert (g["d_tex"] == SENTINEL).all() and (g["d_alpha"] == SENTINEL).all() and (g["d_alpha_fine"] == SENTINEL).all()
    assert (g["d_tex_fine"][1] == SENTINEL).all() and (g["d_tex_fine"][0] != SENTINEL).all() and (g["d_tex_fine"][2] != SENTINEL).all()
    # a negative weight is a switched-off term as well (the reference's `v <= 0.0`)
    terms, g = drv.run(inp, (1.0, -1.0, 3.0, 0.5, 4.0))
    assert terms[1] == 0.0 and (g["d_tex_fine"][0] == SENTINEL).all() and (g["d_tex_fine"][1] != SENTINEL).all()
    # NULL inputs: no fine prediction, no coarse alpha; then no tar_alpha at all
    cut = dict(inp, tex_fine=None, alpha=None)
    terms, g = drv.run(cut, WEIGHTS)
    assert terms[1] == 0.0 and terms[2] == 0.0 and terms[3] == 0.0 and terms[4] == 0.0 and terms[0] > 0.0 and terms[5] > 0.0
    assert (g["d_tex_fine"] == SENTINEL).all() and (g["d_alpha"] == SENTINEL).all() and (g["d_alpha_fine"] != SENTINEL).all()
    terms, g = drv.run(dict(inp, tar_alpha=None), WEIGHTS)
    assert terms[4] == 0.0 and terms[5] == 0.0 and (g["d_alpha"] == SENTINEL).all() and (g["d_alpha_fine"] == SENTINEL).all()
    # value only: no gradient pointer at all
    terms_v, _ = drv.run(inp, WEIGHTS, want=())
    terms_g, _ = drv.run(inp, WEIGHTS)
    assert terms_v.tobytes() == terms_g.tobytes()
