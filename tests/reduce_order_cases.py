"""The summation order of the deterministic fp64 reductions (csrc/kpn_reduce.h) restated in NumPy, and the exact-bit checks
of kpn_mse_psnr, kpn_pix_l1_loss and kpn_train_loss against it that the emulator and the GPU tests share.

The order: blocks = min(ceil(N / 256), 2048); thread (b, t) adds elements b * 256 + t + k * blocks * 256, k = 0, 1, ..., to an
fp64 sum that starts at 0.0; a block's 256 sums go through the tree s = 128 .. 1 (red[t] += red[t + s] for t < s); the blocks'
partials are added to 0.0 in block order.  Nothing here is a tolerance: a changed operand or a changed order of any add moves
the last bits of the sums below, and every comparison is on the bytes.

The element values of the model are exact restatements, not approximations: fp32 subtraction, multiplication and division are
single IEEE operations in NumPy as in the kernels.  Three kinds of seeded inputs:
  * uniform: uniform doubles in [0, 1] rounded to fp32 — for the L1 and squared-error sums (fp32 elements widened to fp64).
    An fp64 sum of a million fp32 values of one magnitude hardly ever rounds, so the L1 sums of these inputs come out the
    same in any order; the squared errors do tell orders apart;
  * wide: the same values times 2^-k, k uniform in 0 .. 40 — L1 sums that round at almost every add, so that their bits
    depend on the order of every one of them;
  * grid: uniform multiples of 2^-24 below 1 — for the two fp64 squares (l2 and the mask terms).  A difference of two has at most
    24 significant bits and its square 48, so the product is exact and independent of whether a compiler fuses the square
    into the add that follows (hipcc does, v_fmac_f64; the emulator's host build does not); the SUMS still round (multiples of
    2^-48 adding up to 2^17), so their bits depend on the order.  For the same reason the grid alphas stay inside the clamp's
    band: its lower end, float32(1e-3), is no multiple of 2^-24, and (1e-3 - t)^2 would need 66 bits; the band's ends have
    their own exact test (train_loss_cases.check_clamp_band).
tests/test_reduce_order_cpu.py asserts which of these sums tell one order from another."""
import functools

import numpy as np

from tests import train_loss_cases as tc

BLOCK, MAX_BLOCKS = 256, 2048
# 1; a block less one, a block, a block and one; 65,539: 257 blocks, the last with three elements; 524,288 = 2048 * 256: exactly the
# grid cap; one more: one thread takes a second element; 1,048,653 = 2 * 524,288 + 77: every thread takes a second, 77 a third
COUNTS = (1, 255, 256, 257, 65539, 524288, 524289, 1048653)
# kpn_train_loss sums over 3 n pixel elements: 3, 255, 258, 524,286 (2048 blocks, the last two short), 524,289 and 1,048,653
TRAIN_N = (1, 85, 86, 174762, 174763, 349551)
LAMBDA = 0.7                                        # kpn_pix_l1_loss: no power of two, so that the fp32 scalings round


def blocks_for(n):
    return min(-(-n // BLOCK), MAX_BLOCKS)


def ordered_sum(e, blocks):
    """the fp64 sum of the non-negative elements e as a grid of `blocks` blocks of 256 threads adds them (module docstring)"""
    e = np.asarray(e, np.float64)
    assert e.ndim == 1 and not (e < 0).any() and not np.signbit(e).any()
    stride = blocks * BLOCK
    rounds = -(-e.size // stride)
    # a thread whose k-th element lies beyond the end adds nothing; here it adds +0.0, the same bits for a sum that is >= +0.0
    padded = np.zeros(rounds * stride, np.float64)
    padded[:e.size] = e
    acc = np.zeros(stride, np.float64)
    for row in padded.reshape(rounds, stride):
        acc = acc + row
    red = acc.reshape(blocks, BLOCK).copy()
    s = BLOCK // 2
    while s > 0:
        red[:, :s] += red[:, s:2 * s]
        s >>= 1
    tot = np.float64(0.0)
    for p in red[:, 0]:
        tot = tot + p
    return tot


@functools.lru_cache(maxsize=None)
def pair(n, seed, kind="uniform"):
    """two seeded float32 vectors in [0, 1] of a kind of the module docstring, about 1 % of the positions exact ties (at least
    one from 100 elements on).  Cached: shared, read-only."""
    r = np.random.default_rng(7919 * seed + n)
    a, b = (r.random(n, dtype=np.float32) if kind == "grid" else r.random(n).astype(np.float32) for _ in range(2))
    if kind == "wide":
        a, b = (np.ldexp(v, -r.integers(0, 41, n)).astype(np.float32) for v in (a, b))
    tie = r.random(n) < 0.01
    if n >= 100:
        tie[r.integers(n)] = True
    a[tie] = b[tie]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def bits(x):
    return np.asarray(x).tobytes()


def sign_gradient(d, gscale):
    """gscale * sign(d), sign(0) = 0, as the kernels store it"""
    return np.where(d > 0, gscale, np.where(d < 0, -gscale, np.float32(0.0))).astype(np.float32)


def check_mse(drv, n):
    a, b = pair(n, 1)
    da, db, out, scratch = drv.to_dev(a), drv.to_dev(b), drv.to_dev(np.zeros(2, np.float64)), drv.to_dev(np.zeros(2048 * 8 + 8, np.uint8))
    drv.L.check(drv.L.kpn_mse_psnr(drv.ptr(da), drv.ptr(db), n, drv.ptr(out), drv.ptr(scratch), drv.stream))
    d = a - b                                                            # fp32
    want = ordered_sum((d * d).astype(np.float64), blocks_for(n)) / np.float64(n)
    got = drv.to_host(out)[0]
    print(f"mse n={n}: got {got!r}, order model {want!r}")
    assert bits(np.float64(got)) == bits(np.float64(want))


def check_pix_l1(drv, n):
    for kind in ("uniform", "wide"):
        src, tar = pair(n, 2, kind)
        loss, grad = drv.pix_l1(src, tar, LAMBDA)
        d = src - tar
        lam = np.float32(LAMBDA)
        want = lam * np.float32(ordered_sum(np.abs(d).astype(np.float64), blocks_for(n)) / np.float64(n))
        print(f"pix_l1 n={n} {kind}: got {loss!r}, order model {want!r}, ties {int((d == 0).sum())}")
        assert bits(np.float32(loss)) == bits(np.float32(want))
        assert bits(grad) == bits(sign_gradient(d, lam / np.float32(n)))


@functools.lru_cache(maxsize=None)
def train_inputs(n, kind):
    tex, tar = pair(3 * n, 3, kind)
    tex_fine, _ = pair(3 * n, 4, kind)
    tex_fine = np.where(pair(3 * n, 5)[0] < 0.01, tar, tex_fine)          # its own ties with THIS tar
    _, tar_alpha = pair(n, 6, kind)
    r = np.random.default_rng(104729 + n)
    alpha, alpha_fine = ((r.integers(1 << 15, 1 << 24, n) * 2.0 ** -24).astype(np.float32) for _ in range(2))   # [2^-9, 1)
    return {"tex": tex, "tex_fine": tex_fine, "tar": tar, "alpha": alpha, "alpha_fine": alpha_fine, "tar_alpha": tar_alpha}


def check_train_loss(drv, n):
    """terms 0, 1 and the two L1 gradients on uniform and on wide inputs, terms 2, 4, 5 on grid inputs (module docstring), by the
    formulas of k_train_loss's last block; lp (term 3) goes through the device's pow and keeps its tolerance test
    (tests/train_loss_cases.py)"""
    l1_c, l1, l2, _, ml = (np.float32(w) for w in tc.WEIGHTS)
    n3, blocks = np.float64(3 * n), blocks_for(3 * n)
    for kind in ("uniform", "wide"):
        inp = train_inputs(n, kind)
        terms, g = drv.run(inp, tc.WEIGHTS)
        d_c, d_f = inp["tex"] - inp["tar"], inp["tex_fine"] - inp["tar"]
        want = {0: l1_c * np.float32(ordered_sum(np.abs(d_c).astype(np.float64), blocks) / n3),
                1: l1 * np.float32(ordered_sum(np.abs(d_f).astype(np.float64), blocks) / n3)}
        for q, w in want.items():
            print(f"train_loss n={n} {kind} {tc.TERMS[q]}: got {terms[q]!r}, order model {w!r}")
            assert bits(np.float32(terms[q])) == bits(np.float32(w)), (kind, tc.TERMS[q], terms[q], w)
        assert bits(g["d_tex"]) == bits(sign_gradient(d_c, l1_c / np.float32(3 * n)))
        assert bits(g["d_tex_fine"][0]) == bits(sign_gradient(d_f, l1 / np.float32(3 * n)))
    inp = train_inputs(n, "grid")
    terms, _ = drv.run(inp, tc.WEIGHTS, want=())
    dd = inp["tex_fine"].astype(np.float64) - inp["tar"].astype(np.float64)

    def mask_sum(a):
        c = np.clip(a, np.float32(1e-3), np.float32(1.0))
        e = c.astype(np.float64) - inp["tar_alpha"].astype(np.float64)
        assert (c == a).all()                                            # inside the band: exact squares (module docstring)
        return ordered_sum(e * e, blocks)

    want = {2: np.float32(np.float64(l2) * ordered_sum(dd * dd, blocks) / n3),
            4: np.float32(np.float64(ml) * mask_sum(inp["alpha"]) / np.float64(n)),
            5: np.float32(np.float64(ml) * mask_sum(inp["alpha_fine"]) / np.float64(n))}
    for q, w in want.items():
        print(f"train_loss n={n} grid {tc.TERMS[q]}: got {terms[q]!r}, order model {w!r}")
    for q, w in want.items():
        assert bits(np.float32(terms[q])) == bits(np.float32(w)), (tc.TERMS[q], terms[q], w)
