"""Times the native resampling steps of an HourGlass (kpn_avg_pool2_* / kpn_upsample2x_add_*) against torch.nn.functional.avg_pool2d
and up1 + torch.nn.functional.interpolate(bicubic, align_corners=True) with their autograd, both on channels_last tensors, at the
hourglass levels of the geometry encoder; and one whole HourGlass(4, 256) forward + backward untouched, with
encoders.install_native_hourglass alone, and with install_native_hourglass + install_native_blocks.

    python scripts/bench_resample.py [--views 3] [--size 512] [--ds 1] [--reps 10] [--inner 5] [--no-hourglass] [--out FILE.md]

The shape list restates enc::geo_walk / enc::hourglass of csrc/api_encoders.hip: the network input is size >> ds, conv1 halves it,
the pool in front of conv3 halves it again, and the four levels of HourGlass(4, 256) pool from that size down (512, ds = 1: high
sizes 64, 32, 16, 8 at 256 channels).

Per shape and leg the two arms alternate: each repetition times `inner` back-to-back calls of one arm between two device events,
then the other arm; the figure is the median over the repetitions, in microseconds per call.  The arms are channels_last on both
sides; torch's upsample and the untouched module are timed on NCHW-contiguous tensors as well, for the record.  Needs a GPU.
"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_norm import HBM_PEAK, alternate  # noqa: E402  (one protocol)


def hourglass_levels(size, ds, depth=4):
    """high sizes of the `depth` levels of the geometry encoder's HourGlass on a (size, size) source"""
    top = (size >> ds) // 4
    return [top >> k for k in range(depth)]


def bench_level(ops, N, C, S, gen, reps, inner):
    cl = torch.channels_last
    r = lambda s: torch.randn(N, C, s, s, device="cuda", generator=gen).contiguous(memory_format=cl)
    x, skip, g_high, low, g_low = r(S), r(S), r(S), r(S // 2), r(S // 2)
    xt, lowt, skipt = (t.clone().requires_grad_(True) for t in (x, low, skip))
    torch_pool = lambda: F.avg_pool2d(xt, 2, stride=2)
    torch_up = lambda: skipt + F.interpolate(lowt, scale_factor=2, mode="bicubic", align_corners=True)
    py, uy = torch_pool(), torch_up()
    torch_pool_bwd = lambda: torch.autograd.grad(py, xt, g_low, retain_graph=True)
    torch_up_bwd = lambda: torch.autograd.grad(uy, [lowt, skipt], g_high, retain_graph=True)
    # for the record, torch's upsample on NCHW-contiguous tensors (the arms of the issue are channels_last: what a ConvBlock hands on)
    lowc, skipc, g_highc = lowt.detach().contiguous().requires_grad_(True), skipt.detach().contiguous().requires_grad_(True), g_high.contiguous()
    torch_up_c = lambda: skipc + F.interpolate(lowc, scale_factor=2, mode="bicubic", align_corners=True)
    uyc = torch_up_c()
    torch_up_bwd_c = lambda: torch.autograd.grad(uyc, [lowc, skipc], g_highc, retain_graph=True)
    nchw = dict(up_fwd=torch_up_c, up_bwd=torch_up_bwd_c)
    native = dict(pool_fwd=lambda: ops.avg_pool2_forward(x), pool_bwd=lambda: ops.avg_pool2_backward(g_low),
                  up_fwd=lambda: ops.upsample2x_add_forward(low, skip), up_bwd=lambda: ops.upsample2x_add_backward(g_high))
    torch_ = dict(pool_fwd=torch_pool, pool_bwd=torch_pool_bwd, up_fwd=torch_up, up_bwd=torch_up_bwd)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    dev = dict(pool_fwd=rel(native["pool_fwd"](), py), pool_bwd=rel(native["pool_bwd"](), torch_pool_bwd()[0]),
               up_fwd=rel(native["up_fwd"](), uy), up_bwd=rel(native["up_bwd"](), torch_up_bwd()[0]))
    n_hi = N * C * S * S
    # bytes a leg has to move: the pool and both backwards read or write one high and one low tensor, the upsample-add two high and one low
    bytes_ = dict(pool_fwd=5 * n_hi, pool_bwd=5 * n_hi, up_fwd=9 * n_hi, up_bwd=5 * n_hi)
    us, frac = {}, {}
    for leg in ("pool_fwd", "pool_bwd", "up_fwd", "up_bwd"):
        if leg in nchw:
            tn, tt, tc = alternate([native[leg], torch_[leg], nchw[leg]], reps, inner)
        else:
            (tn, tt), tc = alternate([native[leg], torch_[leg]], reps, inner), None
        us[leg] = dict(native=tn, torch=tt, torch_nchw=tc)
        frac[leg] = bytes_[leg] / (tn * 1e-6) / HBM_PEAK
    return dict(us=us, max_rel_dev=dev, hbm_frac=frac)


def bench_hourglass(N, S, reps, inner):
    from keypointnerf_amd import encoders
    from tests.encoder_golden import HourGlass
    torch.manual_seed(0)
    ref = HourGlass(4, 256).cuda()
    hg, both = copy.deepcopy(ref), copy.deepcopy(ref)
    served, left = encoders.install_native_hourglass(hg)
    assert served == [""] and not left
    assert encoders.install_native_hourglass(both)[0] == [""] and len(encoders.install_native_blocks(both)[0]) == 13
    cl = torch.channels_last
    x = torch.randn(N, 256, S, S, device="cuda").contiguous(memory_format=cl)
    g = torch.randn(N, 256, S, S, device="cuda").contiguous(memory_format=cl)

    def step(net):
        def run():
            xx = x.detach().requires_grad_(True)
            net.zero_grad(set_to_none=True)
            net(xx).backward(g)
        return run

    xc, gc = x.contiguous(), g.contiguous()

    def step_nchw():
        xx = xc.detach().requires_grad_(True)
        ref.zero_grad(set_to_none=True)
        ref(xx).backward(gc)

    t_ref, t_hg, t_both, t_refc = alternate([step(ref), step(hg), step(both), step_nchw], reps, inner)
    return dict(N=N, size=S, us=dict(untouched=t_ref, hourglass=t_hg, hourglass_blocks=t_both, untouched_nchw=t_refc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-hourglass", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a GPU: a time measured anywhere else says nothing")
    from keypointnerf_amd import ops
    N, C = args.views, 256
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, lines = [], []
    lines.append(f"\nHourGlass levels of the geometry encoder (N = {N}, C = {C}), microseconds per call, native / torch\n")
    lines.append("| high size | pool fwd | pool bwd | upsample-add fwd | upsample bwd | all four, ratio | bytes over time of HBM peak: "
                 "pool fwd / pool bwd / up fwd / up bwd |")
    lines.append("|---|---|---|---|---|---|---|")
    legs = ("pool_fwd", "pool_bwd", "up_fwd", "up_bwd")
    for S in hourglass_levels(args.size, args.ds):
        r = bench_level(ops, N, C, S, gen, args.reps, args.inner)
        r.update(N=N, C=C, size=S)
        rows.append(r)
        u = r["us"]
        sn, st = sum(u[k]["native"] for k in legs), sum(u[k]["torch"] for k in legs)
        lines.append(f"| {S}x{S} | " + " | ".join(f"{u[k]['native']:.1f} / {u[k]['torch']:.1f}" for k in legs) + f" | {sn / st:.4f} | " +
                     " / ".join(f"{r['hbm_frac'][k]:.3f}" for k in legs) + " |")
        print(lines[-1], flush=True)
    tot_n = sum(r["us"][k]["native"] for r in rows for k in legs)
    tot_t = sum(r["us"][k]["torch"] for r in rows for k in legs)
    lines.append(f"\nAll four levels, the four legs each: native {tot_n:.1f} us, torch {tot_t:.1f} us.")
    lines.append("torch's upsample-add on NCHW-contiguous tensors instead, fwd / bwd (us): " +
                 ", ".join(f"{r['size']}x{r['size']} {r['us']['up_fwd']['torch_nchw']:.1f} / {r['us']['up_bwd']['torch_nchw']:.1f}" for r in rows) + ".")
    lines.append("Largest deviation between the arms, relative to the largest value: " +
                 ", ".join(f"{k} {max(r['max_rel_dev'][k] for r in rows):.1e}" for k in legs) + ".")
    hg = None
    if not args.no_hourglass:
        hg = bench_hourglass(N, (args.size >> args.ds) // 4, args.reps, args.inner)
        u = hg["us"]
        lines.append(f"\nHourGlass(4, 256), forward + backward at {N} x 256 x {hg['size']} x {hg['size']}\n")
        lines.append("| untouched module (us) | install_native_hourglass (us) | + install_native_blocks (us) | ratios to untouched | "
                     "untouched module, NCHW-contiguous input (us) |")
        lines.append("|---|---|---|---|---|")
        lines.append(f"| {u['untouched']:.1f} | {u['hourglass']:.1f} | {u['hourglass_blocks']:.1f} | "
                     f"{u['hourglass'] / u['untouched']:.2f} / {u['hourglass_blocks'] / u['untouched']:.2f} | {u['untouched_nchw']:.1f} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
        with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
            json.dump(dict(levels=rows, hourglass=hg), f, indent=1)
    print(json.dumps({"bench": "resample", "native_us": tot_n, "torch_us": tot_t, "levels": len(rows)}))


if __name__ == "__main__":
    main()
