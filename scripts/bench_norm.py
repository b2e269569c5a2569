"""Times the native GroupNorm / InstanceNorm [+ ReLU] (kpn_group_norm_forward / kpn_group_norm_backward) against
torch.nn.functional.group_norm (+ relu) and its autograd, both on channels_last tensors, at the shapes the two image encoders run;
and one ConvBlock(256, 256) forward + backward with encoders.install_native_blocks against the untouched module.

    python scripts/bench_norm.py [--views 3] [--size 512] [--ds 1] [--reps 10] [--inner 5] [--shape H,W,C,G] [--no-blocks] [--out FILE.md]

The shape list restates the host walks of csrc/api_encoders.hip (enc::geo_walk / conv_block / hourglass: GroupNorm(min(32, C), C)
with affine parameters, every one followed by a ReLU; enc::tex_walk for ngf = 64, 3 down, 4 blocks, 2 up: InstanceNorm2d without
parameters), with the number of layers that share a shape.  --shape times that one GroupNorm shape only (for a kernel trace).

Per shape and leg (forward, backward) the two arms alternate: each repetition times `inner` back-to-back calls of one arm between
two device events, then the other arm; the figure is the median over the repetitions, in microseconds per call.  The native
backward is also timed without its dx leg (passes 1 and 2 alone); the difference is pass 3.  Needs a GPU.
"""
import argparse
import collections
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12       # bytes / s: the HBM3E figure the project's other profiles use


def geo_norm_shapes(h, w):
    """{(H, W, C, G, affine): layers} of HGFilterV2(n_stack=1, n_downsample=4) on an (h, w) network input"""
    shapes = collections.OrderedDict()

    def add(H, W, C):
        key = (H, W, C, min(32, C), 1)
        shapes[key] = shapes.get(key, 0) + 1

    def conv_block(H, W, cin, cout):
        for C in (cin, cout // 2, cout // 4) + ((cin,) if cin != cout else ()):
            add(H, W, C)

    def hourglass(level, H, W):
        conv_block(H, W, 256, 256)                       # b1
        conv_block(H // 2, W // 2, 256, 256)             # b2
        if level > 1:
            hourglass(level - 1, H // 2, W // 2)
        else:
            conv_block(H // 2, W // 2, 256, 256)         # b2_plus
        conv_block(H // 2, W // 2, 256, 256)             # b3

    add(h // 2, w // 2, 64)                              # bn1
    conv_block(h // 2, w // 2, 64, 128)                  # conv2
    add(h, w, 32)                                        # unpack1.norm
    conv_block(h // 4, w // 4, 128, 128)                 # conv3
    conv_block(h // 4, w // 4, 128, 256)                 # conv4
    hourglass(4, h // 4, w // 4)                         # m0
    conv_block(h // 4, w // 4, 256, 256)                 # top_m_0
    add(h // 4, w // 4, 256)                             # bn_end0
    return shapes


def tex_norm_shapes(h, w, ngf=64, n_down=3, n_blocks=4, n_up=2):
    """{(H, W, C, G = C, affine = 0): layers} of ResBlkEncoder on an (h, w) network input"""
    shapes = collections.OrderedDict()

    def add(H, W, C, n=1):
        key = (H, W, C, C, 0)
        shapes[key] = shapes.get(key, 0) + n

    C = ngf
    add(h, w, C)
    for _ in range(n_down):
        h, w, C = (h - 1) // 2 + 1, (w - 1) // 2 + 1, 2 * C
        add(h, w, C)
    add(h, w, C, 2 * n_blocks)
    for _ in range(n_up):
        h, w, C = 2 * h, 2 * w, C // 2
        add(h, w, C)
    return shapes


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def alternate(arms, reps, inner):
    """medians (us per call) of arms that take turns per repetition"""
    for _ in range(3):
        for fn in arms:
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in arms]
    for _ in range(reps):
        for i, fn in enumerate(arms):
            t[i].append(timed(fn, inner))
    return [statistics.median(v) for v in t]


def bench_shape(ops, N, H, W, C, G, affine, relu, gen, reps, inner):
    cl = torch.channels_last
    x = torch.randn(N, C, H, W, device="cuda", generator=gen).contiguous(memory_format=cl)
    dy = torch.randn(N, C, H, W, device="cuda", generator=gen).contiguous(memory_format=cl)
    w = torch.randn(C, device="cuda", generator=gen) if affine else None
    b = torch.randn(C, device="cuda", generator=gen) if affine else None
    eps = 1e-5
    _, stats = ops.group_norm_forward(x, w, b, G, eps, relu)
    xt = x.clone().requires_grad_(True)
    wt, bt = (w.clone().requires_grad_(True), b.clone().requires_grad_(True)) if affine else (None, None)

    def torch_fwd():
        y = F.group_norm(xt, G, wt, bt, eps)
        return F.relu(y) if relu else y

    yt = torch_fwd()
    leaves = [xt] + ([wt, bt] if affine else [])
    torch_bwd = lambda: torch.autograd.grad(yt, leaves, dy, retain_graph=True)
    native_fwd = lambda: ops.group_norm_forward(x, w, b, G, eps, relu)
    native_bwd = lambda: ops.group_norm_backward(x, dy, w, stats, G, eps, relu)
    native_bwd_nodx = lambda: ops.group_norm_backward(x, dy, w, stats, G, eps, relu, want_dx=False, want_dw=True, want_db=True)
    # the two arms compute the same thing (largest deviation relative to the largest value, for the record)
    dev = {"fwd": float((native_fwd()[0] - yt).abs().max() / yt.abs().max()),
           "dx": float((native_bwd()[0] - torch_bwd()[0]).abs().max() / torch_bwd()[0].abs().max())}
    fn, ft = alternate([native_fwd, torch_fwd], reps, inner)
    if affine:
        bn, bt_, b12 = alternate([native_bwd, torch_bwd, native_bwd_nodx], reps, inner)
    else:
        (bn, bt_), b12 = alternate([native_bwd, torch_bwd], reps, inner), float("nan")
    n = N * H * W * C
    return dict(us=dict(fwd=dict(native=fn, torch=ft), bwd=dict(native=bn, torch=bt_), bwd_pass12=b12), max_rel_dev=dev,
                hbm_frac=dict(fwd=12.0 * n / (fn * 1e-6) / HBM_PEAK, bwd=20.0 * n / (bn * 1e-6) / HBM_PEAK))


def bench_block(N, hw, reps, inner):
    from keypointnerf_amd import encoders
    from tests.encoder_golden import ConvBlock
    torch.manual_seed(0)
    ref = ConvBlock(256, 256).cuda()
    nat = copy.deepcopy(ref)
    served, left = encoders.install_native_blocks(nat)
    assert served == [""] and not left
    x = torch.randn(N, 256, hw, hw, device="cuda").contiguous(memory_format=torch.channels_last)
    g = torch.randn(N, 256, hw, hw, device="cuda").contiguous(memory_format=torch.channels_last)

    def step(net):
        def run():
            xx = x.detach().requires_grad_(True)
            net.zero_grad(set_to_none=True)
            net(xx).backward(g)
        return run

    tn, tt = alternate([step(nat), step(ref)], reps, inner)
    return dict(hw=hw, N=N, us=dict(native=tn, torch=tt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--no-blocks", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_norm.py needs a GPU: a time measured anywhere else says nothing")
    from keypointnerf_amd import ops
    N, hw = args.views, args.size >> args.ds
    gen = torch.Generator(device="cuda").manual_seed(0)
    if args.shape:
        H, W, C, G = (int(v) for v in args.shape.split(","))
        sets = [("one shape", {(H, W, C, G, 1): 1}, 1)]
    else:
        sets = [("geometry encoder, GroupNorm + ReLU", geo_norm_shapes(hw, hw), 1), ("texture encoder, InstanceNorm2d + ReLU", tex_norm_shapes(hw, hw), 1)]
    rows, lines = [], []
    for title, shapes, relu in sets:
        lines.append(f"\n{title} (N = {N})\n")
        lines.append("| shape | layers | fwd native / torch (us) | bwd native / torch (us) | native bwd passes 1+2 (us) | fwd + bwd ratio | "
                     "fwd / bwd bytes over time, of HBM peak |")
        lines.append("|---|---|---|---|---|---|---|")
        for (H, W, C, G, affine), count in shapes.items():
            r = bench_shape(ops, N, H, W, C, G, affine, relu, gen, args.reps, args.inner)
            u = r["us"]
            name = f"C {C} G {G} @ {H}x{W}"
            r.update(shape=name, set=title, N=N, H=H, W=W, C=C, G=G, affine=affine, relu=relu, layers=count)
            rows.append(r)
            sn, st = u["fwd"]["native"] + u["bwd"]["native"], u["fwd"]["torch"] + u["bwd"]["torch"]
            lines.append(f"| {name} | {count} | {u['fwd']['native']:.1f} / {u['fwd']['torch']:.1f} | {u['bwd']['native']:.1f} / {u['bwd']['torch']:.1f} | "
                         f"{u['bwd_pass12']:.1f} | {sn / st:.2f} | {r['hbm_frac']['fwd']:.3f} / {r['hbm_frac']['bwd']:.3f} |")
            print(lines[-1], flush=True)
    tot_n = sum(r["layers"] * (r["us"]["fwd"]["native"] + r["us"]["bwd"]["native"]) for r in rows)
    tot_t = sum(r["layers"] * (r["us"]["fwd"]["torch"] + r["us"]["bwd"]["torch"]) for r in rows)
    lines.append(f"\nAll listed layers, forward + backward, weighted by the number of layers: native {tot_n / 1000:.2f} ms, torch {tot_t / 1000:.2f} ms.")
    lines.append("Largest deviation between the arms, relative to the largest value: " +
                 ", ".join(f"{leg} {max(r['max_rel_dev'][leg] for r in rows):.1e}" for leg in ("fwd", "dx")) + ".")
    blocks = []
    if not args.no_blocks and not args.shape:
        lines.append(f"\nConvBlock(256, 256), forward + backward (N = {N})\n")
        lines.append("| size | install_native_blocks (us) | untouched module (us) | ratio |")
        lines.append("|---|---|---|---|")
        for s in (64, 16):
            b = bench_block(N, s, args.reps, args.inner)
            blocks.append(b)
            lines.append(f"| {s}x{s} | {b['us']['native']:.1f} | {b['us']['torch']:.1f} | {b['us']['native'] / b['us']['torch']:.2f} |")
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
        with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
            json.dump(dict(norms=rows, blocks=blocks), f, indent=1)
    print(json.dumps({"bench": "norm", "native_ms": tot_n / 1000, "torch_ms": tot_t / 1000, "shapes": len(rows)}))


if __name__ == "__main__":
    main()
