"""Times training (forward + backward) through the layers that kpn_conv2d_s2_* serves, and through a whole HGFilterV2, on one
3 x 3 x 512^2 source set (network input 256^2 for the geometry encoder, ds = 1).

    python scripts/bench_geo_training.py layers [--reps 10] [--inner 5] [--out FILE.md]
    python scripts/bench_geo_training.py net    [--reps 10] [--fused-blocks] [--arith bf16x3] [--out FILE.md]

layers: the three new layer kinds at the shapes of the geometry encoder (conv1, unpack1.conv) and of the texture encoder (its three
        stride-2 convolutions and two transposed ones), torch.ops.kpnerf.conv2d_down2 / conv_transpose2d_up2 under autograd against
        torch.nn.functional.conv2d / conv_transpose2d (MIOpen) on channels_last tensors.  One call is a forward and a backward that
        yields every gradient the layer has (the stem: dW and db only, on both arms).
net:    tests/encoder_golden.HGFilterV2 with encoders.install_native_geo against the untouched module on channels_last tensors
        (and, for the record, against the module with channels_last weights and against NCHW tensors), forward + backward to
        every parameter gradient.  --fused-blocks installs the ConvBlocks as single operators; --arith bf16x3 adds an arm with the
        stride-1 convolutions and the blocks on three bf16 pieces per operand (install_native_geo(arith="bf16x3")).

The two arms alternate: each repetition times `inner` back-to-back calls of one arm between two device events, then the other arm;
the figure is the median over the repetitions.  Run each mode under a time limit of its own.  Needs a GPU.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, kind, cin, cout, H, W of the input, bias) on N = 3 views
LAYERS = (
    ("geo conv1: 7x7 s2 3->64 @ 256", "stem", 3, 64, 256, 256, True),
    ("geo unpack1: convT 128->32 @ 128", "up", 128, 32, 128, 128, False),
    ("tex down1: 3x3 s2 64->128 @ 256", "down", 64, 128, 256, 256, True),
    ("tex down2: 3x3 s2 128->256 @ 128", "down", 128, 256, 128, 128, True),
    ("tex down3: 3x3 s2 256->512 @ 64", "down", 256, 512, 64, 64, True),
    ("tex up1: convT 512->256 @ 32", "up", 512, 256, 32, 32, True),
    ("tex up2: convT 256->128 @ 64", "up", 256, 128, 64, 64, True),
)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def alternate(native, torch_arm, reps, inner, warm=3):
    for _ in range(warm):
        native(), torch_arm()
    torch.cuda.synchronize()
    tn, tt = [], []
    for _ in range(reps):
        tn.append(timed(native, inner))
        tt.append(timed(torch_arm, inner))
    return statistics.median(tn), statistics.median(tt), (min(tn), max(tn)), (min(tt), max(tt))


def bench_layers(args):
    import keypointnerf_amd.torch_ops  # noqa: F401
    N, cl = args.views, torch.channels_last
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, lines = [], [f"| layer (N = {N}) | native fwd+bwd (us) | torch fwd+bwd (us) | native / torch | max rel. dev y, dw |", "|---|---|---|---|---|"]
    for name, kind, cin, cout, H, W, bias in LAYERS:
        x = torch.randn(N, cin, H, W, device="cuda", generator=gen)
        x = (x if kind == "stem" else x.contiguous(memory_format=cl)).requires_grad_(kind != "stem")
        w = (torch.randn((cin, cout, 3, 3) if kind == "up" else (cout, cin, 7 if kind == "stem" else 3, 7 if kind == "stem" else 3),
                         device="cuda", generator=gen) * 0.05).requires_grad_(True)
        b = torch.randn(cout, device="cuda", generator=gen).requires_grad_(True) if bias else None
        if kind == "up":
            fn_n = lambda: torch.ops.kpnerf.conv_transpose2d_up2(x, w, b)                                      # noqa: E731
            fn_t = lambda: F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)                   # noqa: E731
        else:
            fn_n = lambda: torch.ops.kpnerf.conv2d_down2(x, w, b)                                              # noqa: E731
            fn_t = lambda: F.conv2d(x, w, b, stride=2, padding=3 if kind == "stem" else 1)                      # noqa: E731
        leaves = [t for t in (x, w, b) if t is not None and t.requires_grad]
        dy = torch.randn_like(fn_n()).contiguous(memory_format=cl)
        step = lambda fn: torch.autograd.grad(fn(), leaves, dy)                                                # noqa: E731
        y_n, y_t = fn_n().detach(), fn_t().detach()
        dw_n, dw_t = step(fn_n)[-2 if bias else -1], step(fn_t)[-2 if bias else -1]
        dev = (float((y_n - y_t).abs().max() / y_t.abs().max()), float((dw_n - dw_t).abs().max() / dw_t.abs().max()))
        mn, mt, rn, rt = alternate(lambda: step(fn_n), lambda: step(fn_t), args.reps, args.inner)
        rows.append(dict(layer=name, native_us=mn, torch_us=mt, native_range_us=rn, torch_range_us=rt, max_rel_dev=dev))
        lines.append(f"| {name} | {mn:.1f} ({rn[0]:.1f} .. {rn[1]:.1f}) | {mt:.1f} ({rt[0]:.1f} .. {rt[1]:.1f}) | {mn / mt:.2f} | {dev[0]:.1e}, {dev[1]:.1e} |")
        print(lines[-1], flush=True)
    return rows, lines


def bench_net(args):
    from keypointnerf_amd import encoders
    from tests import encoder_golden as eg
    cl = torch.channels_last
    hw = args.size >> 1
    native = eg.stand_in_geo(1).train().cuda()
    plain = copy.deepcopy(native)                               # the untouched module
    plain_cl = copy.deepcopy(native).to(memory_format=cl)       # ... and with its weights channels_last as well
    report = encoders.install_native_geo(native, fused_blocks=args.fused_blocks)
    left = {k: v[1] for k, v in report.items() if v[1]}
    how = "install_native_geo" + ("(fused_blocks=True)" if args.fused_blocks else "")
    x_nchw = eg.net_input(eg.case_image((args.views, 3, args.size, args.size), 1).cuda(), 1).contiguous()
    x = x_nchw.contiguous(memory_format=cl)
    gen = torch.Generator(device="cuda").manual_seed(0)
    gs = [torch.randn(args.views, 64, hw // 4, hw // 4, device="cuda", generator=gen).contiguous(memory_format=cl),
          torch.randn(args.views, 8, hw, hw, device="cuda", generator=gen).contiguous(memory_format=cl)]
    gs_nchw = [g.contiguous() for g in gs]

    def step(net, x, gs):
        return torch.autograd.grad(net(x), list(net.parameters()), gs, allow_unused=True)

    def forward(net, x, gs):
        with torch.no_grad():
            return net(x)

    split = ()
    if args.arith:
        net3 = copy.deepcopy(plain)
        encoders.install_native_geo(net3, fused_blocks=args.fused_blocks, arith=args.arith)
        split = ((f"native ({how}, arith={args.arith}), channels_last tensors", net3, x, gs),)
    arms = ((f"native ({how}), channels_last tensors", native, x, gs),) + split + (
            ("torch, untouched module, channels_last tensors", plain, x, gs),
            ("torch, weights channels_last too", plain_cl, x, gs),
            ("torch, untouched module, NCHW tensors", plain, x_nchw, gs_nchw))
    rows, lines = [], [f"| HGFilterV2, {args.views} x 3 x {hw}^2 input | " + " | ".join(a[0] + " (ms)" for a in arms) + " |", "|---|" + "---|" * len(arms)]
    for what, fn in (("forward + backward", step), ("forward alone (no_grad)", forward)):
        for _ in range(3):
            for _, net, xx, gg in arms:
                fn(net, xx, gg)
        torch.cuda.synchronize()
        ts = [[] for _ in arms]
        for _ in range(args.reps):                              # the arms alternate within every repetition
            for t, (_, net, xx, gg) in zip(ts, arms):
                t.append(timed(lambda: fn(net, xx, gg), 1) / 1000.0)
        rows.append(dict(what=what, ms={a[0]: dict(median=statistics.median(t), min=min(t), max=max(t)) for a, t in zip(arms, ts)}))
        lines.append(f"| {what} | " + " | ".join(f"{statistics.median(t):.2f} ({min(t):.2f} .. {max(t):.2f})" for t in ts) + " |")
        print(lines[-1], flush=True)
    lines.append(f"\nLayers left on torch by install_native_geo: {left or 'none'}.")
    return rows, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("layers", "net"))
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--fused-blocks", action="store_true")
    ap.add_argument("--arith", choices=("bf16x3",), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geo_training.py needs a GPU: a time measured anywhere else says nothing")
    rows, lines = (bench_layers if args.mode == "layers" else bench_net)(args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "geo_training_" + args.mode, "rows": rows}))


if __name__ == "__main__":
    main()
