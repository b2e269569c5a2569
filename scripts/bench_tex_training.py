"""Times training (forward + backward) through the layers that kpn_conv2d_rp_* serves, the adjoint load against the zero-padded input
gradient, and a whole ResBlkEncoder, on one 3 x 3 x 512^2 source set (network input 256^2 for the texture encoder, ds = 1).

    python scripts/bench_tex_training.py layers  [--reps 10] [--inner 5] [--out FILE.md]
    python scripts/bench_tex_training.py adjoint [--reps 10] [--inner 5] [--out FILE.md]
    python scripts/bench_tex_training.py net     [--reps 10] [--out FILE.md]

layers:  the three replication-padded layers at the shipped widths (tests/encoder_golden.TEX_ARGS): the stem 3 -> 64 at 256^2, a ResBlk
         convolution 512 -> 512 at 32^2, the output layer 128 -> 8 at 128^2; torch.ops.kpnerf.conv2d_replicate under autograd against
         F.conv2d(F.pad(x, mode="replicate")) (MIOpen) on channels_last tensors (the stem: NCHW on both arms).  One call is a forward and
         a backward that yields every gradient the layer has (the stem: dW and db only, on both arms).
adjoint: the input gradient alone, kpn_conv2d_rp_backward(KPN_RP_CONV3) against kpn_conv2d_backward(k 3, pad 1) at the same shapes: the
         same GEMM, only the loads of the outermost ring of pixels differ.
net:     tests/encoder_golden.ResBlkEncoder with encoders.install_native_tex, and with install_native_tex(fused=True) (one
         torch.ops.kpnerf.res_encoder per forward), against the untouched module, on channels_last and on NCHW tensors, forward + backward
         to every parameter gradient, and forward alone; and each arm's peak memory above parameters and inputs over one training step.

The arms alternate: each repetition times `inner` back-to-back calls of one arm between two device events, then the next arm; the
figure is the median over the repetitions.  Run each mode under a time limit of its own.  Needs a GPU.
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

# (name, k, cin, cout, H = W of the input, stem) on N = 3 views
LAYERS = (
    ("stem: pad 3 + 7x7 3->64 @ 256", 7, 3, 64, 256, True),
    ("ResBlk conv: pad 1 + 3x3 512->512 @ 32", 3, 512, 512, 32, False),
    ("output: pad 3 + 7x7 128->8 @ 128", 7, 128, 8, 128, False),
)
# (cin = cout, H = W): the ResBlk convolution as shipped, and two wider grids of the same layer kind for the ring's share
ADJOINT = ((512, 32), (128, 64), (64, 128))


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def alternate(arms, reps, inner, warm=3):
    """arms: callables -> [(median, min, max) in us per arm]; the arms alternate within every repetition"""
    for _ in range(warm):
        for fn in arms:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in arms]
    for _ in range(reps):
        for t, fn in zip(ts, arms):
            t.append(timed(fn, inner))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def cell(m, scale=1.0, digits=1):
    return f"{m[0] * scale:.{digits}f} ({m[1] * scale:.{digits}f} .. {m[2] * scale:.{digits}f})"


def bench_layers(args):
    import keypointnerf_amd.torch_ops  # noqa: F401
    N, cl = args.views, torch.channels_last
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, lines = [], [f"| layer (N = {N}) | native fwd+bwd (us) | torch fwd+bwd (us) | native / torch | max rel. dev y, dw |", "|---|---|---|---|---|"]
    for name, k, cin, cout, hw, stem in LAYERS:
        x = torch.randn(N, cin, hw, hw, device="cuda", generator=gen)
        x = (x if stem else x.contiguous(memory_format=cl)).requires_grad_(not stem)
        w = (torch.randn(cout, cin, k, k, device="cuda", generator=gen) * 0.05).requires_grad_(True)
        b = torch.randn(cout, device="cuda", generator=gen).requires_grad_(True)
        p = k // 2
        fn_n = lambda: torch.ops.kpnerf.conv2d_replicate(x, w, b)                                              # noqa: E731
        fn_t = lambda: F.conv2d(F.pad(x, (p, p, p, p), mode="replicate"), w, b)                                # noqa: E731
        leaves = [t for t in (x, w, b) if t.requires_grad]
        dy = torch.randn_like(fn_n()).contiguous(memory_format=cl)
        step = lambda fn: torch.autograd.grad(fn(), leaves, dy)                                                # noqa: E731
        y_n, y_t = fn_n().detach(), fn_t().detach()
        dw_n, dw_t = step(fn_n)[-2], step(fn_t)[-2]
        dev = (float((y_n - y_t).abs().max() / y_t.abs().max()), float((dw_n - dw_t).abs().max() / dw_t.abs().max()))
        mn, mt = alternate((lambda: step(fn_n), lambda: step(fn_t)), args.reps, args.inner)
        rows.append(dict(layer=name, native_us=mn, torch_us=mt, max_rel_dev=dev))
        lines.append(f"| {name} | {cell(mn)} | {cell(mt)} | {mn[0] / mt[0]:.2f} | {dev[0]:.1e}, {dev[1]:.1e} |")
        print(lines[-1], flush=True)
    return rows, lines


def bench_adjoint(args):
    """dX alone through the two C-ABI paths: the replication-padded layer's adjoint load, and the zero-padded layer's plain load.  The
    zero-padded arm is listed twice (it runs twice per repetition): the gap between its two columns is the run-to-run spread the ratio
    is read against."""
    from keypointnerf_amd import ops
    from keypointnerf_amd import lib as kl
    N, cl = args.views, torch.channels_last
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, lines = [], [f"| 3x3 C->C, dX alone (N = {N}) | replicate: adjoint load (us) | zero padding (us) | zero padding, again (us) | adjoint / zero | "
                       "again / zero | max rel. dev on the interior |", "|---|---|---|---|---|---|---|"]
    for C, hw in ADJOINT:
        w = torch.randn(C, C, 3, 3, device="cuda", generator=gen) * 0.05
        dy = torch.randn(N, C, hw, hw, device="cuda", generator=gen).contiguous(memory_format=cl)
        p_rp, p_z = ops.conv2d_rp_pack(w, kl.RP_CONV3), ops.conv2d_pack(w)
        fn_rp = lambda: ops.conv2d_rp_backward(None, dy, p_rp, (N, C, hw, hw), kl.RP_CONV3, False, True, False, False)[0]   # noqa: E731
        fn_z = lambda: ops.conv2d_backward(None, dy, p_z, C, 3, 1, False, True, False, False)[0]                            # noqa: E731
        a, z = fn_rp(), fn_z()
        dev = float((a - z)[:, :, 1:-1, 1:-1].abs().max() / z.abs().max())
        m_rp, m_z, m_z2 = alternate((fn_rp, fn_z, fn_z), args.reps, args.inner)
        rows.append(dict(C=C, hw=hw, adjoint_us=m_rp, zero_us=m_z, zero_again_us=m_z2, interior_dev=dev))
        lines.append(f"| {C} @ {hw} | {cell(m_rp)} | {cell(m_z)} | {cell(m_z2)} | {m_rp[0] / m_z[0]:.3f} | {m_z2[0] / m_z[0]:.3f} | {dev:.1e} |")
        print(lines[-1], flush=True)
    return rows, lines


def bench_net(args):
    from keypointnerf_amd import encoders
    from tests import encoder_golden as eg
    cl = torch.channels_last
    hw = args.size >> 1
    native = eg.stand_in_tex(1).train().cuda()
    plain = copy.deepcopy(native)                               # the untouched module
    fused = copy.deepcopy(native)
    report = encoders.install_native_tex(native)
    left = {k: v[1] for k, v in report.items() if v[1]}
    assert encoders.install_native_tex(fused, fused=True)["fused"] == ([""], {})
    x_nchw = eg.net_input(eg.case_image((args.views, 3, args.size, args.size), 1).cuda(), 1).contiguous()
    x = x_nchw.contiguous(memory_format=cl)
    a = eg.TEX_ARGS
    ho = (hw >> a["n_downsample"]) << a["n_upsample"]
    g = torch.randn(args.views, a["out_ch"], ho, ho, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)).contiguous(memory_format=cl)
    g_nchw = g.contiguous()

    def step(net, x, g):
        return torch.autograd.grad(net(x), list(net.parameters()), g)

    def forward(net, x, g):
        with torch.no_grad():
            return net(x)

    arms = (("native (install_native_tex), channels_last tensors", native, x, g),
            ("native (install_native_tex), NCHW tensors", native, x_nchw, g_nchw),
            ("native fused (install_native_tex(fused=True)), channels_last tensors", fused, x, g),
            ("native fused (install_native_tex(fused=True)), NCHW tensors", fused, x_nchw, g_nchw),
            ("torch, untouched module, channels_last tensors", plain, x, g),
            ("torch, untouched module, NCHW tensors", plain, x_nchw, g_nchw))
    calls = encoders.NativeTraining.tex_calls, encoders.NativeTraining.fused_tex_calls
    rows, lines = [], [f"| ResBlkEncoder, {args.views} x 3 x {hw}^2 input | " + " | ".join(a[0] + " (ms)" for a in arms) + " |", "|---|" + "---|" * len(arms)]
    for what, fn in (("forward + backward", step), ("forward alone (no_grad)", forward)):
        ms = alternate([lambda net=net, xx=xx, gg=gg: fn(net, xx, gg) for _, net, xx, gg in arms], args.reps, 1)
        rows.append(dict(what=what, ms={a[0]: dict(median=m[0] / 1000.0, min=m[1] / 1000.0, max=m[2] / 1000.0) for a, m in zip(arms, ms)}))
        lines.append(f"| {what} | " + " | ".join(cell(m, 1e-3, 2) for m in ms) + " |")
        print(lines[-1], flush=True)
    # peak memory of one training step above what is resident before it (parameters, inputs, the packed weights of earlier calls)
    peaks = []
    for _, net, xx, gg in arms:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        grads = step(net, xx, gg)
        torch.cuda.synchronize()
        peaks.append((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20)
        del grads
    rows.append(dict(what="peak memory of forward + backward (MiB)", mib={a[0]: p for a, p in zip(arms, peaks)}))
    lines.append("| peak memory of forward + backward above parameters and inputs (MiB) | " + " | ".join(f"{p:.0f}" for p in peaks) + " |")
    print(lines[-1], flush=True)
    assert encoders.NativeTraining.tex_calls > calls[0] and encoders.NativeTraining.fused_tex_calls > calls[1]    # served natively
    lines.append(f"\nLayers left on torch by install_native_tex: {left or 'none'}.")
    return rows, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("layers", "adjoint", "net"))
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tex_training.py needs a GPU: a time measured anywhere else says nothing")
    rows, lines = {"layers": bench_layers, "adjoint": bench_adjoint, "net": bench_net}[args.mode](args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "tex_training_" + args.mode, "rows": rows}))


if __name__ == "__main__":
    main()
