"""Times the native convolution (kpn_conv2d_forward / kpn_conv2d_backward) against torch.nn.functional.conv2d and
aten.convolution_backward (MIOpen), both on channels_last tensors, at the shapes the geometry encoder runs.

    python scripts/bench_conv.py [--views 3] [--size 512] [--ds 1] [--all] [--arith bf16x3] [--reps 10] [--inner 5] [--out FILE.md]

The shape list restates the host walk of csrc/api_encoders.hip (enc::geo_walk / conv_block / hourglass): every stride-1
convolution with a 1x1, 3x3 or 5x5 kernel, with the number of layers that share the shape.  By default the hourglass, top_m_0, the
two heads and conv_out are timed (the bulk of the arithmetic); --all adds the ConvBlocks in front of the hourglass.

Per shape and leg (forward, dX, dW + db) the two arms alternate: each repetition times `inner` back-to-back calls of one arm between
two device events, then the other arm; the figure is the median over the repetitions, in microseconds per call.  Needs a GPU.

--arith bf16x3 adds a third arm between the two: the same calls with arith = CONV_BF16X3 (kpn_conv2d_ex_*, three bf16 pieces per operand
on the 16-bit MFMA); the three arms alternate within every repetition.  The table then carries, per leg, native fp32 / native bf16x3 /
torch, and per native arm the achieved TF-equivalent of the three GEMMs together (fp32 FLOP of the layer, 2 N H W cin cout k^2 per GEMM,
over the time of the leg; dW + db counts the GEMM alone), to be read against 155 TF (fp32 MFMA) and 417 TF-equivalent (six bf16 MFMAs).
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def geo_conv_shapes(h, w, out_ch=64, out_ch_hd=8, everything=False):
    """{(H, W, cin, cout, k, pad, bias): layers} of HGFilterV2(n_stack=1, n_downsample=4) on an (h, w) network input"""
    shapes = collections.OrderedDict()

    def add(H, W, cin, cout, k, pad, bias, on=True):
        if on:
            key = (H, W, cin, cout, k, pad, bias)
            shapes[key] = shapes.get(key, 0) + 1

    def conv_block(H, W, cin, cout, on=True):
        add(H, W, cin, cout // 2, 3, 1, False, on)
        add(H, W, cout // 2, cout // 4, 3, 1, False, on)
        add(H, W, cout // 4, cout // 4, 3, 1, False, on)
        if cin != cout:
            add(H, W, cin, cout, 1, 0, False, on)

    def hourglass(level, H, W):
        conv_block(H, W, 256, 256)                       # b1
        conv_block(H // 2, W // 2, 256, 256)             # b2
        if level > 1:
            hourglass(level - 1, H // 2, W // 2)
        else:
            conv_block(H // 2, W // 2, 256, 256)         # b2_plus
        conv_block(H // 2, W // 2, 256, 256)             # b3

    # conv1 is the 7x7 stride-2 stem and unpack1 a ConvTranspose2d: not served
    conv_block(h // 2, w // 2, 64, 128, everything)      # conv2
    add(h, w, 32, out_ch_hd, 5, 2, True)                 # conv_out
    conv_block(h // 4, w // 4, 128, 128, everything)     # conv3
    conv_block(h // 4, w // 4, 128, 256, everything)     # conv4
    hourglass(4, h // 4, w // 4)                         # m0
    conv_block(h // 4, w // 4, 256, 256)                 # top_m_0
    add(h // 4, w // 4, 256, 256, 1, 0, True)            # conv_last0
    add(h // 4, w // 4, 256, out_ch, 1, 0, True)         # l0
    return shapes


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ds", type=int, default=1)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--arith", choices=("bf16x3",), default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv.py needs a GPU: a time measured anywhere else says nothing")
    from keypointnerf_amd import lib as kl
    from keypointnerf_amd import ops
    L = kl.get_library()
    N, hw = args.views, args.size >> args.ds
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, lines = [], []
    A3 = kl.CONV_BF16X3
    if args.arith:
        lines.append(f"| shape (N = {N}) | layers | ranges f32, bf16x3 | fwd f32 / bf16x3 / torch (us) | dX f32 / bf16x3 / torch | dW+db f32 / bf16x3 / torch | "
                     "sum f32 / bf16x3 / torch | bf16x3 / f32 | bf16x3 / torch | TF-eq fwd, dX, dW: f32 | TF-eq fwd, dX, dW: bf16x3 |")
        lines.append("|---|---|---|---|---|---|---|---|---|---|---|")
    else:
        lines.append(f"| shape (N = {N}) | layers | ranges | fwd native / torch (us) | dX native / torch | dW+db native / torch | sum native / torch | ratio |")
        lines.append("|---|---|---|---|---|---|---|---|")
    for (H, W, cin, cout, k, pad, bias), count in geo_conv_shapes(hw, hw, everything=args.all).items():
        cl = torch.channels_last
        x = torch.randn(N, cin, H, W, device="cuda", generator=gen).contiguous(memory_format=cl)
        w = torch.randn(cout, cin, k, k, device="cuda", generator=gen) * 0.05
        b = torch.randn(cout, device="cuda", generator=gen) if bias else None
        dy = torch.randn(N, cout, H, W, device="cuda", generator=gen).contiguous(memory_format=cl)
        packed = ops.conv2d_pack(w)
        ranges = L.kpn_conv2d_wgrad_ranges(ops._layer_plan(L, "conv2d", (k, pad), cin, cout, N, H, W, bias)[0])
        bsz = [cout] if bias else None
        cb = lambda mask: torch.ops.aten.convolution_backward(dy, x, w, bsz, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)
        arms = {
            "fwd": (lambda: ops.conv2d_forward(x, packed, b, cout, k, pad), lambda: F.conv2d(x, w, b, padding=pad)),
            "dx": (lambda: ops.conv2d_backward(None, dy, packed, cin, k, pad, bias, True, False, False), lambda: cb([True, False, False])),
            "dw": (lambda: ops.conv2d_backward(x, dy, None, cin, k, pad, bias, False, True, True), lambda: cb([False, True, bias])),
        }
        # the two arms compute the same thing (largest deviation relative to the largest value, for the record)
        dev = {}
        y_n, y_t = arms["fwd"][0](), arms["fwd"][1]()
        dev["fwd"] = float((y_n - y_t).abs().max() / y_t.abs().max())
        dev["dx"] = float((arms["dx"][0]()[0] - arms["dx"][1]()[0]).abs().max() / arms["dx"][1]()[0].abs().max())
        dev["dw"] = float((arms["dw"][0]()[1] - arms["dw"][1]()[1]).abs().max() / arms["dw"][1]()[1].abs().max())
        med, med3 = {}, {}
        if args.arith:
            packed3 = ops.conv2d_pack(w, arith=A3)
            ranges3 = L.kpn_conv2d_ex_wgrad_ranges(ops._layer_plan(L, "conv2d", (k, pad), cin, cout, N, H, W, bias)[0], A3)
            arms3 = {
                "fwd": lambda: ops.conv2d_forward(x, packed3, b, cout, k, pad, arith=A3),
                "dx": lambda: ops.conv2d_backward(None, dy, packed3, cin, k, pad, bias, True, False, False, arith=A3),
                "dw": lambda: ops.conv2d_backward(x, dy, None, cin, k, pad, bias, False, True, True, arith=A3),
            }
            dev3 = {"fwd": float((arms3["fwd"]() - y_t).abs().max() / y_t.abs().max()),
                    "dx": float((arms3["dx"]()[0] - arms["dx"][1]()[0]).abs().max() / arms["dx"][1]()[0].abs().max()),
                    "dw": float((arms3["dw"]()[1] - arms["dw"][1]()[1]).abs().max() / arms["dw"][1]()[1].abs().max())}
        for leg, (native, torch_arm) in arms.items():
            trio = [native] + ([arms3[leg]] if args.arith else []) + [torch_arm]
            for _ in range(3):
                for fn in trio:
                    fn()
            torch.cuda.synchronize()
            ts = [[] for _ in trio]
            for _ in range(args.reps):                      # the arms alternate within every repetition
                for t, fn in zip(ts, trio):
                    t.append(timed(fn, args.inner))
            med[leg] = (statistics.median(ts[0]), statistics.median(ts[-1]))
            if args.arith:
                med3[leg] = statistics.median(ts[1])
        sn, st = sum(v[0] for v in med.values()), sum(v[1] for v in med.values())
        name = f"{k}x{k} {cin}->{cout} @ {H}x{W}" + (" +b" if bias else "")
        rows.append(dict(shape=name, N=N, H=H, W=W, cin=cin, cout=cout, k=k, pad=pad, bias=bias, layers=count, wgrad_ranges=ranges,
                         us={leg: {"native": v[0], "torch": v[1]} for leg, v in med.items()}, max_rel_dev=dev))
        if args.arith:
            s3 = sum(med3.values())
            flop = 2.0 * N * H * W * cin * cout * k * k
            tf = lambda us: flop / (us * 1e-6) / 1e12  # noqa: E731
            rows[-1].update(wgrad_ranges_bf16x3=ranges3, max_rel_dev_bf16x3=dev3)
            for leg in med:
                rows[-1]["us"][leg]["bf16x3"] = med3[leg]
            rows[-1]["tf_equivalent"] = {leg: {"f32": tf(med[leg][0]), "bf16x3": tf(med3[leg])} for leg in med}
            lines.append(f"| {name} | {count} | {ranges}, {ranges3} | " +
                         " | ".join(f"{med[leg][0]:.1f} / {med3[leg]:.1f} / {med[leg][1]:.1f}" for leg in ("fwd", "dx", "dw")) +
                         f" | {sn:.1f} / {s3:.1f} / {st:.1f} | {s3 / sn:.2f} | {s3 / st:.2f} | " +
                         ", ".join(f"{tf(med[leg][0]):.0f}" for leg in ("fwd", "dx", "dw")) + " | " +
                         ", ".join(f"{tf(med3[leg]):.0f}" for leg in ("fwd", "dx", "dw")) + " |")
        else:
            lines.append(f"| {name} | {count} | {ranges} | " + " | ".join(f"{med[leg][0]:.1f} / {med[leg][1]:.1f}" for leg in ("fwd", "dx", "dw")) +
                         f" | {sn:.1f} / {st:.1f} | {sn / st:.2f} |")
        print(lines[-1], flush=True)
    tot_n = sum(r["layers"] * sum(v["native"] for v in r["us"].values()) for r in rows)
    tot_t = sum(r["layers"] * sum(v["torch"] for v in r["us"].values()) for r in rows)
    lines.append(f"\nAll listed layers, forward + dX + dW + db, weighted by the number of layers: native {tot_n / 1000:.2f} ms, torch {tot_t / 1000:.2f} ms.")
    if args.arith:
        tot_3 = sum(r["layers"] * sum(v["bf16x3"] for v in r["us"].values()) for r in rows)
        lines.append(f"The same with arith = bf16x3: {tot_3 / 1000:.2f} ms.  Largest deviation of that arm from torch, relative to the largest value: " +
                     ", ".join(f"{leg} {max(r['max_rel_dev_bf16x3'][leg] for r in rows):.1e}" for leg in ("fwd", "dx", "dw")) + ".")
    lines.append(f"Largest deviation between the arms, relative to the largest value: " +
                 ", ".join(f"{leg} {max(r['max_rel_dev'][leg] for r in rows):.1e}" for leg in ("fwd", "dx", "dw")) + ".")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
        with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"bench": "conv", "native_ms": tot_n / 1000, "torch_ms": tot_t / 1000, "shapes": len(rows)}))


if __name__ == "__main__":
    main()
