"""Times training (forward + backward to every parameter gradient) and the forward alone through a whole HGFilterV2 three ways - the
untouched module, the single-operator blocks (encoders.install_native_geo(fused_blocks=True)) and the single-operator network
(``fused=True``, torch.ops.kpnerf.hg_filter) - and records the peak memory of one training step per arm.

    python scripts/bench_geo_fused.py [--views 3] [--size 512] [--reps 20] [--root CHECKOUT] [--label NAME] [--out FILE.md]

net:    tests/encoder_golden.HGFilterV2 on views x 3 x (size / 2)^2 input (the geometry encoder at ds = 1), train mode.
memory: torch.cuda.max_memory_allocated over one forward + backward per arm, above what was allocated before the step (parameters, input
        and seed gradients).

The arms alternate within every repetition: a repetition times one step of one arm between two device events, then the next arm; the
figures are the median and the range over the repetitions, after three warm-up rounds.  ``--root`` imports keypointnerf_amd and tests from
another checkout of the project (one built there), e.g. the parent commit for a baseline; a checkout without the single-operator network is
measured without that arm.  Each call is one fresh process.  Needs a GPU.
"""
import argparse
import copy
import inspect
import json
import os
import statistics
import sys

import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)                    # ms


def alternate(arms, reps, warm=3):
    """arms: [(name, fn)] -> {name: dict(median, min, max)} in ms"""
    for _ in range(warm):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in arms}
    for _ in range(reps):
        for n, fn in arms:
            ts[n].append(timed(fn))
    return {n: dict(median=statistics.median(t), min=min(t), max=max(t)) for n, t in ts.items()}


def cell(r):
    return f"{r['median']:.2f} ({r['min']:.2f} .. {r['max']:.2f})"


def step_of(net, x, gs):
    params = [p for p in net.parameters()]
    return lambda: torch.autograd.grad(net(x), params, gs, allow_unused=True)


def forward_of(net, x):
    def run():
        with torch.no_grad():
            return net(x)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geo_fused.py needs a GPU: a time measured anywhere else says nothing")
    sys.path.insert(0, os.path.abspath(args.root))
    from keypointnerf_amd import encoders
    from tests import encoder_golden as eg
    has_fused = "fused" in inspect.signature(encoders.install_native_geo).parameters
    label = args.label or os.path.abspath(args.root)
    hw = args.size >> 1
    plain = eg.stand_in_geo(1).train().cuda()
    nets = [("untouched module", plain), ("install_native_geo(fused_blocks=True)", copy.deepcopy(plain))]
    report = encoders.install_native_geo(nets[1][1], fused_blocks=True)
    assert not any(left for _, left in report.values()), report
    if has_fused:
        nets.append(("install_native_geo(fused=True)", copy.deepcopy(plain)))
        assert encoders.install_native_geo(nets[2][1], fused=True)["fused"] == ([""], {})
    x = eg.net_input(eg.case_image((args.views, 3, args.size, args.size), 1).cuda(), 1).contiguous()
    gen = torch.Generator(device="cuda").manual_seed(0)
    cl = torch.channels_last
    gs = [torch.randn(args.views, 64, hw // 4, hw // 4, device="cuda", generator=gen).contiguous(memory_format=cl),
          torch.randn(args.views, 8, hw, hw, device="cuda", generator=gen).contiguous(memory_format=cl)]
    steps = [(n, step_of(net, x, gs)) for n, net in nets]
    step_ms = alternate(steps, args.reps)
    forward_ms = alternate([(n, forward_of(net, x)) for n, net in nets], args.reps)
    memory = {}
    for n, fn in steps:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        memory[n] = dict(peak_above_base_mib=(torch.cuda.max_memory_allocated() - base) / 2**20, base_mib=base / 2**20)
        del out
    names = [n for n, _ in nets]
    lines = [f"Checkout: {label} ({'with' if has_fused else 'without'} the single-operator network); HGFilterV2, {args.views} x 3 x {hw}^2 input; "
             f"median (min .. max) over {args.reps} repetitions", "",
             "| | " + " | ".join(names) + " |", "|---|" + "---|" * len(names),
             "| forward + backward (ms) | " + " | ".join(cell(step_ms[n]) for n in names) + " |",
             "| forward alone, no_grad (ms) | " + " | ".join(cell(forward_ms[n]) for n in names) + " |",
             "| peak memory of one step above parameters and inputs (MiB) | " + " | ".join(f"{memory[n]['peak_above_base_mib']:.1f}" for n in names) + " |"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"bench": "geo_fused", "label": label, "step_ms": step_ms, "forward_ms": forward_ms, "memory": memory}))


if __name__ == "__main__":
    main()
