"""Times the two image encoders on one 3 x 512^2 source set (network input 256^2, ds = 1): the plain-PyTorch modules of
tests/encoder_golden.py on PyTorch / MIOpen in NCHW and channels-last, and the native encoders (keypointnerf_amd/encoders.py).
Device events, warm-up, median and min .. max of the repeats, one JSON line.

    python scripts/bench_encoders.py [--reps 30]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keypointnerf_amd import encoders  # noqa: E402
from tests import encoder_golden as eg  # noqa: E402


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--native-only", action="store_true", help="skip the PyTorch paths (for a kernel trace of the native encoders)")
    args = ap.parse_args()
    img = eg.case_image((3, 3, 512, 512), 1).cuda()
    res = {}
    with torch.no_grad():
        for tag, net in (("geo", eg.stand_in_geo(1).cuda()), ("tex", eg.stand_in_tex(2).cuda())):
            if not args.native_only:
                res[f"{tag}_torch_nchw"] = timed(lambda: net(eg.net_input(img, 1)), args.reps)
                cl = net.to(memory_format=torch.channels_last)
                res[f"{tag}_torch_channels_last"] = timed(lambda: cl(eg.net_input(img, 1).contiguous(memory_format=torch.channels_last)), args.reps)
            nat = (encoders.NativeGeoEncoder if tag == "geo" else encoders.NativeTexEncoder)(net)
            res[f"{tag}_native"] = timed(lambda: nat(img, ds=1), args.reps)
    print(json.dumps({"bench": "encoders_3x512", **res}))


if __name__ == "__main__":
    main()
