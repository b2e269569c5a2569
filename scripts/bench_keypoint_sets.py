#!/usr/bin/env python
"""What a model with another skeleton costs (profiles/keypoint_sets.md).  Two measurements, each alternating its arms in one process:

  frame   the headline frame of bench.py (configs[1]: 512 x 512 target, 3 source views of 512 x 512, 64 + 64 samples, ellipsoid
          masks, target focal 800) rendered by the shipped 24-keypoint / 3-octave model and by a 13-keypoint / 3-octave model on
          the same scene with its keypoints cut to 13.  The kernels run the 13 / 3 model as the 24 / 3 model with zero weights
          on the padded encoding values, so the arithmetic per row is the same; the two models have different random weights,
          hence different densities (the share of samples whose colour is evaluated differs).
  step    the drop-in training step of scripts/bench_param_step.py at --rays rays for the 13 / 3 model: install(net) +
          torch.optim.Adam against install(net, native_params=True) + keypointnerf_amd.optim.Adam.

    python scripts/bench_keypoint_sets.py [--what frame step] [--reps 12] [--steps 20] [--runs 3] [--rays 1024]
    python scripts/bench_keypoint_sets.py --what step --only native --steps K --runs 1     (behind a kernel trace: launches per step
                                                                                          = the difference of two K, divided)
Prints a line per arm and one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dropin_train import Carrier  # noqa: E402
from keypointnerf_amd import ops, optim  # noqa: E402
from keypointnerf_amd.dropin import install  # noqa: E402
from keypointnerf_amd.losses import compute_error  # noqa: E402
from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict, to_device  # noqa: E402

SCENE = dict(n_views=3, src_hw=(512, 512), tar_hw=(512, 512), mask="ellipsoid", seed=1, tar_focal_at_512=800.0)


def frame_arm(dev, n, lv, res=512, samples=64):
    s = to_device(make_scene(n_kpt=n, **SCENE), dev)
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    w = ops.PackedWeights(random_hotpath_state_dict(seed=3, n_kpt=n, sp_level=lv), device=dev, shape=(n, lv))
    plan = ops.RenderPlan(ps, (0, 0, 1, res, res), samples, samples, fine=True)

    def frame():
        return ops.render_rays(ps, w, s["cam_tar"], s["bounds"], plan=plan)
    return frame


def time_frames(dev, reps, warm=2):
    arms = [("24 keypoints / 3 octaves", frame_arm(dev, 24, 3)), ("13 keypoints / 3 octaves", frame_arm(dev, 13, 3))]
    for _ in range(warm):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in arms}
    for _ in range(reps):
        for k, fn in arms:                                             # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
            assert bool(torch.isfinite(out["tex_fg_fine"]).all())
    for k in ms:
        print(f"frame, {k}: median {statistics.median(ms[k]):.3f} ms (min {min(ms[k]):.3f} .. max {max(ms[k]):.3f}) over {reps} frames", flush=True)
    return {k: [round(x, 4) for x in v] for k, v in ms.items()}


def make_step(dev, mode, patch, n, lv):
    s = to_device(make_scene(n_kpt=n, **SCENE), dev)
    net = Carrier(random_hotpath_state_dict(seed=3, n_kpt=n, sp_level=lv), s).to(dev)
    net.sp_encoder.n_kpt, net.sp_encoder.sp_level = n, lv
    native = mode == "native"
    install(net, native_params=True) if native else install(net)
    net.train()
    net.train_out_h = net.train_out_w = patch
    yy, xx = torch.meshgrid(torch.arange(512), torch.arange(512), indexing="ij")
    msk = (((yy - 256) ** 2 + (xx - 256) ** 2) < 60 ** 2)[None, None].to(dev)
    feat_geo = [f.clone().requires_grad_(True) for f in s["feat_geo"]]
    feat_tex = s["feat_tex"].clone().requires_grad_(True)
    opt = optim.Adam(net.parameters(), net=net, lr=1e-5) if native else torch.optim.Adam(net.parameters(), lr=1e-5)
    tar = torch.rand(1, 3, 512, 512, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        out = net.batch_render_pifu_nerf(net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=5, stride=0,
                                         tar_img=tar, bg_img=None, feat_geo=feat_geo, feat_tex=feat_tex, sp_data=dict(s["sp_data"]),
                                         camcenter=None, objcenter=None, msk=msk, src_foreground_mask=s["src_foreground_mask"],
                                         bounds=s["bounds"], fine=True, uniform=False, blur=3, sample_per_ray_c=64,
                                         sample_per_ray_f=64, rand_noise_std=0.01)
        out["tex_cal"], out["tex_cal_fine"] = out["tex_fg"], out["tex_fg_fine"]
        loss, _ = compute_error(out_nerf=out, vggloss=None, lambdas={"lambda_l1_c": 1.0, "lambda_l1": 10.0, "lambda_vgg": 0.5})
        loss.backward()
        opt.step()
        return float(loss.detach())
    return step


def time_steps(dev, a):
    modes = [a.only] if a.only else ["default", "native"]
    patch = int(round(a.rays ** 0.5))
    steps = {m: make_step(dev, m, patch, 13, 3) for m in modes}
    ms = {m: [] for m in modes}
    for run in range(a.runs):
        for m in modes:                                                # alternating
            np.random.seed(run)
            torch.manual_seed(run)
            for _ in range(a.warmup if run == 0 else 1):
                steps[m]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = steps[m]()
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / a.steps * 1e3)
            assert np.isfinite(loss)
    for m in modes:
        print(f"step, 13 keypoints / 3 octaves, {a.rays} rays, {m}: {min(ms[m]):.3f} - {max(ms[m]):.3f} ms/step over {a.runs} runs of "
              f"{a.steps} steps", flush=True)
    return {m: [round(x, 4) for x in v] for m, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["frame", "step"], choices=["frame", "step"])
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["default", "native"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keypoint_sets.py needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"bench": "keypoint_sets"}
    if "frame" in a.what:
        result["frame_ms"] = time_frames(dev, a.reps)
    if "step" in a.what:
        result["step_ms"] = time_steps(dev, a)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
