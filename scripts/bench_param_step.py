#!/usr/bin/env python
"""The drop-in training step of scripts/bench_dropin_train.py two ways, alternating in one process:

    default  install(net)                      + torch.optim.Adam            (the parent commit's step, code path untouched)
    native   install(net, native_params=True)  + keypointnerf_amd.optim.Adam (one-launch fold, fold backward and Adam)

at 1024 (32 x 32) and 4096 (64 x 64) rays, --runs runs of --steps steps each; prints min - max ms per step of each and one JSON
line.  `--only default|native --rays N --steps K --runs 1` is the form to put behind `rocprofv3 --kernel-trace --stats --` for
the launch count per step (count two step numbers and divide the difference)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dropin_train import Carrier  # noqa: E402
from keypointnerf_amd import optim  # noqa: E402
from keypointnerf_amd.dropin import install  # noqa: E402
from keypointnerf_amd.losses import compute_error  # noqa: E402
from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict, to_device  # noqa: E402


def make_step(s, dev, mode, patch):
    native = mode == "native"
    net = Carrier(random_hotpath_state_dict(seed=3), s).to(dev)
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
        return float(loss.detach())                                    # the loop of bench_dropin_train.py: one read-back per step
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["default", "native"])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = to_device(make_scene(n_views=3, src_hw=(512, 512), tar_hw=(512, 512), mask="ellipsoid", seed=1, tar_focal_at_512=800.0), dev)
    modes = [a.only] if a.only else ["default", "native"]
    result = {}
    for rays in a.rays:
        patch = int(round(rays ** 0.5))
        steps = {m: make_step(s, dev, m, patch) for m in modes}
        ms = {m: [] for m in modes}
        for run in range(a.runs):
            for m in modes:                                            # alternating
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
            print(f"{rays} rays, {m}: {min(ms[m]):.3f} - {max(ms[m]):.3f} ms/step over {a.runs} runs of {a.steps} steps", flush=True)
            result[f"{m}_{rays}"] = [round(x, 4) for x in ms[m]]
    print(json.dumps({"bench": "param_step", "ms_per_step": result}))


if __name__ == "__main__":
    main()
