#!/usr/bin/env python
"""Refining noisy keypoints against the photometric loss through install(net) (profiles/keypoint_grad.md).

A synthetic scene (3 views of 512 x 512, random maps in place of the encoders, random hot-path weights).  The targets are the train
branch's own outputs at the TRUE keypoints for a few recorded draws (patch position, sample jitter, view dropout - the seeds are
replayed), so that the loss at the true keypoints is exactly 0.  The keypoints are then displaced by a known random offset and
refined with torch.optim.Adam([kpt3d]) alone - 50 training steps of 1024 rays cycling through those draws, the model's parameters
frozen - against the reference's L1 terms.  Printed per step: the loss and the RMS distance of the keypoints to the true ones.

    python scripts/refine_keypoints_demo.py [--steps 50] [--offset 0.02] [--lr 2e-3]

Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dropin_train import Carrier  # noqa: E402
from keypointnerf_amd.dropin import install  # noqa: E402
from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict, to_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--offset", type=float, default=0.02, help="standard deviation of the displacement per coordinate (scene units)")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--patches", type=int, default=5, help="recorded draws (patch, samples, view dropout) the steps cycle through")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_keypoints_demo.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = a.res
    s = to_device(make_scene(n_views=3, src_hw=(512, 512), tar_hw=(res, res), mask="ellipsoid", seed=1, tar_focal_at_512=800.0), dev)
    net = install(Carrier(random_hotpath_state_dict(seed=3), s).to(dev))
    for p in net.parameters():
        p.requires_grad_(False)
    true_kpt = s["sp_data"]["kpt3d"].clone()
    common = dict(net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=1, stride=0, tar_img=None, bg_img=None,
                  feat_geo=s["feat_geo"], feat_tex=s["feat_tex"], camcenter=None, objcenter=None,
                  src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"], fine=True, uniform=False, blur=3, sample_per_ray_c=64,
                  sample_per_ray_f=64, rand_noise_std=0.0)
    yy, xx = torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")
    msk = (((yy - res // 2) ** 2 + (xx - res // 2) ** 2) < (res // 5) ** 2)[None, None].to(dev)
    net.train()
    net.train_out_h = net.train_out_w = 32

    def render(kpt, seed):
        """the train branch on the patch, the samples and the view dropout that `seed` draws"""
        np.random.seed(seed)
        torch.manual_seed(seed)
        return net.batch_render_pifu_nerf(sp_data=dict(s["sp_data"], kpt3d=kpt), msk=msk, **common)

    with torch.no_grad():                                               # the targets: the same draws at the true keypoints
        targets = [{k: v.detach().clone() for k, v in render(true_kpt, seed).items() if k in ("tex_fg", "tex_fg_fine")}
                   for seed in range(a.patches)]
    g = torch.Generator().manual_seed(7)
    kpt = (true_kpt + a.offset * torch.randn(true_kpt.shape, generator=g).to(dev)).requires_grad_(True)
    opt = torch.optim.Adam([kpt], lr=a.lr)
    curve = []
    rms = lambda: float((kpt.detach() - true_kpt).pow(2).sum(-1).mean().sqrt())
    print(f"step   loss        RMS distance to the true keypoints (start {rms():.5f})")
    for it in range(a.steps):
        opt.zero_grad(set_to_none=True)
        out, tar = render(kpt, it % a.patches), targets[it % a.patches]
        # the reference's L1 terms with the shipped lambdas (configs/zju.json:109-119)
        loss = (out["tex_fg"] - tar["tex_fg"]).abs().mean() + 10.0 * (out["tex_fg_fine"] - tar["tex_fg_fine"]).abs().mean()
        loss.backward()
        opt.step()
        curve.append((it, round(float(loss.detach()), 6), round(rms(), 6)))
        print(f"{it:4d}   {curve[-1][1]:.6f}    {curve[-1][2]:.6f}", flush=True)
    print(json.dumps({"demo": "refine_keypoints", "offset": a.offset, "lr": a.lr, "curve": curve}))


if __name__ == "__main__":
    main()
