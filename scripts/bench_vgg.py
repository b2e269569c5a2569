#!/usr/bin/env python
"""The perceptual term of the training loss (VGGLoss, reference src/utils.py:750-805), native (kpn_vgg_loss) against the
same-weight module through MIOpen, in one process, both warmed up, timed with device events: two forwards (rendered and
target patch) + the gradient to the rendered patch, as training_step does.  Then the drop-in training step of
scripts/bench_dropin_train.py (render + compute_error + backward + Adam) at 1024 and 4096 rays with each VGG path.

    python scripts/bench_vgg.py [--skip-train]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keypointnerf_amd.vgg import NativeVGGLoss  # noqa: E402
from tests.vgg_golden import StandInVGGLoss  # noqa: E402


def timed(fn, iters=50, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def term(vggloss, x, y):
    def step():
        (g,) = torch.autograd.grad(0.5 * vggloss(x, y), x)
        return g
    return step


def train_step_ms(size, vgg):
    from keypointnerf_amd.dropin import install
    from keypointnerf_amd.losses import compute_error
    from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict, to_device
    from scripts.bench_dropin_train import Carrier
    dev = torch.device("cuda", 0)
    s = to_device(make_scene(n_views=3, src_hw=(512, 512), tar_hw=(512, 512), mask="ellipsoid", seed=1, tar_focal_at_512=800.0), dev)
    net = install(Carrier(random_hotpath_state_dict(seed=3), s).to(dev))
    net.train()
    net.train_out_h = net.train_out_w = size
    yy, xx = torch.meshgrid(torch.arange(512), torch.arange(512), indexing="ij")
    msk = (((yy - 256) ** 2 + (xx - 256) ** 2) < 60 ** 2)[None, None].to(dev)
    feat_geo = [f.clone().requires_grad_(True) for f in s["feat_geo"]]
    feat_tex = s["feat_tex"].clone().requires_grad_(True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-5)
    tar = torch.rand(1, 3, 512, 512, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        out = net.batch_render_pifu_nerf(net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=5, stride=0,
                                         tar_img=tar, bg_img=None, feat_geo=feat_geo, feat_tex=feat_tex, sp_data=dict(s["sp_data"]),
                                         camcenter=None, objcenter=None, msk=msk, src_foreground_mask=s["src_foreground_mask"],
                                         bounds=s["bounds"], fine=True, uniform=False, blur=3, sample_per_ray_c=64,
                                         sample_per_ray_f=64, rand_noise_std=0.01)
        out["tex_cal"], out["tex_cal_fine"] = out["tex_fg"], out["tex_fg_fine"]
        loss, _ = compute_error(out_nerf=out, vggloss=vgg, lambdas={"lambda_l1_c": 1.0, "lambda_l1": 10.0, "lambda_vgg": 0.5})
        loss.backward()
        opt.step()

    np.random.seed(0)
    torch.manual_seed(0)
    return timed(step, iters=10, warm=3)


def main():
    dev = torch.device("cuda", 0)
    m = StandInVGGLoss().to(dev)
    nat = NativeVGGLoss(m)
    print("| patch | native (ms) | MIOpen (ms) | speed-up |")
    print("|---|---|---|---|")
    for size in (32, 64):
        torch.manual_seed(0)
        x = torch.rand(1, 3, size, size, device=dev, requires_grad=True)
        y = torch.rand(1, 3, size, size, device=dev)
        t_nat, t_ref = timed(term(nat, x, y)), timed(term(m, x, y))
        print(f"| {size}x{size} | {t_nat:.3f} | {t_ref:.3f} | {t_ref / t_nat:.2f}x |", flush=True)
    if "--skip-train" in sys.argv:
        return
    print("| rays | step, no VGG (ms) | step, native VGG (ms) | step, MIOpen VGG (ms) |")
    print("|---|---|---|---|")
    for size in (32, 64):
        t0, t1, t2 = train_step_ms(size, None), train_step_ms(size, nat), train_step_ms(size, m)
        print(f"| {size * size} | {t0:.2f} | {t1:.2f} | {t2:.2f} |", flush=True)


if __name__ == "__main__":
    main()
