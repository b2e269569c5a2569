#!/usr/bin/env python
"""What the keypoint gradient costs (profiles/keypoint_grad.md).

  step      the drop-in training step of scripts/bench_dropin_train.py (install(net) + torch.optim.Adam, 3 views of 512 x 512,
            64 + 64 samples) at 1024 and 4096 rays, with sp_data["kpt3d"].requires_grad off and on, the arms alternating in one
            process.  The "off" arm is the default step: run this script on two commits in alternating processes to see that it
            did not move.
  backward  ops.render_rays_train_backward on the kept state of one forward, want_kpt off and on, alternating: the difference is
            k_kpt_grad_pack + k_kpt_grad + k_kpt_grad_finish of both passes; the (point, view) rows come from the backward's
            profile hooks (kpn_bwd_profile_collect), which also give the time of the backward's own kernel groups.

    python scripts/bench_keypoint_grad.py [--what step backward] [--rays 1024 4096] [--steps 20] [--runs 3]

Prints a line per arm and one JSON line.  Needs a GPU."""
import argparse
import ctypes
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
from keypointnerf_amd import lib as kl, ops  # noqa: E402
from keypointnerf_amd.dropin import install  # noqa: E402
from keypointnerf_amd.losses import compute_error  # noqa: E402
from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict, to_device  # noqa: E402

SCENE = dict(n_views=3, src_hw=(512, 512), tar_hw=(512, 512), mask="ellipsoid", seed=1, tar_focal_at_512=800.0)


def make_step(dev, patch, with_kpt):
    s = to_device(make_scene(**SCENE), dev)
    net = install(Carrier(random_hotpath_state_dict(seed=3), s).to(dev))
    net.train()
    net.train_out_h = net.train_out_w = patch
    yy, xx = torch.meshgrid(torch.arange(512), torch.arange(512), indexing="ij")
    msk = (((yy - 256) ** 2 + (xx - 256) ** 2) < 60 ** 2)[None, None].to(dev)
    feat_geo = [f.clone().requires_grad_(True) for f in s["feat_geo"]]
    feat_tex = s["feat_tex"].clone().requires_grad_(True)
    kpt = s["sp_data"]["kpt3d"].clone().requires_grad_(with_kpt)
    opt = torch.optim.Adam(list(net.parameters()) + ([kpt] if with_kpt else []), lr=1e-5)
    tar = torch.rand(1, 3, 512, 512, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        out = net.batch_render_pifu_nerf(net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=5, stride=0,
                                         tar_img=tar, bg_img=None, feat_geo=feat_geo, feat_tex=feat_tex, sp_data=dict(s["sp_data"], kpt3d=kpt),
                                         camcenter=None, objcenter=None, msk=msk, src_foreground_mask=s["src_foreground_mask"],
                                         bounds=s["bounds"], fine=True, uniform=False, blur=3, sample_per_ray_c=64,
                                         sample_per_ray_f=64, rand_noise_std=0.01)
        out["tex_cal"], out["tex_cal_fine"] = out["tex_fg"], out["tex_fg_fine"]
        loss, _ = compute_error(out_nerf=out, vggloss=None, lambdas={"lambda_l1_c": 1.0, "lambda_l1": 10.0, "lambda_vgg": 0.5})
        loss.backward()
        assert (kpt.grad is not None) == with_kpt
        opt.step()
        return float(loss.detach())
    return step


def time_steps(dev, a, rays):
    patch = int(round(rays ** 0.5))
    arms = {"off": make_step(dev, patch, False), "on": make_step(dev, patch, True)}
    ms = {m: [] for m in arms}
    for run in range(a.runs):
        for m, fn in arms.items():                                     # alternating
            np.random.seed(run)
            torch.manual_seed(run)
            for _ in range(a.warmup if run == 0 else 1):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = fn()
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) / a.steps * 1e3)
            assert np.isfinite(loss)
    for m in arms:
        print(f"step, {rays} rays, kpt3d.requires_grad {m}: {min(ms[m]):.3f} - {max(ms[m]):.3f} ms/step over {a.runs} runs of {a.steps} steps",
              flush=True)
    return {m: [round(x, 4) for x in v] for m, v in ms.items()}


def time_backward(dev, a, rays):
    L = kl.get_library()
    s = to_device(make_scene(**SCENE), dev)
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    w = ops.PackedWeights(random_hotpath_state_dict(seed=3), device=dev)
    patch = int(round(rays ** 0.5))
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(patch), torch.arange(patch), indexing="ij")
    pix = (torch.stack([xx, yy], -1).reshape(-1, 2) + (256 - patch // 2)).to(torch.int32).to(dev)
    R = pix.shape[0]
    args = (ps, w, s["cam_tar"], s["bounds"], pix, torch.rand(R, 64, generator=g).to(dev), torch.rand(R, 64, generator=g).to(dev), 0b111, 0b111)
    kw = dict(noise_coarse=torch.randn(R * 64, generator=g).to(dev), noise_fine=torch.randn(R * 128, generator=g).to(dev), rand_noise_std=0.01,
              n_coarse=64, n_fine=64)
    out, state = ops.render_rays_train(*args, keep_state=True, **kw)
    grads = {k: torch.randn(v.shape, generator=g).to(dev) for k, v in out.items()}
    ms = {"off": [], "on": []}
    for rep in range(a.reps + 2):
        for m in ms:                                                   # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.render_rays_train_backward(*args, grads, state=state, want_kpt=(m == "on"), **kw)
            e1.record()
            e1.synchronize()
            if rep >= 2:
                ms[m].append(e0.elapsed_time(e1))
    # rows and the backward's own kernel groups, from one profiled call
    L.check(L.kpn_bwd_profile_enable(1))
    ops.render_rays_train_backward(*args, grads, state=state, **kw)
    ms5, n5 = (ctypes.c_double * 5)(), (ctypes.c_int64 * 5)()
    rows, kept, points = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    L.check(L.kpn_bwd_profile_collect(ms5, n5, ctypes.byref(rows), ctypes.byref(kept), ctypes.byref(points)))
    L.check(L.kpn_bwd_profile_enable(0))
    off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
    groups = dict(zip(("rows_fwd", "color_bwd", "fuse_bwd", "rows_bwd", "wgrad"), [round(x, 4) for x in ms5]))
    print(f"backward, {rays} rays: want_kpt off {off:.3f} ms (min {min(ms['off']):.3f} .. max {max(ms['off']):.3f}), on {on:.3f} ms "
          f"(min {min(ms['on']):.3f} .. max {max(ms['on']):.3f}) over {a.reps} calls; {kept.value} kept (point, view) rows; "
          f"difference {on - off:.3f} ms = {(on - off) * 1e6 / max(kept.value, 1):.2f} ns per row = {100 * (on - off) / on:.1f} % of the backward; "
          f"kernel groups of the plain backward {groups}", flush=True)
    return {"off_ms": [round(x, 4) for x in ms["off"]], "on_ms": [round(x, 4) for x in ms["on"]], "kept_rows": kept.value, "groups_ms": groups}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["step", "backward"], choices=["step", "backward"])
    ap.add_argument("--rays", nargs="+", type=int, default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_keypoint_grad.py needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    result = {"bench": "keypoint_grad"}
    for rays in a.rays:
        if "step" in a.what:
            result[f"step_ms_{rays}"] = time_steps(dev, a, rays)
        if "backward" in a.what:
            result[f"backward_{rays}"] = time_backward(dev, a, rays)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
