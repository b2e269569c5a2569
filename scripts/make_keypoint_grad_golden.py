"""Reference fixture of the keypoint gradient: tests/golden/case_kpgrad.npz.

    python scripts/make_keypoint_grad_golden.py          (where the reference source tree is; see oracle/ref_shim.py)

The UNMODIFIED reference class (built as scripts/make_keypoint_set_golden.py builds it, at 24 / 3, 13 / 3 and 17 / 2) runs the
train branch on an 8 x 8 patch, 16 + 16 samples, V = 3, with sp_data["kpt3d"].requires_grad_(); loss = sum_k <out_k, G_k>;
loss.backward() fills kpt3d.grad through SpatialEncoder.forward (src/spatial.py:76-118).  Every random draw is recorded.

Stored per case: the generator arguments and SHA-256 digests of the regenerated inputs (tests/keypoint_set_cases.py), the draws,
the upstream G, the (n, 3) gradient, and the reference's own error on it.

Seed rule (as the keypoint-set fixtures): a seed of the draws is usable only if the reference's own float32 gradient is within
OWN_ERROR_MAX = 0.25 of the bar (1e-4 of the largest float64 entry) of its float64 repeat on the recorded draws, and both passes
keep at least two views.  The first seed from 20 on that qualifies is taken; every seed tried is printed with its own-error.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_keypoint_set_golden as ks  # noqa: E402
from tests.keypoint_set_cases import digests, recorded_draws, regenerate, train_patch_mask  # noqa: E402

CASES = [(24, 3), (13, 3), (17, 2)]
ks.WEIGHT_SEED.setdefault(24, 30)
SEEDS = range(20, 40)
BAR = 1e-4
DRAW_KEYS = ("train.seed", "train.pix", "train.u_c", "train.noise_c", "train.u_f", "train.noise_f", "train.keep_c", "train.keep_f",
             "train.noise_std")


def step32(net, scene, seed):
    """ks.train_part with kpt3d a leaf that requires a gradient -> (record of the draws and G, kpt3d.grad (n, 3) float32)"""
    kpt = scene["sp_data"]["kpt3d"].clone().requires_grad_(True)
    s = dict(scene, sp_data=dict(scene["sp_data"], kpt3d=kpt))
    d, _, keep_c, keep_f, alpha = ks.train_part(net, s, seed)
    assert kpt.grad is not None
    return d, kpt.grad.detach().reshape(-1, 3).clone(), keep_c, keep_f, alpha


def step64(n, lv, sd, scene, d):
    """ks.own_error's float64 repeat on the recorded draws -> kpt3d.grad (n, 3) float64"""
    f64 = torch.float64
    net = ks.reference_net(n, lv, sd).to(f64)

    def cast(o):
        if isinstance(o, torch.Tensor):
            return o.to(f64) if o.is_floating_point() else o
        if isinstance(o, dict):
            return {k: cast(v) for k, v in o.items()}
        return type(o)(cast(v) for v in o) if isinstance(o, (list, tuple)) else o

    s = cast(scene)
    kpt = s["sp_data"]["kpt3d"].clone().requires_grad_(True)
    queue = recorded_draws(d, dtype=f64)
    replay = lambda *a, **k: queue.pop(0)
    net.train()
    net.train_out_h = net.train_out_w = ks.TILE
    np.random.seed(int(d["train.seed"]))
    with ks._replaced([(torch, fn, replay) for fn in ("rand", "rand_like", "randn", "randn_like")] +
                      [(torch.Tensor, "float", lambda self, *a, **k: self.to(f64))]), ks._default_dtype(f64):
        out = net.batch_render_pifu_nerf(net, s["img"], s["cam"], 3, s["cam_tar"], 5, 0, None, s["feat_geo"], s["feat_tex"],
                                         dict(s["sp_data"], kpt3d=kpt), None, fine=True, uniform=False, sample_per_ray_c=ks.SC,
                                         sample_per_ray_f=ks.SF, rand_noise_std=float(d["train.noise_std"]),
                                         src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"],
                                         msk=train_patch_mask(s["cam_tar"]["height"], s["cam_tar"]["width"]))
    assert not queue
    sum((out[k] * torch.from_numpy(d["train.G." + k]).to(f64)).sum() for k in ks.OUT_KEYS).backward()
    return kpt.grad.detach().reshape(-1, 3).clone()


def main():
    out = {}
    for n, lv in CASES:
        tag = f"kp{n}_l{lv}"
        args = ks.generator_args(n, lv)
        sd, scene_r, scene_t = regenerate(args)
        net = ks.reference_net(n, lv, sd)
        tried, chosen = [], None
        for seed in SEEDS:
            d, g32, keep_c, keep_f, alpha = step32(net, scene_t, seed)
            if sum(keep_c) < 2 or sum(keep_f) < 2:
                print(f"{tag} seed {seed}: keep_c {keep_c} keep_f {keep_f}: a pass keeps fewer than two views")
                continue
            g64 = step64(n, lv, sd, scene_t, d)
            own = float((g32.double() - g64).abs().max()) / (BAR * float(g64.abs().max()))
            tried.append((seed, own))
            print(f"{tag} seed {seed}: the reference's own float32 error = {own:.3f} of the bar (max |grad64| = {float(g64.abs().max()):.4e}), "
                  f"alpha_fine mean {alpha:.3f}")
            if own <= ks.OWN_ERROR_MAX:
                chosen = (seed, own, d, g32, g64)
                break
        bar_factor = 1.0
        if chosen is None:
            # no seed qualifies: four times the reference's smallest own-error, on the seed that gave it
            seed, own = min(tried, key=lambda t: t[1])
            d, g32, _, _, _ = step32(net, scene_t, seed)
            chosen = (seed, own, d, g32, step64(n, lv, sd, scene_t, d))
            bar_factor = 4.0 * own
            print(f"{tag}: no seed in {SEEDS.start}..{SEEDS.stop - 1} is within {ks.OWN_ERROR_MAX} of the bar; seed {seed}, bar x {bar_factor:.3f}")
        seed, own, d, g32, g64 = chosen
        out[tag + ".generator_json"] = np.array(json.dumps(args))
        out[tag + ".digests_json"] = np.array(json.dumps(digests(sd, scene_r, scene_t)))
        for k in DRAW_KEYS:
            out[f"{tag}.{k}"] = d[k]
        for k in ks.OUT_KEYS:
            out[f"{tag}.train.G.{k}"] = d["train.G." + k]
        out[tag + ".kpt_grad"] = g32.numpy()
        out[tag + ".kpt_grad64"] = g64.numpy()
        out[tag + ".own_error"] = np.float64(own)
        out[tag + ".bar_factor"] = np.float64(bar_factor)
        out[tag + ".seeds_tried_json"] = np.array(json.dumps(tried))
    path = os.path.join(ks.GOLDEN_DIR, "case_kpgrad.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
