#!/usr/bin/env python
"""Writes tests/golden/case_v_vgg_loss.npz from the LIVE, unmodified reference VGGLoss / Vgg19 (src/utils.py:750-805).

Stubs only for what is missing here: torchvision.models.vgg19(pretrained=True).features becomes vgg19.features[0:21] with
seeded default init (tests/vgg_golden.py:features; the pretrained weights cannot be had offline), transforms.Normalize a
module that keeps mean / std and computes (v - mean) / std as torchvision does, .cuda() the identity on the CPU (oracle/ref_shim).
Recorded per case: the inputs, the reference's loss and d loss / d x from its own autograd in fp32 and with the module in
fp64, plus the weight seed and per-convolution checksums (the weights are rebuilt from the seed by the tests).

    python scripts/make_vgg_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from tests import vgg_golden as vg  # noqa: E402

SEED = 0
OUT = os.path.join(ROOT, "tests", "golden", "case_v_vgg_loss.npz")
CASES = {"c32": (1, 32, 32), "c64": (1, 64, 64), "c19x27": (2, 19, 27), "half32": (1, 32, 32)}


class Normalize(torch.nn.Module):
    """torchvision.transforms.Normalize: keeps mean / std, F.normalize's (tensor - mean) / std in the tensor's dtype"""

    def __init__(self, mean, std, inplace=False):
        super().__init__()
        self.mean, self.std = mean, std

    def forward(self, t):
        m = torch.as_tensor(self.mean, dtype=t.dtype, device=t.device).view(-1, 1, 1)
        s = torch.as_tensor(self.std, dtype=t.dtype, device=t.device).view(-1, 1, 1)
        return t.sub(m).div(s)


class _VGG19:
    def __init__(self, seed):
        self.features = vg.features(seed)


def load_reference_vggloss(seed=SEED):
    """-> the reference's VGGLoss class (loaded from its unmodified src/utils.py), with vgg19 seeded by `seed`"""
    ref_shim.load_reference()                     # stubs the missing modules (cv2, torchvision, ...) and .cuda()
    sys.modules["torchvision.models"].vgg19 = lambda pretrained=False, **k: _VGG19(seed)
    sys.modules["torchvision.transforms"].Normalize = Normalize
    spec = importlib.util.spec_from_file_location("kpn_reference_utils_vgg", os.path.join(ref_shim.REFERENCE_ROOT, "src", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                  # ref_shim swaps VGGLoss out of src.utils; this copy keeps the real one
    return mod.VGGLoss


def run(m, x, y, dtype):
    xs = torch.tensor(x, dtype=dtype, requires_grad=True)
    loss = m.to(dtype)(xs, torch.tensor(y, dtype=dtype))
    loss.backward()
    return float(loss.detach()), xs.grad.numpy().astype(np.float32 if dtype == torch.float32 else np.float64)


def main():
    VGGLoss = load_reference_vggloss()
    m = VGGLoss()
    feats = vg.features(SEED)
    rng = np.random.default_rng(2024)
    d = {"seed": np.int64(SEED), "checksums": vg.checksums(feats), "cases": np.array(list(CASES))}
    for name, (B, H, W) in CASES.items():
        x = rng.random((B, 3, H, W), dtype=np.float32)
        y = rng.random((B, 3, H, W), dtype=np.float32)
        if name == "half32":
            y[..., : W // 2] = x[..., : W // 2]   # y = x on the left half of the patch
        d[f"{name}_x"], d[f"{name}_y"] = x, y
        d[f"{name}_loss32"], d[f"{name}_dx32"] = run(m, x, y, torch.float32)
        d[f"{name}_loss64"], d[f"{name}_dx64"] = run(m, x, y, torch.float64)
        m.to(torch.float32)
        print(name, d[f"{name}_loss64"], abs(d[f"{name}_loss32"] - d[f"{name}_loss64"]) / d[f"{name}_loss64"])
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
