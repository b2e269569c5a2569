"""Test infrastructure of the native image encoders: the project's own plain-PyTorch statement of the two networks, written
from their layer lists (reference src/utils.py:199-474), the seeded parameters of tests/golden/case_w_encoders.npz and the
emulator driver.

The golden records seeds and a checksum per parameter tensor, not the 113 MB of weights: ``seeded(module, seed)`` rebuilds them
(the reference's init — every convolution drawn from N(0, 0.02) after ``manual_seed(125)``, biases 0, src/model.py:610-640 —
then a seeded perturbation of EVERY parameter, biases and GroupNorm gamma / beta included) and ``check_checksums`` verifies
them.  scripts/make_encoder_golden.py asserts that these modules and the live reference classes agree bit for bit on the CPU
(parameters and outputs), so on a machine without the reference tree they stand in for it.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "case_w_encoders.npz")
GEO_ARGS = dict(n_stack=1, n_downsample=4, out_ch=64, hd=False)                                   # configs/zju.json:46-51
TEX_ARGS = dict(ngf=64, n_downsample=3, n_blocks=4, n_upsample=2, out_ch=8, norm="instance")       # configs/zju.json:82-89


class ConvBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.bn1, self.bn2 = nn.GroupNorm(min(32, cin), cin), nn.GroupNorm(min(32, cout // 2), cout // 2)
        self.bn3, self.bn4 = nn.GroupNorm(min(32, cout // 4), cout // 4), nn.GroupNorm(min(32, cin), cin)
        self.downsample = nn.Sequential(self.bn4, nn.ReLU(True), nn.Conv2d(cin, cout, 1, bias=False)) if cin != cout else None
        self.conv1 = nn.Conv2d(cin, cout // 2, 3, padding=1, bias=False)
        self.conv2 = nn.Conv2d(cout // 2, cout // 4, 3, padding=1, bias=False)
        self.conv3 = nn.Conv2d(cout // 4, cout // 4, 3, padding=1, bias=False)
        self.nl = nn.ReLU(inplace=True)

    def forward(self, x):
        o1 = self.conv1(self.nl(self.bn1(x)))
        o2 = self.conv2(self.nl(self.bn2(o1)))
        o3 = self.conv3(self.nl(self.bn3(o2)))
        out = torch.cat((o1, o2, o3), 1)
        out += x if self.downsample is None else self.downsample(x)
        return out


class HourGlass(nn.Module):
    def __init__(self, depth, features):
        super().__init__()
        self.depth, self.features = depth, features
        self._make(depth)

    def _make(self, level):
        self.add_module(f"b1_{level}", ConvBlock(self.features, self.features))
        self.add_module(f"b2_{level}", ConvBlock(self.features, self.features))
        if level > 1:
            self._make(level - 1)
        else:
            self.add_module(f"b2_plus_{level}", ConvBlock(self.features, self.features))
        self.add_module(f"b3_{level}", ConvBlock(self.features, self.features))

    def _run(self, level, x):
        up1 = self._modules[f"b1_{level}"](x)
        low = self._modules[f"b2_{level}"](F.avg_pool2d(x, 2, stride=2))
        low = self._run(level - 1, low) if level > 1 else self._modules[f"b2_plus_{level}"](low)
        low = self._modules[f"b3_{level}"](low)
        return up1 + F.interpolate(low, scale_factor=2, mode="bicubic", align_corners=True)

    def forward(self, x):
        return self._run(self.depth, x)


class DeconvReLUGroup(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False)
        self.nl = nn.ReLU(inplace=True)
        self.norm = nn.GroupNorm(min(32, cout), cout)

    def forward(self, x):
        return self.nl(self.norm(self.conv(x)))


class HGFilterV2(nn.Module):
    """n_stack = 1, norm = "group", hd = False"""

    def __init__(self, out_ch=64, out_ch_hd=8):
        super().__init__()
        self.n_stack, self.hd = 1, False
        self.nl = nn.ReLU(True)
        self.unpack1 = DeconvReLUGroup(128, 32)
        self.conv_out = nn.Conv2d(32, out_ch_hd, 5, padding=2)
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3)
        self.bn1 = nn.GroupNorm(32, 64)
        self.conv2, self.conv3, self.conv4 = ConvBlock(64, 128), ConvBlock(128, 128), ConvBlock(128, 256)
        self.m0 = HourGlass(4, 256)
        self.top_m_0 = ConvBlock(256, 256)
        self.conv_last0 = nn.Conv2d(256, 256, 1)
        self.bn_end0 = nn.GroupNorm(32, 256)
        self.l0 = nn.Conv2d(256, out_ch, 1)

    def forward(self, x):
        x = self.conv2(self.nl(self.bn1(self.conv1(x))))
        x_hd = self.conv_out(self.unpack1(x))
        x = self.conv4(self.conv3(F.avg_pool2d(x, 2, stride=2)))
        ll = self.top_m_0(self.m0(x))
        ll = F.relu(self.bn_end0(self.conv_last0(ll)), True)
        return [self.l0(ll), x_hd]


class ResBlk(nn.Module):
    def __init__(self, ch):
        super().__init__()
        norm = lambda: nn.InstanceNorm2d(ch, affine=False, track_running_stats=False)     # noqa: E731
        self.layers = nn.Sequential(nn.ReplicationPad2d(1), nn.Conv2d(ch, ch, 3), norm(), nn.ReLU(True),
                                    nn.ReplicationPad2d(1), nn.Conv2d(ch, ch, 3), norm())

    def forward(self, x):
        return x + self.layers(x)


class ResBlkEncoder(nn.Module):
    """norm = "instance" """

    def __init__(self, out_ch=8, ngf=64, n_downsample=3, n_blocks=4, n_upsample=2):
        super().__init__()
        norm = lambda c: nn.InstanceNorm2d(c, affine=False, track_running_stats=False)    # noqa: E731
        L = [nn.ReplicationPad2d(3), nn.Conv2d(3, ngf, 7), norm(ngf), nn.ReLU(True)]
        for i in range(n_downsample):
            c = ngf << i
            L += [nn.Conv2d(c, 2 * c, 3, stride=2, padding=1), norm(2 * c), nn.ReLU(True)]
        L += [ResBlk(ngf << n_downsample) for _ in range(n_blocks)]
        for i in range(n_upsample):
            c = ngf << (n_downsample - i)
            L += [nn.ConvTranspose2d(c, c // 2, 3, stride=2, padding=1, output_padding=1), norm(c // 2), nn.ReLU(True)]
        if n_upsample > 0:
            L += [nn.ReplicationPad2d(3), nn.Conv2d(c // 2, out_ch, 7)]
        self.layers = nn.Sequential(*L)

    def forward(self, x):
        return self.layers(x)


def init_like_reference(net):
    """KeypointNeRF.init_weights(net) with its defaults (src/model.py:610-640)."""
    def f(m):
        torch.manual_seed(125)
        name = type(m).__name__
        if hasattr(m, "weight") and ("Conv" in name or "Linear" in name):
            nn.init.normal_(m.weight.data, 0.0, 0.02)
            if getattr(m, "bias", None) is not None:
                nn.init.constant_(m.bias.data, 0.0)
    net.apply(f)


def perturb(net, seed):
    """Seeded perturbation of every parameter: 0.01 N(0,1) on weights of rank > 1, 0.1 N(0,1) on biases, gamma and beta."""
    with torch.no_grad():
        for i, (_, p) in enumerate(net.named_parameters()):
            g = torch.Generator().manual_seed(seed + i)
            p.add_(torch.randn(p.shape, generator=g, dtype=torch.float32) * (0.01 if p.dim() > 1 else 0.1))


def seeded(net, seed):
    init_like_reference(net)
    perturb(net, seed)
    return net.eval()


def checksums(net):
    """Two exact integer sums over the bit patterns of every parameter tensor (independent of summation order and threads)."""
    out = []
    for _, p in net.named_parameters():
        b = p.detach().cpu().contiguous().numpy().view(np.int32).astype(np.int64).reshape(-1)
        out.append([int(b.sum()), int((b >> 9).sum())])
    return np.array(out, np.int64)


def stand_in_geo(seed, out_ch=64, out_ch_hd=8):
    return seeded(HGFilterV2(out_ch, out_ch_hd), seed)


def stand_in_tex(seed):
    a = TEX_ARGS
    return seeded(ResBlkEncoder(a["out_ch"], a["ngf"], a["n_downsample"], a["n_blocks"], a["n_upsample"]), seed)


GEO_STAGE_MODULES = ("conv1", "conv2", "unpack1.conv", "conv4", "top_m_0", "conv_last0", "m0") + \
    tuple(f"m0.b{j}_{lv}" for lv in (1, 2, 3, 4) for j in (1, 3))
TEX_STAGE_MODULES = {"stem": "layers.1", "down1": "layers.4", "down2": "layers.7", "down3": "layers.10", "res1": "layers.13",
                     "res2": "layers.14", "res3": "layers.15", "res4": "layers.16", "up1": "layers.17", "up2": "layers.20"}


def run_with_stages(net, x, names):
    """(outputs, {stage name: NCHW tensor}) with forward hooks on the named sub-modules (names: {stage: module path})."""
    mods, got, hooks = dict(net.named_modules()), {}, []
    for st, path in names.items():
        hooks.append(mods[path].register_forward_hook(lambda m, i, o, st=st: got.__setitem__(st, o.detach().clone())))
    with torch.no_grad():
        out = net(x)
    for h in hooks:
        h.remove()
    return out, got


def case_image(shape, seed):
    """The source images of a golden case, in [0, 1): torch's CPU generator is reproducible across machines."""
    return torch.rand(tuple(int(v) for v in shape), generator=torch.Generator().manual_seed(int(seed)))


def golden_reference(G, case, tag, i):
    """(fp64 reference values, flat indices or None (= every element), NCHW shape, e_ref) of output i of a case."""
    key = f"{case}_{tag}{i}"
    idx = G[key + "_idx"] if key + "_idx" in G.files else None
    return G[key + "_f64"], idx, tuple(int(v) for v in G[key + "_shape"]), float(G[key + "_eref"])


def net_input(img, ds):
    x = img
    for _ in range(ds):
        x = F.avg_pool2d(x, 2, stride=2)
    return 2.0 * x - 1.0


# ---- emulator driver (host memory) ----
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _stages(info, args, flat):
    out, name = {}, ctypes.create_string_buffer(64)
    off, dims = ctypes.c_int64(0), (ctypes.c_int32 * 4)()
    i = 0
    while info(*args, i, name, 64, ctypes.byref(off), dims) == 0:
        n = dims[0] * dims[1] * dims[2] * dims[3]
        out[name.value.decode()] = flat[off.value:off.value + n].reshape(*dims)
        i += 1
    return out


def emu_geo(L, plain, img, ds, out_ch=64, out_ch_hd=8, eps=1e-5, want_stages=True):
    """kpn_geo_encode through library L with numpy buffers -> (feat NHWC, feat_hd NHWC, stages)"""
    plain, img = np.ascontiguousarray(plain, np.float32), np.ascontiguousarray(img, np.float32)
    assert plain.size == L.kpn_geo_encoder_plain_floats(out_ch, out_ch_hd)
    packed = np.zeros(L.kpn_geo_encoder_packed_floats(out_ch, out_ch_hd), np.float32)
    L.check(L.kpn_geo_encoder_pack_device(_ptr(plain), _ptr(packed), out_ch, out_ch_hd, None))
    V, _, H, W = img.shape
    args = (V, H, W, ds, out_ch, out_ch_hd)
    nb = L.kpn_geo_encoder_workspace_bytes(*args)
    assert nb > 0
    h, w = H >> ds, W >> ds
    feat, hd = np.full((V, h // 4, w // 4, out_ch), np.nan, np.float32), np.full((V, h, w, out_ch_hd), np.nan, np.float32)
    st = np.full(L.kpn_geo_encoder_stage_floats(*args), np.nan, np.float32) if want_stages else None
    ws = np.zeros(nb // 4 + 4, np.float32)
    L.check(L.kpn_geo_encode(_ptr(img), *args, _ptr(packed), eps, _ptr(feat), _ptr(hd), _ptr(st), _ptr(ws), nb, None))
    return feat, hd, (_stages(L.kpn_geo_encoder_stage_info, args, st) if want_stages else None)


def emu_tex(L, plain, img, ds, cfg=(64, 3, 4, 2, 8), eps=1e-5, want_stages=True):
    plain, img = np.ascontiguousarray(plain, np.float32), np.ascontiguousarray(img, np.float32)
    assert plain.size == L.kpn_tex_encoder_plain_floats(*cfg)
    packed = np.zeros(L.kpn_tex_encoder_packed_floats(*cfg), np.float32)
    L.check(L.kpn_tex_encoder_pack_device(_ptr(plain), _ptr(packed), *cfg, None))
    V, _, H, W = img.shape
    args = (V, H, W, ds) + tuple(cfg)
    nb = L.kpn_tex_encoder_workspace_bytes(*args)
    assert nb > 0
    h, w = H >> ds, W >> ds
    for _ in range(cfg[1]):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    feat = np.full((V, h << cfg[3], w << cfg[3], cfg[4]), np.nan, np.float32)
    st = np.full(L.kpn_tex_encoder_stage_floats(*args), np.nan, np.float32) if want_stages else None
    ws = np.zeros(nb // 4 + 4, np.float32)
    L.check(L.kpn_tex_encode(_ptr(img), *args, _ptr(packed), eps, _ptr(feat), _ptr(st), _ptr(ws), nb, None))
    return feat, (_stages(L.kpn_tex_encoder_stage_info, args, st) if want_stages else None)
