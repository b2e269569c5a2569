"""Test helpers of the native VGG perceptual term (kpn_vgg_loss; reference VGGLoss, src/utils.py:750-805): the seeded
stand-in for vgg19.features[0:21] the golden case_v_vgg_loss.npz was recorded with (scripts/make_vgg_golden.py), and the
three parity rules of the issue in fp64:

1. stage-wise forward: every convolution's output (the library's `stages`) against fp64 (normalize / pool ->) conv -> bias
   -> ReLU of the library's OWN previous stage, |d| <= 2e-6 (sum|w a| + |b|) per element (fp32-MFMA error model, K <= 2304);
2. decision-matched backward: an fp64 backward that takes its ReLU masks, L1 signs and first-max pool arg-maxes from the
   library's stages;
3. end to end against the reference's fp64 result, with every differing decision inside the margin of rule 1.

Pure torch on the CPU: the GPU tests use it too (the oracle is built on the CPU, not through MIOpen's fp64 path)."""
import numpy as np
import torch
import torch.nn.functional as F

CONV = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 512)]
POOLED_IN = (2, 4, 8)        # convolutions that read a 2x2 max-pool of the previous one
TAPS = (0, 2, 4, 8)          # relu1_1, relu2_1, relu3_1, relu4_1
LEVEL = (0, 0, 1, 1, 2, 2, 2, 2, 3)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
TAP_W = (1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)
RULE1 = 2e-6


def features(seed):
    """vgg19.features[0:21] with seeded default init (the pretrained weights cannot be had offline)."""
    torch.manual_seed(seed)
    layers = []
    for i in range(9):
        if i in POOLED_IN:
            layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2, padding=0, dilation=1, ceil_mode=False))
        layers += [torch.nn.Conv2d(CONV[i][0], CONV[i][1], kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
    return torch.nn.Sequential(*layers)


def conv_params(feats):
    return [(m.weight.detach(), m.bias.detach()) for m in feats if isinstance(m, torch.nn.Conv2d)]


def checksums(feats):
    """per convolution: sum and sum of squares (fp64) of the weight and of the bias"""
    out = []
    for w, b in conv_params(feats):
        w, b = w.double(), b.double()
        out.append([float(w.sum()), float((w * w).sum()), float(b.sum()), float((b * b).sum())])
    return np.array(out, np.float64)


def plain(feats):
    return torch.cat([t.reshape(-1) for wb in conv_params(feats) for t in wb]).float()


def check_checksums(feats, recorded):
    got = checksums(feats)
    assert np.allclose(got, recorded, rtol=1e-9, atol=1e-9), ("the seeded VGG weights changed (torch RNG?)", got - recorded)


def stages_nchw(flat, B, H, W):
    """the library's `stages` buffer -> list of 9 fp64 (2B, C, H_l, W_l) tensors (x images first)"""
    flat = torch.as_tensor(np.asarray(flat)).reshape(-1)
    out, off = [], 0
    for l in range(9):
        h, w, c = H >> LEVEL[l], W >> LEVEL[l], CONV[l][1]
        n = 2 * B * h * w * c
        out.append(flat[off:off + n].reshape(2 * B, h, w, c).permute(0, 3, 1, 2).double())
        off += n
    assert off == flat.numel()
    return out


def normalize64(x):
    m = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return (torch.as_tensor(np.asarray(x)).double() - m) / s


def rule1(x, y, st, params, B):
    """-> (worst |d| / bound over all layers, fp64 loss from the library's own stages)"""
    inp = normalize64(np.concatenate([np.asarray(x), np.asarray(y)]))
    worst = 0.0
    for l, (w, b) in enumerate(params):
        if l > 0:
            inp = F.max_pool2d(st[l - 1], 2, 2) if l in POOLED_IN else st[l - 1]
        w64, b64 = w.double(), b.double()
        z = F.conv2d(inp, w64, b64, padding=1)
        bound = RULE1 * (F.conv2d(inp.abs(), w64.abs(), padding=1) + b64.abs().view(1, -1, 1, 1))
        worst = max(worst, float(((st[l] - z.clamp_min(0)).abs() / bound).max()))
    loss = sum(TAP_W[t] * float((st[l][:B] - st[l][B:]).abs().mean()) for t, l in enumerate(TAPS))
    return worst, loss


def unpool_first_max(g, a):
    """max_pool2d(2, 2, floor) backward: g (B, C, h, w) goes to the first maximum (row-major) of each window of a"""
    B, C, H, W = a.shape
    h, w = H // 2, W // 2
    win = a[:, :, :2 * h, :2 * w].reshape(B, C, h, 2, w, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, h, w, 4)
    hot = F.one_hot(win.argmax(-1), 4).to(g.dtype) * g.unsqueeze(-1)
    out = torch.zeros_like(a)
    out[:, :, :2 * h, :2 * w] = hot.reshape(B, C, h, w, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h, 2 * w)
    return out


def decision_matched_backward(st, params, B, lam=1.0):
    """fp64 d loss / d x with the ReLU masks, L1 signs and pool arg-maxes of the library's stages"""
    d = None
    for l in range(8, -1, -1):
        a = st[l][:B]
        if l in TAPS:
            t = TAPS.index(l)
            seed = torch.sign(st[l][:B] - st[l][B:]) * (lam * TAP_W[t] / a.numel())
            d = seed if d is None else d + seed
        g = d * (a > 0)
        din = F.conv_transpose2d(g, params[l][0].double(), padding=1)
        if l == 0:
            return din / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
        d = unpool_first_max(din, st[l - 1][:B]) if l in POOLED_IN else din


def reference64(x, y, params):
    """the reference's fp64 forward (pre-activations of every convolution) for x and y"""
    inp = normalize64(np.concatenate([np.asarray(x), np.asarray(y)]))
    zs, acts, bounds = [], [], []
    for l, (w, b) in enumerate(params):
        if l > 0:
            inp = F.max_pool2d(acts[-1], 2, 2) if l in POOLED_IN else acts[-1]
        w64, b64 = w.double(), b.double()
        z = F.conv2d(inp, w64, b64, padding=1)
        zs.append(z)
        bounds.append(RULE1 * (F.conv2d(inp.abs(), w64.abs(), padding=1) + b64.abs().view(1, -1, 1, 1)))
        acts.append(z.clamp_min(0))
    return zs, acts, bounds


def differing_decisions(st, zs, acts, bounds, B):
    """decisions of the library (its stages) that differ from the fp64 reference's: -> (count, count outside the margin)"""
    n = bad = 0
    for l in range(9):
        flip = (st[l] > 0) != (zs[l] > 0)                      # ReLU masks (x and y)
        n += int(flip.sum())
        bad += int((flip & (zs[l].abs() > bounds[l])).sum())
        if l in TAPS:                                          # L1 signs
            s_lib, s_ref = torch.sign(st[l][:B] - st[l][B:]), torch.sign(acts[l][:B] - acts[l][B:])
            flip = s_lib != s_ref
            margin = bounds[l][:B] + bounds[l][B:]
            n += int(flip.sum())
            bad += int((flip & ((acts[l][:B] - acts[l][B:]).abs() > margin)).sum())
        if l + 1 in POOLED_IN:                                 # pool arg-maxes (x images)
            def wins(a):
                Bn, C, H, W = a.shape
                h, w = H // 2, W // 2
                return a[:, :, :2 * h, :2 * w].reshape(Bn, C, h, 2, w, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C, h, w, 4)
            wl, wr, wb = wins(st[l][:B]), wins(acts[l][:B]), wins(bounds[l][:B])
            flip = wl.argmax(-1) != wr.argmax(-1)
            top = wr.topk(2, -1).values
            gap = top[..., 0] - top[..., 1]
            n += int(flip.sum())
            bad += int((flip & (gap > 2 * wb.max(-1).values)).sum())
    return n, bad


def end_to_end(loss, dx, g, case):
    """rule 3 numbers: (rel loss err, cosine of d_x) vs the reference's fp64, and the reference's own fp32 ones"""
    l64, d64 = float(g[f"{case}_loss64"]), np.asarray(g[f"{case}_dx64"], np.float64).reshape(-1)
    d = np.asarray(dx, np.float64).reshape(-1)
    l32, d32 = float(g[f"{case}_loss32"]), np.asarray(g[f"{case}_dx32"], np.float64).reshape(-1)

    def cos(a, b):
        return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    return abs(float(loss) - l64) / abs(l64), cos(d, d64), abs(l32 - l64) / abs(l64), cos(d32, d64)


class _Normalize(torch.nn.Module):
    """what VGGLoss.normalize is (torchvision.transforms.Normalize): mean / std kept as lists, (v - mean) / std"""

    def __init__(self, mean, std):
        super().__init__()
        self.mean, self.std = list(mean), list(std)

    def forward(self, t):
        m = torch.as_tensor(self.mean, dtype=t.dtype, device=t.device).view(-1, 1, 1)
        s = torch.as_tensor(self.std, dtype=t.dtype, device=t.device).view(-1, 1, 1)
        return t.sub(m).div(s)


class StandInVGGLoss(torch.nn.Module):
    """A module with VGGLoss's attributes (vgg_net.slice1..4, weights, normalize; reference src/utils.py:750-805) and its
    forward, over the seeded features — the caller's module the native term reads, where the reference is not mounted."""

    def __init__(self, seed=0):
        super().__init__()
        f = features(seed)
        self.vgg_net = torch.nn.Module()
        for i, (a, b) in enumerate(((0, 2), (2, 7), (7, 12), (12, 21))):
            sl = torch.nn.Sequential()
            for k in range(a, b):
                sl.add_module(str(k), f[k])
            setattr(self.vgg_net, f"slice{i + 1}", sl)
        for p in self.parameters():
            p.requires_grad = False
        self.weights = list(TAP_W)
        self.normalize = _Normalize(MEAN, STD)

    def forward(self, x, y):
        x, y = self.normalize(x), self.normalize(y)
        loss = 0
        hx, hy = x, y
        for i in range(4):
            sl = getattr(self.vgg_net, f"slice{i + 1}")
            hx, hy = sl(hx), sl(hy)
            loss += self.weights[i] * torch.nn.functional.l1_loss(hx, hy.detach())
        return loss
