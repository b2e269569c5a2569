"""The perceptual term of the training loss, VGGLoss (reference src/utils.py:750-805), on the device: vgg19.features[0:21]
applied to the rendered and the target patch, the L1 distances of its four relu taps, and the gradient to the rendered
patch — ``torch.ops.kpnerf.vgg_loss`` (kpn_vgg_loss, csrc/vgg_kernels.hip).

The weights stay the caller's: ``NativeVGGLoss(module)`` reads ``vgg_net.slice1..4``, ``weights`` and ``normalize.mean/std``
of the reference's ``VGGLoss`` instance and packs them on the device (again whenever a parameter changes).  It has
``VGGLoss.forward``'s signature, so it can be passed as ``vggloss=`` to ``losses.compute_error`` or to the reference's own.
``install_vgg(net)`` rebinds ``net.vgg_loss.forward`` on the instance — module tree and ``state_dict`` names stay as they are,
so checkpoints load unchanged — and ``uninstall_vgg(net)`` restores it.  Nothing changes unless the caller installs it.

Served: CUDA fp32 (B, 3, H, W) pairs with H, W >= 8; anything else (CPU tensors, smaller patches) goes to the module's own
forward.  Refused at construction (NotImplementedError): slices that differ from vgg19.features[0:21] (kernel, stride,
padding, dilation, groups, bias, pool mode) and VGG parameters with requires_grad=True (no weight gradient is built; the
reference freezes them, src/utils.py:772-774).
"""
import torch

from . import ops
from . import torch_ops  # noqa: F401  (registers torch.ops.kpnerf.*)
from .dropin import _version_key

# vgg19.features[0:21] split as Vgg19 splits it (src/utils.py:759-770): ("conv", cin, cout) | "relu" | "pool"
VGG_SLICES = (
    (("conv", 3, 64), "relu"),
    (("conv", 64, 64), "relu", "pool", ("conv", 64, 128), "relu"),
    (("conv", 128, 128), "relu", "pool", ("conv", 128, 256), "relu"),
    (("conv", 256, 256), "relu", ("conv", 256, 256), "relu", ("conv", 256, 256), "relu", "pool", ("conv", 256, 512), "relu"),
)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _check_layer(m, spec, where):
    nn = torch.nn
    if spec == "relu":
        ok = isinstance(m, nn.ReLU)
    elif spec == "pool":
        ok = (isinstance(m, nn.MaxPool2d) and _pair(m.kernel_size) == (2, 2) and _pair(m.stride) == (2, 2)
              and _pair(m.padding) == (0, 0) and _pair(m.dilation) == (1, 1) and not m.ceil_mode and not m.return_indices)
    else:
        _, cin, cout = spec
        ok = (isinstance(m, nn.Conv2d) and m.in_channels == cin and m.out_channels == cout and _pair(m.kernel_size) == (3, 3)
              and _pair(m.stride) == (1, 1) and _pair(m.padding) == (1, 1) and _pair(m.dilation) == (1, 1) and m.groups == 1
              and m.bias is not None and m.padding_mode == "zeros")
    if not ok:
        raise NotImplementedError(f"{where}: {m} is not the layer of vgg19.features[0:21] the kernels implement ({spec})")


def vgg_convs(vgg_module):
    """The nine Conv2d modules of a VGGLoss instance, in features order, after checking every slice against
    vgg19.features[0:21] and that no VGG parameter requires a gradient (NotImplementedError otherwise)."""
    net = vgg_module.vgg_net
    convs = []
    for si, specs in enumerate(VGG_SLICES):
        sl = list(getattr(net, f"slice{si + 1}").children())
        if len(sl) != len(specs):
            raise NotImplementedError(f"vgg_net.slice{si + 1} has {len(sl)} layers, vgg19.features[0:21] has {len(specs)} there")
        for j, (m, spec) in enumerate(zip(sl, specs)):
            _check_layer(m, spec, f"vgg_net.slice{si + 1}[{j}]")
            if spec not in ("relu", "pool"):
                convs.append(m)
    for name, p in vgg_module.named_parameters():
        if p.requires_grad:
            raise NotImplementedError(f"VGG parameter {name} requires a gradient: the native term builds no weight gradient "
                                      "(the reference freezes them, src/utils.py:772-774)")
    return convs


def plain_from_module(vgg_module, device=None):
    """The flat parameter vector kpn_vgg_pack_device takes: each convolution's OIHW weight, then its bias."""
    parts = []
    for c in vgg_convs(vgg_module):
        parts += [c.weight.detach().reshape(-1), c.bias.detach().reshape(-1)]
    flat = torch.cat([p.to(device=device or p.device, dtype=torch.float32) for p in parts])
    return flat


def module_consts(vgg_module):
    """mean[3] + std[3] (VGGLoss.normalize) + the four tap weights (VGGLoss.weights), as floats."""
    def floats(v):
        return [float(u) for u in torch.as_tensor(v, dtype=torch.float64).reshape(-1)]
    mean, std, w = floats(vgg_module.normalize.mean), floats(vgg_module.normalize.std), floats(vgg_module.weights)
    if len(mean) != 3 or len(std) != 3 or len(w) != 4:
        raise NotImplementedError("VGGLoss with other than 3 normalisation channels / 4 tap weights")
    return mean + std + w


class NativeVGGLoss:
    """``VGGLoss.forward(x, y)`` of ``vgg_module`` (reference src/utils.py:795-805) through kpn_vgg_loss."""

    def __init__(self, vgg_module):
        self.module = vgg_module
        self.convs = vgg_convs(vgg_module)
        module_consts(vgg_module)
        self.reference_forward = type(vgg_module).forward.__get__(vgg_module)
        self.packed = None
        self.key = None

    def served(self, x, y):
        return (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.is_cuda and y.is_cuda
                and x.dtype == torch.float32 and y.dtype == torch.float32 and x.dim() == 4 and x.shape == y.shape
                and x.shape[1] == 3 and x.shape[2] >= 8 and x.shape[3] >= 8)

    def packed_weights(self, device):
        params = [t for c in self.convs for t in (c.weight, c.bias)]
        key = _version_key(params)
        if key is None or key != self.key or self.packed is None or self.packed.device != device:
            with torch.no_grad():
                self.packed = ops.vgg_pack(plain_from_module(self.module, device=device))
            self.key = key
        return self.packed

    def __call__(self, x, y):
        if not self.served(x, y):
            return self.reference_forward(x, y)
        consts = module_consts(self.module)
        return torch.ops.kpnerf.vgg_loss(x.contiguous(), y.detach().contiguous(), self.packed_weights(x.device), consts, 1.0)[0]


def install_vgg(net):
    """Serves ``net.vgg_loss`` (a reference VGGLoss) natively: rebinds its ``forward`` on the instance.  Returns ``net``."""
    net.vgg_loss.forward = NativeVGGLoss(net.vgg_loss)
    return net


def uninstall_vgg(net):
    net.vgg_loss.__dict__.pop("forward", None)
    return net
