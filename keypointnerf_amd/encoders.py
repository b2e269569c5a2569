"""The two image encoders in front of the ray march on the device, forward only: the reference's HGFilterV2 (geometry) and
ResBlkEncoder (texture), src/utils.py:199-474 — ``ops.geo_encode`` / ``ops.tex_encode`` (kpn_geo_encode / kpn_tex_encode,
csrc/encoder_kernels.hip).

The weights stay the caller's: ``NativeGeoEncoder(module)`` / ``NativeTexEncoder(module)`` read the caller's module by
structure (sub-modules, eps, group counts, affine parameters, biases), pack once on the device and again whenever a
parameter's identity, storage or version changes.  What the kernels do not implement is refused at construction with a
NotImplementedError that names it: norm="batch", hd=True, n_stack != 1, a ResBlkEncoder with another norm, unexpected layers.

``install_encoders(net, geo=True, tex=False)`` rebinds ``net.attach_geo_feat`` / ``net.attach_tex_feat`` on the instance
(src/model.py:653-680): when no gradient is needed (``not net.training``, or gradients disabled, or no encoder parameter
requires one) and the images are CUDA fp32, the maps come from the native encoders, otherwise from the module's own forward
(training keeps autograd).  The maps have the reference's NCHW shapes, dtype and device, in channels-last memory.
``uninstall_encoders(net)`` restores what was bound before.  Nothing changes unless the caller installs them; ``install(net)``
does not.  The texture encoder is off by default: on the 3 x 512^2 source set it is slower than the module on MIOpen
(profiles/encoders.md); ``tex=True`` serves it natively all the same.

``install_native_convs(module)`` is a separate opt-in for training: it puts torch.ops.kpnerf.conv2d (HIP forward and backward of one
stride-1 convolution) behind the eligible ``nn.Conv2d`` instances of a module tree; ``uninstall_native_convs`` undoes it.
``install_native_norms`` does the same for ``nn.GroupNorm`` / ``nn.InstanceNorm2d`` (torch.ops.kpnerf.group_norm), and
``install_native_blocks`` rebinds whole ConvBlocks to ``group_norm(relu=True)`` + ``conv2d`` legs.  ``install_native_hourglass``
rebinds a whole HourGlass to its own recursion with torch.ops.kpnerf.avg_pool2 and torch.ops.kpnerf.upsample2x_add between the
blocks, whatever forward those have.  ``install_native_strided`` serves what ``install_native_convs`` leaves: the stride-2 3x3
convolutions, the 7x7 stride-2 stem and the ConvTranspose2d layers (torch.ops.kpnerf.conv2d_down2 / conv_transpose2d_up2).  The five
are independent: they rebind different modules, so they compose and uninstall in any order.  ``install_native_geo`` applies all
five to every HGFilterV2 and rebinds its forward so that the functional calls in it run on the project's kernels too.
``install_native_tex`` does the same for every ResBlkEncoder: ``install_native_strided`` and ``install_native_norms`` on its subtree,
and a forward that runs every ReplicationPad2d + Conv2d pair as torch.ops.kpnerf.conv2d_replicate and every InstanceNorm2d + ReLU
pair as one fused torch.ops.kpnerf.group_norm; with ``fused=True`` the forward is one torch.ops.kpnerf.res_encoder call instead.
"""
import types

import torch

from . import lib as kl
from . import ops
from . import torch_ops  # noqa: F401  (registers torch.ops.kpnerf.*)
from .dropin import _version_key


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _refuse(what):
    raise NotImplementedError(f"native encoders: {what} is not implemented")


def _check_conv(m, where, cin, cout, k, stride, pad, bias, transposed=False):
    nn = torch.nn
    cls = nn.ConvTranspose2d if transposed else nn.Conv2d
    ok = (type(m) is cls and m.in_channels == cin and m.out_channels == cout and _pair(m.kernel_size) == (k, k)
          and _pair(m.stride) == (stride, stride) and _pair(m.padding) == (pad, pad) and _pair(m.dilation) == (1, 1)
          and m.groups == 1 and (m.bias is not None) == bias and m.padding_mode == "zeros"
          and (not transposed or _pair(m.output_padding) == (1, 1)))
    if not ok:
        _refuse(f"{where}: {m} (expected {cls.__name__}({cin}, {cout}, kernel_size={k}, stride={stride}, padding={pad}, bias={bias}))")
    return [m.weight] + ([m.bias] if bias else [])


def _check_gn(m, where, groups, C, eps_seen):
    if type(m) is torch.nn.BatchNorm2d:
        _refuse(f'{where}: norm="batch" (BatchNorm2d)')
    if type(m) is not torch.nn.GroupNorm or m.num_groups != groups or m.num_channels != C or not m.affine:
        _refuse(f"{where}: {m} (expected GroupNorm({groups}, {C}))")
    eps_seen.add(float(m.eps))
    return [m.weight, m.bias]


def _conv_block_params(m, where, cin, cout, eps_seen):
    """bn1, conv1, bn2, conv2, bn3, conv3 [, bn4, downsample convolution] of a ConvBlock (src/utils.py:416-474)."""
    if type(m).__name__ != "ConvBlock":
        _refuse(f"{where}: {type(m).__name__} where a ConvBlock is expected")
    p, w = [], (cin, cout // 2, cout // 4)
    outs = (cout // 2, cout // 4, cout // 4)
    for i in range(3):
        p += _check_gn(getattr(m, f"bn{i + 1}"), f"{where}.bn{i + 1}", min(32, w[i]), w[i], eps_seen)
        p += _check_conv(getattr(m, f"conv{i + 1}"), f"{where}.conv{i + 1}", w[i], outs[i], 3, 1, 1, False)
    if not isinstance(m.nl, torch.nn.ReLU):
        _refuse(f"{where}.nl: {m.nl}")
    if cin != cout:
        ds = m.downsample
        if ds is None or len(ds) != 3 or ds[0] is not m.bn4 or not isinstance(ds[1], torch.nn.ReLU):
            _refuse(f"{where}.downsample: {ds}")
        p += _check_gn(m.bn4, f"{where}.bn4", min(32, cin), cin, eps_seen)
        p += _check_conv(ds[2], f"{where}.downsample[2]", cin, cout, 1, 1, 0, False)
    elif m.downsample is not None:
        _refuse(f"{where}.downsample: {m.downsample}")
    return p


def geo_params(module):
    """(parameters in the order kpn_geo_encoder_pack_device takes them, out_ch, out_ch_hd, eps) of an HGFilterV2, after
    checking its structure against what the kernels implement (NotImplementedError otherwise)."""
    if type(module).__name__ != "HGFilterV2":
        _refuse(f"{type(module).__name__} as geometry encoder (HGFilterV2 expected)")
    if getattr(module, "n_stack", None) != 1:
        _refuse(f"n_stack={getattr(module, 'n_stack', None)} (stacked hourglasses; n_stack=1 only)")
    if getattr(module, "hd", False):
        _refuse("hd=True")
    known = {"nl", "unpack1", "conv_out", "conv1", "bn1", "conv2", "conv3", "conv4", "m0", "top_m_0", "conv_last0", "bn_end0", "l0"}
    extra = [n for n, _ in module.named_children() if n not in known]
    if extra or not all(hasattr(module, n) for n in known):
        _refuse(f"an HGFilterV2 with the layers {sorted(extra) or sorted(known - {n for n, _ in module.named_children()})}")
    eps = set()
    p = _check_conv(module.conv1, "conv1", 3, 64, 7, 2, 3, True)
    p += _check_gn(module.bn1, "bn1", 32, 64, eps)
    p += _conv_block_params(module.conv2, "conv2", 64, 128, eps)
    un = module.unpack1
    if type(un).__name__ != "DeconvReLUGroup" or not isinstance(un.nl, torch.nn.ReLU):
        _refuse(f"unpack1: {un}")
    p += _check_conv(un.conv, "unpack1.conv", 128, 32, 3, 2, 1, False, transposed=True)
    p += _check_gn(un.norm, "unpack1.norm", 32, 32, eps)
    out_ch_hd = module.conv_out.out_channels
    p += _check_conv(module.conv_out, "conv_out", 32, out_ch_hd, 5, 1, 2, True)
    p += _conv_block_params(module.conv3, "conv3", 128, 128, eps)
    p += _conv_block_params(module.conv4, "conv4", 128, 256, eps)
    hg = module.m0
    if type(hg).__name__ != "HourGlass" or hg.depth != 4 or hg.features != 256:
        _refuse(f"m0: {type(hg).__name__}(depth={getattr(hg, 'depth', None)}, features={getattr(hg, 'features', None)}) (HourGlass(4, 256) only)")
    names = [f"b{j}_{lv}" for lv in (4, 3, 2, 1) for j in (1, 2)] + ["b2_plus_1", "b3_1", "b3_2", "b3_3", "b3_4"]
    if sorted(n for n, _ in hg.named_children()) != sorted(names):
        _refuse(f"m0 with the layers {[n for n, _ in hg.named_children()]}")
    for n in names:
        p += _conv_block_params(getattr(hg, n), f"m0.{n}", 256, 256, eps)
    p += _conv_block_params(module.top_m_0, "top_m_0", 256, 256, eps)
    p += _check_conv(module.conv_last0, "conv_last0", 256, 256, 1, 1, 0, True)
    p += _check_gn(module.bn_end0, "bn_end0", 32, 256, eps)
    out_ch = module.l0.out_channels
    p += _check_conv(module.l0, "l0", 256, out_ch, 1, 1, 0, True)
    if len(eps) != 1:
        _refuse(f"GroupNorm layers with different eps {sorted(eps)}")
    return p, out_ch, out_ch_hd, eps.pop()


def _check_in(m, where, C, eps_seen):
    if type(m) is not torch.nn.InstanceNorm2d or m.affine or m.track_running_stats or m.num_features != C:
        _refuse(f'{where}: {m} (a ResBlkEncoder with another norm than "instance")')
    eps_seen.add(float(m.eps))


def _check_pad(m, where, n):
    if type(m) is not torch.nn.ReplicationPad2d or tuple(m.padding) != (n, n, n, n):
        _refuse(f"{where}: {m} (expected ReplicationPad2d({n}))")


def tex_params(module):
    """(parameters in `layers` order, (ngf, n_downsample, n_blocks, n_upsample, out_ch), eps) of a ResBlkEncoder."""
    if type(module).__name__ != "ResBlkEncoder":
        _refuse(f"{type(module).__name__} as texture encoder (ResBlkEncoder expected)")
    L = list(module.layers)
    eps, p = set(), []
    if len(L) < 4 or type(L[1]) is not torch.nn.Conv2d:
        _refuse(f"a ResBlkEncoder starting with {L[:2]}")
    ngf = L[1].out_channels
    _check_pad(L[0], "layers.0", 3)
    p += _check_conv(L[1], "layers.1", 3, ngf, 7, 1, 0, True)
    _check_in(L[2], "layers.2", ngf, eps)
    i, C, n_down, n_blocks, n_up = 4, ngf, 0, 0, 0
    if not isinstance(L[3], torch.nn.ReLU):
        _refuse(f"layers.3: {L[3]}")
    while i + 2 < len(L) and type(L[i]) is torch.nn.Conv2d:
        p += _check_conv(L[i], f"layers.{i}", C, 2 * C, 3, 2, 1, True)
        C *= 2
        _check_in(L[i + 1], f"layers.{i + 1}", C, eps)
        if not isinstance(L[i + 2], torch.nn.ReLU):
            _refuse(f"layers.{i + 2}: {L[i + 2]}")
        i, n_down = i + 3, n_down + 1
    while i < len(L) and type(L[i]).__name__ == "ResBlk":
        b = list(L[i].layers)
        if len(b) != 7 or not isinstance(b[3], torch.nn.ReLU):
            _refuse(f"layers.{i}: a ResBlk with the layers {b}")
        for j in (0, 4):
            _check_pad(b[j], f"layers.{i}.layers.{j}", 1)
            p += _check_conv(b[j + 1], f"layers.{i}.layers.{j + 1}", C, C, 3, 1, 0, True)
            _check_in(b[j + 2], f"layers.{i}.layers.{j + 2}", C, eps)
        i, n_blocks = i + 1, n_blocks + 1
    while i + 2 < len(L) and type(L[i]) is torch.nn.ConvTranspose2d:
        p += _check_conv(L[i], f"layers.{i}", C, C // 2, 3, 2, 1, True, transposed=True)
        C //= 2
        _check_in(L[i + 1], f"layers.{i + 1}", C, eps)
        if not isinstance(L[i + 2], torch.nn.ReLU):
            _refuse(f"layers.{i + 2}: {L[i + 2]}")
        i, n_up = i + 3, n_up + 1
    if n_up == 0 or i + 2 != len(L):
        _refuse(f"a ResBlkEncoder whose layers continue with {L[i:i + 3]} (n_upsample=0 or unexpected layers)")
    _check_pad(L[i], f"layers.{i}", 3)
    out_ch = L[i + 1].out_channels
    p += _check_conv(L[i + 1], f"layers.{i + 1}", C, out_ch, 7, 1, 0, True)
    if len(eps) != 1:
        _refuse(f"InstanceNorm2d layers with different eps {sorted(eps)}")
    return p, (ngf, n_down, n_blocks, n_up, out_ch), eps.pop()


def flat_plain(params, device=None):
    return torch.cat([t.detach().reshape(-1).to(device=device or t.device, dtype=torch.float32) for t in params])


class _NativeEncoder:
    calls = 0      # native forward calls of all instances (the tests assert that a call was, or was not, served natively)

    def packed_weights(self, device):
        key = _version_key(self.params)
        if key is None or key != self.key or self.packed is None or self.packed.device != device:
            with torch.no_grad():
                self.packed = self._pack(flat_plain(self.params, device=device))
            self.key = key
        return self.packed


class NativeGeoEncoder(_NativeEncoder):
    """``HGFilterV2.forward(2 * avg_pool2d^ds(im) - 1)`` of ``module`` through kpn_geo_encode."""

    def __init__(self, module):
        self.module = module
        self.params, self.out_ch, self.out_ch_hd, self.eps = geo_params(module)
        self.packed = self.key = None

    def _pack(self, plain):
        return ops.geo_encoder_pack(plain, self.out_ch, self.out_ch_hd)

    def __call__(self, im, ds=0, want_stages=False):
        """im: (V, 3, H, W) in [0, 1] -> [feat (V, out_ch, h/4, w/4), feat_hd (V, out_ch_hd, h, w)] (NCHW shapes, channels-last
        memory), as HGFilterV2.forward returns them."""
        type(self).calls += 1
        if want_stages:
            f, fhd, st = ops.geo_encode(im, self.packed_weights(im.device), ds, self.out_ch, self.out_ch_hd, self.eps, True)
        else:
            st = None
            f, fhd = torch.ops.kpnerf.geo_encode(im, self.packed_weights(im.device), [int(ds), self.out_ch, self.out_ch_hd], self.eps)
        out = [f.permute(0, 3, 1, 2), fhd.permute(0, 3, 1, 2)]
        return (out, st) if want_stages else out


class NativeTexEncoder(_NativeEncoder):
    """``ResBlkEncoder.forward(2 * avg_pool2d^ds(im) - 1)`` of ``module`` through kpn_tex_encode."""

    def __init__(self, module):
        self.module = module
        self.params, self.cfg, self.eps = tex_params(module)
        self.packed = self.key = None

    def _pack(self, plain):
        return ops.tex_encoder_pack(plain, *self.cfg)

    def __call__(self, im, ds=0, want_stages=False):
        type(self).calls += 1
        if want_stages:
            f, st = ops.tex_encode(im, self.packed_weights(im.device), ds, *self.cfg, eps=self.eps, want_stages=True)
        else:
            st = None
            f = torch.ops.kpnerf.tex_encode(im, self.packed_weights(im.device), [int(ds)] + list(self.cfg), self.eps)
        out = f.permute(0, 3, 1, 2)
        return (out, st) if want_stages else out


def _served(net, enc, im):
    no_grad = (not net.training) or (not torch.is_grad_enabled()) or not any(p.requires_grad for p in enc.params)
    return (no_grad and isinstance(im, torch.Tensor) and ops._on_gpu(im) and im.dtype == torch.float32 and im.dim() in (4, 5)
            and not (im.requires_grad and torch.is_grad_enabled()))


def install_encoders(net, geo=True, tex=False):
    """Serves ``net.attach_geo_feat`` / ``net.attach_tex_feat`` (src/model.py:653-680) natively when no gradient is needed;
    the module's own forward (whatever was bound before, e.g. by ``dropin.install``) otherwise.  Returns ``net``."""
    uninstall_encoders(net)
    saved = {}
    if geo:
        enc = NativeGeoEncoder(net.geo_encoder)
        prev = net.attach_geo_feat
        saved["attach_geo_feat"] = net.__dict__.get("attach_geo_feat")

        def attach_geo_feat(self, im, return_val=False):
            im4 = im.view(-1, *im.shape[2:]) if isinstance(im, torch.Tensor) and im.dim() == 5 else im
            if (not _served(self, enc, im4) or self.ds_geo > 1 or (im4.shape[-2] >> self.ds_geo) % 64
                    or (im4.shape[-1] >> self.ds_geo) % 64):
                return prev(im, return_val)
            if not return_val:
                self.im = im.clone()
            self.feat_geo = enc(im4, ds=self.ds_geo)
            st = self.__dict__.get("_kpnerf_state")
            if st is not None and not return_val:
                st.note_attached(im)
            if return_val:
                return self.feat_geo

        net.attach_geo_feat = types.MethodType(attach_geo_feat, net)
        net._kpnerf_native_geo = enc
    if tex and getattr(net, "tex_encoder", None) is not None:
        enct = NativeTexEncoder(net.tex_encoder)
        prevt = net.attach_tex_feat
        saved["attach_tex_feat"] = net.__dict__.get("attach_tex_feat")

        def attach_tex_feat(self, im, return_val=False):
            im4 = im.view(-1, *im.shape[2:]) if isinstance(im, torch.Tensor) and im.dim() == 5 else im
            if not _served(self, enct, im4) or self.ds_tex > 1:
                return prevt(im, return_val)
            self.feat_tex = enct(im4, ds=self.ds_tex)
            st = self.__dict__.get("_kpnerf_state")
            if st is not None and not return_val:
                st.note_attached_tex(im)
            if return_val:
                return self.feat_tex

        net.attach_tex_feat = types.MethodType(attach_tex_feat, net)
        net._kpnerf_native_tex = enct
    net._kpnerf_encoder_saved = saved
    return net


def uninstall_encoders(net):
    saved = net.__dict__.pop("_kpnerf_encoder_saved", None)
    if saved is not None:
        for k, v in saved.items():
            if v is None:
                net.__dict__.pop(k, None)
            else:
                net.__dict__[k] = v
    for k in ("_kpnerf_native_geo", "_kpnerf_native_tex"):
        net.__dict__.pop(k, None)
    return net


# ---- the opt-in installers below rebind ``forward`` on single module instances; this is their one scaffold ----
def _restore_forward(module, key):
    for m in module.modules():
        if key in m.__dict__:
            saved = m.__dict__.pop(key)
            if saved is None:
                m.__dict__.pop("forward", None)
            else:
                m.__dict__["forward"] = saved
    return module


def _rebind_forward(module, key, candidate, ineligible, make_forward):
    """Undoes an earlier install under ``key`` (what that installer's uninstaller does), then rebinds ``forward`` on every module
    under ``module`` that ``candidate(m)`` selects and for which ``ineligible(m, name)`` gives no reason, to ``make_forward(prev)``,
    ``prev`` being the forward the instance had.  What the instance's own ``forward`` attribute was (None when the class's forward
    was in place) is kept under ``key`` for ``_restore_forward``.  Returns (served, left): the names served and {name: reason}."""
    _restore_forward(module, key)
    served, left = [], {}
    for name, m in module.named_modules():
        if not candidate(m):
            continue
        why = ineligible(m, name)
        if why is not None:
            left[name] = why
            continue
        prev = m.forward
        setattr(m, key, m.__dict__.get("forward"))
        m.forward = types.MethodType(make_forward(prev), m)
        served.append(name)
    return served, left


# ---- training convolutions natively: torch.ops.kpnerf.conv2d behind the nn.Conv2d instances of a module tree ----
# The installers of the stride-1 convolutions and of the ConvBlocks take ``arith``: "f32" (the default: the fp32 MFMA kernels) or "bf16x3"
# (every operand as three bf16 pieces on the 16-bit MFMA, csrc/encoder_split_kernels.hip; torch.ops.kpnerf.conv2d_arith /
# conv_block_arith).  The stems, the stride-2, transposed and replication-padded layers have no split kernel and stay on their fp32 ones.
_ARITH = {"f32": 0, "bf16x3": 1}


def _arith_code(arith):
    if arith not in _ARITH:
        raise ValueError(f'arith must be "f32" or "bf16x3", got {arith!r}')
    return _ARITH[arith]


def _conv_ineligible(m, arith=0):
    """None if kpn_conv2d_* serves this nn.Conv2d, else the reason it is left on torch"""
    k, s, p, d = _pair(m.kernel_size), _pair(m.stride), m.padding, _pair(m.dilation)
    if isinstance(p, str):
        return f"padding={p!r}"
    p = _pair(p)
    if s != (1, 1):
        return f"stride={s[0] if s[0] == s[1] else s}"
    if d != (1, 1):
        return f"dilation={d}"
    if m.groups != 1:
        return f"groups={m.groups}"
    if m.padding_mode != "zeros":
        return f"padding_mode={m.padding_mode!r}"
    if k[0] != k[1] or k[0] not in (1, 3, 5):
        return f"kernel_size={k} (1, 3 or 5, square)"
    if p[0] != p[1] or not 0 <= p[0] <= k[0] - 1:
        return f"padding={p} (0 .. k - 1, the same on both axes)"
    if m.in_channels % 4 or m.out_channels % 4 or not ops.conv2d_supported(m.in_channels, m.out_channels, k[0], arith):
        return f"channels {m.in_channels} -> {m.out_channels} (multiples of 4, at most 1024)"
    return None


def install_native_convs(module, arith="f32"):
    """Opt-in: rebinds ``forward`` on every eligible ``nn.Conv2d`` instance under ``module`` to torch.ops.kpnerf.conv2d, forward and
    backward in HIP (kpn_conv2d_forward / kpn_conv2d_backward).  Eligible: groups = 1, dilation = 1, stride 1, a square kernel of
    1, 3 or 5, zero padding 0 .. k - 1 (``padding_mode="zeros"``), channel counts that are multiples of 4.  Every other layer
    (stride 2, the 7x7 stems, ConvTranspose2d, ...) is left on torch, not refused.  The rebound forward serves CUDA fp32 input and
    calls the module's own forward for anything else; its result is channels_last.  The module tree, the parameter names and the
    state_dict are untouched.  Independent of ``install_encoders``: both may be installed on one ``net`` (the whole-network
    native forward still wins where it is served).  Returns (served, left): the names served, and {name: reason} of the
    nn.Conv2d layers left alone.  ``arith="bf16x3"``: every served layer runs torch.ops.kpnerf.conv2d_arith on three bf16 pieces per
    operand (kpn_conv2d_ex_*); the same layers are eligible."""
    a = _arith_code(arith)

    def make_forward(_prev):
        def forward(self, x):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                    and self.weight.is_cuda and self.weight.dtype == torch.float32):
                return _prev(x)
            if a:
                return torch.ops.kpnerf.conv2d_arith(x, self.weight, self.bias, _pair(self.padding)[0], a)
            return torch.ops.kpnerf.conv2d(x, self.weight, self.bias, _pair(self.padding)[0])
        return forward

    return _rebind_forward(module, "_kpnerf_conv_saved", lambda m: type(m) is torch.nn.Conv2d, lambda m, name: _conv_ineligible(m, a),
                           make_forward)


def uninstall_native_convs(module):
    """Restores what ``forward`` was on every layer ``install_native_convs`` rebound (the class's bound method, or an earlier
    instance attribute)."""
    return _restore_forward(module, "_kpnerf_conv_saved")


# ---- training normalisations natively: torch.ops.kpnerf.group_norm behind nn.GroupNorm / nn.InstanceNorm2d ----
class NativeTraining:
    """native forward calls served by the rebound norms, blocks, hourglasses, strided layers, HGFilterV2s and ResBlkEncoders of all modules (the tests assert that a call was served
    natively)"""
    norm_calls = 0
    block_calls = 0
    fused_block_calls = 0
    hourglass_calls = 0
    strided_calls = 0
    geo_calls = 0
    tex_calls = 0
    fused_tex_calls = 0
    fused_geo_calls = 0


def _pow2_channels(C):
    return 4 <= C <= 1024 and not C & (C - 1)


def _norm_ineligible(m):
    """None if kpn_group_norm_* serves this nn.GroupNorm / nn.InstanceNorm2d, else the reason it is left on torch"""
    if type(m) is torch.nn.InstanceNorm2d:
        if m.affine:
            return "affine=True (an InstanceNorm2d with parameters)"
        if m.track_running_stats:
            return "track_running_stats=True (running statistics)"
        C = m.num_features
    else:
        C = m.num_channels
    if not _pow2_channels(C):
        return f"channels {C} (a power of two in 4 .. 1024)"
    return None


def _native_input(x, *params):
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and all(p is None or (p.is_cuda and p.dtype == torch.float32) for p in params))


def install_native_norms(module):
    """Opt-in: rebinds ``forward`` on every eligible ``nn.GroupNorm`` and ``nn.InstanceNorm2d`` instance under ``module`` to
    torch.ops.kpnerf.group_norm (``relu=False``), forward and backward in HIP (kpn_group_norm_forward / kpn_group_norm_backward).
    Eligible: a channel count that is a power of two in 4 .. 1024; an InstanceNorm2d only with ``affine=False`` and
    ``track_running_stats=False``.  Every other layer is left on torch, not refused.  The rebound forward serves CUDA fp32
    (N, C, H, W) input and calls the module's own forward for anything else; its result is channels_last.  The module tree, the
    parameter names and the state_dict are untouched.  Returns (served, left): the names served, and {name: reason} of the layers
    left alone."""
    def make_forward(_prev):
        def forward(self, x):
            w, b = getattr(self, "weight", None), getattr(self, "bias", None)
            if not _native_input(x, w, b):
                return _prev(x)
            NativeTraining.norm_calls += 1
            groups = self.num_groups if isinstance(self, torch.nn.GroupNorm) else self.num_features
            return torch.ops.kpnerf.group_norm(x, w, b, groups, self.eps, False)
        return forward

    return _rebind_forward(module, "_kpnerf_norm_saved", lambda m: type(m) in (torch.nn.GroupNorm, torch.nn.InstanceNorm2d),
                           lambda m, name: _norm_ineligible(m), make_forward)


def uninstall_native_norms(module):
    """Restores what ``forward`` was on every layer ``install_native_norms`` rebound."""
    return _restore_forward(module, "_kpnerf_norm_saved")


# ---- whole ConvBlocks natively: group_norm(relu=True) + conv2d per leg ----
def _block_ineligible(m, name):
    """None if every leg of this ConvBlock is served by kpn_group_norm_* and kpn_conv2d_*, else the reason"""
    try:
        cin, cout = m.bn1.num_channels, 2 * m.conv1.out_channels
        _conv_block_params(m, name or "block", cin, cout, set())
    except NotImplementedError as e:
        return str(e)
    except AttributeError as e:
        return f"native encoders: {name or 'block'}: {e}"
    widths = (cin, cout // 2, cout // 4)
    if not all(_pow2_channels(w) for w in widths):
        return f"channels {widths} (the norms need powers of two in 4 .. 1024)"
    return None


def _fused_block_ineligible(m, name, arith=0):
    """_block_ineligible, and that kpn_conv_block_* serves the widths and every norm has one eps"""
    why = _block_ineligible(m, name)
    if why is not None:
        return why
    cin, cout = m.bn1.num_channels, 2 * m.conv1.out_channels
    if not ops.conv_block_supported(cin, cout, arith):
        return f"channels {cin} -> {cout} (the single-operator block serves at most 1024 output channels behind a downsample leg)"
    eps = {float(getattr(m, f"bn{i}").eps) for i in range(1, 5 if cin != cout else 4)}
    if len(eps) != 1:
        return f"the norms have different eps {sorted(eps)}"
    return None


def install_native_blocks(module, fused=False, arith="f32"):
    """Opt-in: rebinds ``forward`` on every ConvBlock under ``module`` whose structure is the reference's (src/utils.py:416-474; the
    check the native encoder makes) to the same dataflow on the project's kernels: each ``bn -> nl -> conv`` leg, the downsample leg
    included, is torch.ops.kpnerf.group_norm(relu=True) followed by torch.ops.kpnerf.conv2d; ``torch.cat`` and the residual add
    stay on torch.  A ConvBlock that fails the check is left alone.  CPU or non-fp32 input goes to the original forward.  The module
    tree, the parameter names and the state_dict are untouched.  Returns (served, left): the names served, and {name: reason} of
    the ConvBlocks left alone.

    ``fused=True``: the rebound forward is one torch.ops.kpnerf.conv_block call instead (kpn_conv_block_forward / _backward): one
    autograd node per block, no aten operator inside it - the norms and the ReLUs run in the loads of the convolutions, forward and
    backward, the convolutions write their slices of the concatenation, the residual is added once - and x plus 3/4 of an
    output-sized tensor kept for the backward instead of every leg's input and normalised input.  Its forward has the bits of the
    unfused path.  ``NativeTraining.fused_block_calls`` counts these calls (``block_calls`` the unfused ones).

    ``arith="bf16x3"``: the convolutions of every served block run on three bf16 pieces per operand - torch.ops.kpnerf.conv2d_arith per leg,
    or torch.ops.kpnerf.conv_block_arith with ``fused=True`` (whose forward again has the bits of the unfused path in that arithmetic).  The
    norms do not change."""
    a = _arith_code(arith)

    def make_fused(_prev):
        def forward(self, x):
            if not _native_input(x, *self.parameters()):
                return _prev(x)
            NativeTraining.fused_block_calls += 1
            legs = [(self.bn1, self.conv1), (self.bn2, self.conv2), (self.bn3, self.conv3)]
            if self.downsample is not None:
                legs.append((self.bn4, self.downsample[2]))
            tensors = [t for bn, conv in legs for t in (bn.weight, bn.bias, conv.weight)]
            if a:
                return torch.ops.kpnerf.conv_block_arith(x, tensors, self.bn1.eps, a)
            return torch.ops.kpnerf.conv_block(x, tensors, self.bn1.eps)
        return forward

    if fused:
        return _rebind_forward(module, "_kpnerf_block_saved", lambda m: type(m).__name__ == "ConvBlock",
                               lambda m, name: _fused_block_ineligible(m, name, a), make_fused)

    def make_forward(_prev):
        def forward(self, x):
            if not _native_input(x, *self.parameters()):
                return _prev(x)
            NativeTraining.block_calls += 1

            def leg(bn, conv, t, pad):
                t = torch.ops.kpnerf.group_norm(t, bn.weight, bn.bias, bn.num_groups, bn.eps, True)
                if a:
                    return torch.ops.kpnerf.conv2d_arith(t, conv.weight, None, pad, a)
                return torch.ops.kpnerf.conv2d(t, conv.weight, None, pad)

            o1 = leg(self.bn1, self.conv1, x, 1)
            o2 = leg(self.bn2, self.conv2, o1, 1)
            o3 = leg(self.bn3, self.conv3, o2, 1)
            out = torch.cat((o1, o2, o3), 1)
            out += x if self.downsample is None else leg(self.bn4, self.downsample[2], x, 0)
            return out
        return forward

    return _rebind_forward(module, "_kpnerf_block_saved", lambda m: type(m).__name__ == "ConvBlock", _block_ineligible, make_forward)


def uninstall_native_blocks(module):
    """Restores what ``forward`` was on every ConvBlock ``install_native_blocks`` rebound, fused or not."""
    return _restore_forward(module, "_kpnerf_block_saved")


# ---- a whole HourGlass natively: avg_pool2 and upsample2x_add between whatever forwards its ConvBlocks have ----
def _hourglass_ineligible(m):
    """None if this HourGlass has the reference's structure (src/utils.py:261-306) and a channel count the resampling kernels serve,
    else the reason it is left on torch"""
    depth, features = getattr(m, "depth", None), getattr(m, "features", None)
    if not isinstance(depth, int) or isinstance(depth, bool) or depth < 1:
        return f"depth={depth!r} (an integer >= 1)"
    want = [f"b{j}_{k}" for k in range(1, depth + 1) for j in (1, 2, 3)] + ["b2_plus_1"]
    missing = [n for n in want if not isinstance(m._modules.get(n), torch.nn.Module)]
    if missing:
        return f"missing children {', '.join(missing)}"
    if not isinstance(features, int) or isinstance(features, bool) or features < 4 or features % 4:
        return f"features={features!r} (a positive multiple of 4)"
    return None


def install_native_hourglass(module):
    """Opt-in: rebinds ``forward`` on every HourGlass under ``module`` whose structure is the reference's (an integer ``depth`` >= 1,
    children ``b1_k``, ``b2_k``, ``b3_k`` for k = 1 .. depth and ``b2_plus_1``, ``features`` a multiple of 4) to the same recursion
    (src/utils.py:287-306) with torch.ops.kpnerf.avg_pool2 in place of ``avg_pool2d`` and torch.ops.kpnerf.upsample2x_add in place of
    ``up1 + interpolate(...)``, forward and backward in HIP.  The blocks run whatever forward they have, so this composes with
    ``install_native_blocks`` / ``install_native_norms`` / ``install_native_convs`` in any order.  Input that is not a CUDA fp32
    (N, C, H, W) tensor with H and W divisible by 2^depth goes to the original forward.  The module tree, the parameter names and the
    state_dict are untouched.  Returns (served, left): the names served, and {name: reason} of the HourGlasses left alone."""
    def make_forward(_prev):
        def forward(self, x):
            if not _native_input(x) or x.shape[2] % (1 << self.depth) or x.shape[3] % (1 << self.depth):
                return _prev(x)
            NativeTraining.hourglass_calls += 1

            def run(level, inp):
                up1 = self._modules[f"b1_{level}"](inp)
                low = self._modules[f"b2_{level}"](torch.ops.kpnerf.avg_pool2(inp))
                low = run(level - 1, low) if level > 1 else self._modules[f"b2_plus_{level}"](low)
                low = self._modules[f"b3_{level}"](low)
                return torch.ops.kpnerf.upsample2x_add(low, up1)

            return run(self.depth, x)
        return forward

    return _rebind_forward(module, "_kpnerf_hourglass_saved", lambda m: type(m).__name__ == "HourGlass",
                           lambda m, name: _hourglass_ineligible(m), make_forward)


def uninstall_native_hourglass(module):
    """Restores what ``forward`` was on every HourGlass ``install_native_hourglass`` rebound."""
    return _restore_forward(module, "_kpnerf_hourglass_saved")


# ---- the resolution-changing layers natively: torch.ops.kpnerf.conv2d_down2 / conv_transpose2d_up2 ----
def _strided_candidate(m):
    """the layers install_native_strided answers for: every nn.ConvTranspose2d, and the nn.Conv2d that are not stride 1 (those are
    install_native_convs')"""
    return type(m) is torch.nn.ConvTranspose2d or (type(m) is torch.nn.Conv2d and _pair(m.stride) != (1, 1))


def _strided_ineligible(m):
    """None if kpn_conv2d_s2_* serves this layer, else the reason it is left on torch"""
    k, s, p, d = _pair(m.kernel_size), _pair(m.stride), m.padding, _pair(m.dilation)
    transposed = type(m) is torch.nn.ConvTranspose2d
    if isinstance(p, str):
        return f"padding={p!r}"
    p = _pair(p)
    if s != (2, 2):
        return f"stride={s} (2)"
    if d != (1, 1):
        return f"dilation={d}"
    if m.groups != 1:
        return f"groups={m.groups}"
    if m.padding_mode != "zeros":
        return f"padding_mode={m.padding_mode!r}"
    if k not in (((3, 3),) if transposed else ((3, 3), (7, 7))):
        return f"kernel_size={k} ({'3' if transposed else '3 or 7'}, square)"
    if p != (k[0] // 2, k[0] // 2):
        return f"padding={p} ({k[0] // 2} for kernel_size {k[0]})"
    if transposed and _pair(m.output_padding) != (1, 1):
        return f"output_padding={_pair(m.output_padding)} (1)"
    kind = kl.S2_DECONV3 if transposed else (kl.S2_STEM7 if k[0] == 7 else kl.S2_CONV3)
    if not ops.conv2d_s2_supported(kind, m.in_channels, m.out_channels):
        return (f"channels {m.in_channels} -> {m.out_channels} " +
                ("(at most 4 input channels, output channels a multiple of 4)" if kind == kl.S2_STEM7 else "(multiples of 4, at most 1024)"))
    return None


def install_native_strided(module):
    """Opt-in: rebinds ``forward`` on the resolution-changing layers under ``module`` to the project's kernels, forward and backward in
    HIP (kpn_conv2d_s2_forward / kpn_conv2d_s2_backward): ``nn.Conv2d`` with stride 2 and (kernel_size, padding) = (3, 1) or (7, 3) -
    torch.ops.kpnerf.conv2d_down2 - and ``nn.ConvTranspose2d`` with kernel_size 3, stride 2, padding 1, output_padding 1 -
    torch.ops.kpnerf.conv_transpose2d_up2; groups = 1, dilation = 1, zero padding, channel counts that are multiples of 4 (the 7x7 stem:
    at most 4 input channels).  It serves none of the layers ``install_native_convs`` serves, and lists every other strided or
    transposed layer with its reason.  The rebound forward calls the module's own forward for input that is not a CUDA fp32
    (N, C, H, W) tensor, for odd H or W in front of a 3x3 stride-2 convolution, and for a stem input that requires a gradient (the
    stem has no native input gradient); its result is channels_last.  The module tree, the parameter names and the state_dict are
    untouched.  Returns (served, left): the names served, and {name: reason} of the layers left alone."""
    def make_forward(_prev):
        def forward(self, x, *args, **kwargs):
            if args or kwargs or not _native_input(x, self.weight, self.bias):
                return _prev(x, *args, **kwargs)
            if type(self) is torch.nn.ConvTranspose2d:
                NativeTraining.strided_calls += 1
                return torch.ops.kpnerf.conv_transpose2d_up2(x, self.weight, self.bias)
            if _pair(self.kernel_size)[0] == 3 and (x.shape[2] % 2 or x.shape[3] % 2):
                return _prev(x)
            if _pair(self.kernel_size)[0] == 7 and x.requires_grad and torch.is_grad_enabled():
                return _prev(x)
            NativeTraining.strided_calls += 1
            return torch.ops.kpnerf.conv2d_down2(x, self.weight, self.bias)
        return forward

    return _rebind_forward(module, "_kpnerf_strided_saved", _strided_candidate, lambda m, name: _strided_ineligible(m), make_forward)


def uninstall_native_strided(module):
    """Restores what ``forward`` was on every layer ``install_native_strided`` rebound."""
    return _restore_forward(module, "_kpnerf_strided_saved")


# ---- a whole HGFilterV2 natively: the five installers above on its subtree, and its own forward on the project's kernels ----
def _geo_ineligible(m, name):
    """None if this HGFilterV2 has the reference's structure (src/utils.py:322-414, norm = "group", any n_stack >= 1, hd either way)
    and its fused norms and its pool are served, else the reason it is left alone"""
    n_stack = getattr(m, "n_stack", None)
    if not isinstance(n_stack, int) or isinstance(n_stack, bool) or n_stack < 1:
        return f"n_stack={n_stack!r} (an integer >= 1)"
    if not hasattr(m, "hd"):
        return "no attribute hd"
    want = {"nl": None, "unpack1": "DeconvReLUGroup", "conv_out": "Conv2d", "conv1": "Conv2d", "bn1": "GroupNorm", "conv2": "ConvBlock",
            "conv3": "ConvBlock", "conv4": "ConvBlock"}
    for i in range(n_stack):
        want.update({f"m{i}": "HourGlass", f"top_m_{i}": "ConvBlock", f"conv_last{i}": "Conv2d", f"bn_end{i}": "GroupNorm", f"l{i}": "Conv2d"})
        if i < n_stack - 1:
            want.update({f"bl{i}": "Conv2d", f"al{i}": "Conv2d"})
    have = dict(m.named_children())
    if set(have) != set(want):
        return f"children {sorted(set(have) ^ set(want))} missing or unexpected (an HGFilterV2 with n_stack={n_stack})"
    for n, t in want.items():
        if type(have[n]) is torch.nn.BatchNorm2d:
            return f'{n}: norm="batch" (BatchNorm2d)'
        if t is not None and type(have[n]).__name__ != t:
            return f"{n}: {type(have[n]).__name__} where {t} is expected"
    un = m.unpack1
    if type(getattr(un, "conv", None)) is not torch.nn.ConvTranspose2d or type(getattr(un, "norm", None)) is not torch.nn.GroupNorm \
            or not isinstance(getattr(un, "nl", None), torch.nn.ReLU):
        return f"unpack1: {un} (ConvTranspose2d, ReLU, GroupNorm expected)"
    if not isinstance(m.nl, torch.nn.ReLU):
        return f"nl: {m.nl}"
    for n in ["bn1", "unpack1.norm"] + [f"bn_end{i}" for i in range(n_stack)]:      # the norms the forward fuses with their ReLU
        why = _norm_ineligible(m.get_submodule(n))
        if why is not None:
            return f"{n}: {why}"
    if not m.hd and m.conv2.conv1.out_channels % 2:
        return f"conv2: {2 * m.conv2.conv1.out_channels} channels in front of the pool (a multiple of 4)"
    return None


_GEO_PARTS = ("strided", "convs", "norms", "blocks", "hourglass")


def _fused_geo_plan(m):
    """([(module, parameter name)] in the tensor order of torch.ops.kpnerf.hg_filter, depth, eps) if kpn_hg_filter_* serves this HGFilterV2
    (one that _geo_ineligible has passed), else the reason it stays on the per-layer path"""
    if m.n_stack != 1:
        return f"n_stack={m.n_stack} (the single-operator network has one stack)"
    if m.hd:
        return "hd=True (the single-operator network pools in front of conv3)"
    why = _hourglass_ineligible(m.m0)
    if why is not None:
        return f"m0: {why}"
    hg = m.m0
    blocks = [("conv2", m.conv2), ("conv3", m.conv3), ("conv4", m.conv4)]
    blocks += [(f"m0.b{j}_{k}", hg._modules[f"b{j}_{k}"]) for k in range(hg.depth, 0, -1) for j in (1, 2)]
    blocks += [("m0.b2_plus_1", hg._modules["b2_plus_1"])] + [(f"m0.b3_{k}", hg._modules[f"b3_{k}"]) for k in range(1, hg.depth + 1)]
    blocks.append(("top_m_0", m.top_m_0))
    refs = [(m.conv1, "weight"), (m.conv1, "bias"), (m.bn1, "weight"), (m.bn1, "bias")]
    norms, widths = [("bn1", m.bn1), ("unpack1.norm", m.unpack1.norm), ("bn_end0", m.bn_end0)], []
    for name, b in blocks:
        why = _fused_block_ineligible(b, name)
        if why is not None:
            return f"{name}: {why}"
        cin, cout = b.bn1.num_channels, 2 * b.conv1.out_channels
        widths.append((cin, cout))
        legs = [(b.bn1, b.conv1), (b.bn2, b.conv2), (b.bn3, b.conv3)] + ([(b.bn4, b.downsample[2])] if cin != cout else [])
        for i, (bn, conv) in enumerate(legs):
            norms.append((f"{name}.bn{i + 1}", bn))
            refs += [(bn, "weight"), (bn, "bias"), (conv, "weight")]
    un, tail = m.unpack1, [m.conv_out, m.conv_last0, m.l0]
    refs += [(un.conv, "weight"), (un.norm, "weight"), (un.norm, "bias"), (m.conv_out, "weight"), (m.conv_out, "bias"),
             (m.conv_last0, "weight"), (m.conv_last0, "bias"), (m.bn_end0, "weight"), (m.bn_end0, "bias"), (m.l0, "weight"), (m.l0, "bias")]
    if un.conv.bias is not None:
        return "unpack1.conv has a bias"
    if m.conv1.bias is None or any(c.bias is None for c in tail):
        return "a convolution without bias among conv1, conv_out, conv_last0, l0"
    for n, norm in norms:
        if norm.weight is None or norm.num_groups != min(32, norm.num_channels):
            return f"{n}: GroupNorm({norm.num_groups}, {norm.num_channels}) (min(32, C) groups with parameters)"
    eps = {float(norm.eps) for _, norm in norms}
    if len(eps) != 1:
        return f"the norms have different eps {sorted(eps)}"
    k = [(c, _pair(c.kernel_size), _pair(c.stride), _pair(c.padding)) for c in [m.conv1] + tail]
    if [t[1:] for t in k] != [((7, 7), (2, 2), (3, 3)), ((5, 5), (1, 1), (2, 2)), ((1, 1), (1, 1), (0, 0)), ((1, 1), (1, 1), (0, 0))] \
            or any(c.groups != 1 or _pair(c.dilation) != (1, 1) or c.padding_mode != "zeros" for c, *_ in k):
        return "conv1, conv_out, conv_last0 or l0 is not the reference's layer (7x7 stride 2, 5x5 pad 2, 1x1, 1x1)"
    if _strided_ineligible(un.conv) is not None:
        return f"unpack1.conv: {_strided_ineligible(un.conv)}"
    c4 = widths[2][1]
    chain = [m.conv1.out_channels, widths[0][1], widths[1][1], c4]
    if [w[0] for w in widths[:3]] != chain[:3] or any(w != (c4, c4) for w in widths[3:]) or hg.features != c4 \
            or un.conv.in_channels != chain[1] or m.conv_out.in_channels != un.conv.out_channels \
            or (m.conv_last0.in_channels, m.conv_last0.out_channels, m.l0.in_channels) != (c4, c4, c4):
        return "the widths of the layers do not chain as the reference's do"
    cfg = (m.conv1.in_channels, chain[0], chain[1], chain[2], c4, hg.depth, un.conv.out_channels, m.conv_out.out_channels, m.l0.out_channels)
    why = ops.hg_filter_refusal(cfg)
    if why is not None:
        return f"the single-operator network does not serve it: {why}"
    return refs, hg.depth, eps.pop()


def install_native_geo(module, fused_blocks=False, arith="f32", fused=False):
    """Opt-in: trains every HGFilterV2 under ``module`` (``module`` itself included) on the project's kernels.  An HGFilterV2 whose
    structure is the reference's (src/utils.py:322-414: its children for any ``n_stack`` >= 1, ``norm="group"``, ``hd`` either way) gets
    ``install_native_strided``, ``install_native_convs``, ``install_native_norms``, ``install_native_blocks`` and
    ``install_native_hourglass`` on its subtree, and its ``forward`` is rebound to the same dataflow with
    ``conv1 -> torch.ops.kpnerf.group_norm(bn1, relu=True)``, the transposed convolution of ``unpack1`` followed by the same fused norm,
    torch.ops.kpnerf.avg_pool2 in place of ``avg_pool2d`` and ``group_norm(bn_end_i, relu=True)`` behind ``conv_last_i``: no
    convolution, normalisation, pool, upsample or ReLU is left to torch; ``torch.cat`` and the residual / skip adds are.  Input that
    is not a CUDA fp32 (N, C, H, W) tensor whose stem output has even H and W goes to the original forward.  The module tree, the
    parameter names and the state_dict are untouched.  Returns {installer: (served, left)} for "geo" and the five installers, the
    names relative to ``module``; a layer that one of the five leaves because it is another's (the stride-2 stem among the
    nn.Conv2d) is not listed as left.  ``fused_blocks=True`` installs the ConvBlocks as ``install_native_blocks(fused=True)`` does:
    one torch.ops.kpnerf.conv_block per block, and no ``torch.cat`` or residual add left inside a block.

    ``arith="bf16x3"``: the stride-1 convolutions and the ConvBlocks (``install_native_convs`` / ``install_native_blocks`` with the same
    keyword) run on three bf16 pieces per operand; the stem and the transposed convolution of ``unpack1`` have no such kernel and stay on
    their fp32 ones.  The report then has one more entry, ``"arith": {"bf16x3": [names], "f32": [names]}``: the served convolution
    layers and blocks on each arithmetic.  Any other value raises ValueError; the default leaves the report as it was.

    ``fused=True``: the rebound forward of every served HGFilterV2 that kpn_hg_filter_* serves - ``n_stack == 1``, ``hd`` false, one
    ``eps`` over all norms, ``min(32, C)`` groups on every norm, widths the descriptor accepts - is one torch.ops.kpnerf.hg_filter call
    instead (kpn_hg_filter_forward / _backward): one autograd node per network and no aten operator inside it - the norms and ReLUs of
    ``unpack1`` and ``bn_end0`` run in the loads of the next convolution, the sums where a tensor feeds two consumers run in the
    backward's kernels - with x and one ``state`` buffer kept for the backward.  Its outputs and parameter gradients have the bits of the
    ``fused_blocks=True`` path.  Such a network gets none of the five installers on its subtree.  Input that is not a CUDA fp32
    (N, C, H, W) tensor with H and W divisible by 2^(depth + 2), or that requires a gradient (the stem has no native input gradient),
    goes to the original forward.  A network the operator does not serve stays on the per-layer path exactly as without the keyword;
    the report gains ``"fused"``: (the names on the operator, {name: reason} of those left on the per-layer path).
    ``NativeTraining.fused_geo_calls`` counts the operator's calls (``geo_calls`` the per-layer ones).  ``fused=True`` with
    ``arith="bf16x3"`` raises ValueError: the operator has no such arithmetic."""
    _arith_code(arith)
    if fused and arith != "f32":
        raise ValueError('install_native_geo: fused=True runs the fp32 kernels only; arith="bf16x3" needs the per-layer path (fused=False)')

    def make_forward(_prev):
        def forward(self, x):
            plan = self.__dict__.get("_kpnerf_geo_fused")
            if plan is not None:
                refs, depth, eps = plan
                f = 4 << depth
                if (not _native_input(x, *self.parameters()) or x.shape[2] % f or x.shape[3] % f
                        or (x.requires_grad and torch.is_grad_enabled())):
                    return _prev(x)
                NativeTraining.fused_geo_calls += 1
                return torch.ops.kpnerf.hg_filter(x, [getattr(a, n) for a, n in refs], depth, eps)
            if not _native_input(x, *self.parameters()) or (((x.shape[2] - 1) // 2 + 1) % 2 or ((x.shape[3] - 1) // 2 + 1) % 2):
                return _prev(x)
            NativeTraining.geo_calls += 1

            def gn(norm, t):
                return torch.ops.kpnerf.group_norm(t, norm.weight, norm.bias, norm.num_groups, norm.eps, True)

            x = self.conv2(gn(self.bn1, self.conv1(x)))
            x_hd = self.conv_out(gn(self.unpack1.norm, self.unpack1.conv(x)))
            if not self.hd:
                x = torch.ops.kpnerf.avg_pool2(x)
            previous = self.conv4(self.conv3(x))
            sub = self._modules
            for i in range(self.n_stack):
                ll = sub[f"top_m_{i}"](sub[f"m{i}"](previous))
                ll = gn(sub[f"bn_end{i}"], sub[f"conv_last{i}"](ll))
                out = sub[f"l{i}"](ll)
                if i < self.n_stack - 1:
                    previous = previous + sub[f"bl{i}"](ll) + sub[f"al{i}"](out)
            return [out, x_hd]
        return forward

    uninstall_native_geo(module)
    served, left = _rebind_forward(module, "_kpnerf_geo_saved", lambda m: type(m).__name__ == "HGFilterV2", _geo_ineligible, make_forward)
    report = {k: ([], {}) for k in _GEO_PARTS}
    subs = dict(module.named_modules())
    if fused:
        report["fused"] = ([], {})
    for name in served:
        if fused:
            plan = _fused_geo_plan(subs[name])
            if not isinstance(plan, str):
                subs[name]._kpnerf_geo_fused = plan
                report["fused"][0].append(name)
                continue
            report["fused"][1][name] = plan
        for part, fn in zip(_GEO_PARTS, (install_native_strided, lambda m: install_native_convs(m, arith=arith), install_native_norms,
                                         lambda m: install_native_blocks(m, fused=fused_blocks, arith=arith), install_native_hourglass)):
            s_, l_ = fn(subs[name])
            pre = name + "." if name else ""
            report[part][0].extend(pre + n for n in s_)
            report[part][1].update({pre + n: why for n, why in l_.items()})
    everything = {n for part in _GEO_PARTS for n in report[part][0]}
    for part in _GEO_PARTS:
        for n in [n for n in report[part][1] if n in everything]:
            del report[part][1][n]
    report["geo"] = (served, left)
    if arith != "f32":
        # a convolution inside a served block is the block's: listed once, under the block
        blocks = report["blocks"][0]
        own = [n for n in report["convs"][0] if not any(n.startswith(b + ".") for b in blocks)]
        report["arith"] = {arith: sorted(own + blocks), "f32": sorted(report["strided"][0])}
    return report


def uninstall_native_geo(module):
    """Restores what ``forward`` was on every HGFilterV2 ``install_native_geo`` rebound, and undoes the five installers on its
    subtree: no attribute it added is left."""
    for m in module.modules():
        if "_kpnerf_geo_saved" in m.__dict__:
            m.__dict__.pop("_kpnerf_geo_fused", None)
            for undo in (uninstall_native_strided, uninstall_native_convs, uninstall_native_norms, uninstall_native_blocks,
                         uninstall_native_hourglass):
                undo(m)
    return _restore_forward(module, "_kpnerf_geo_saved")


# ---- a whole ResBlkEncoder natively: the replication-padded convolutions, the fused norms and the two installers its other layers need ----
def _tex_structure_error(m):
    """None if this ResBlkEncoder has the reference's structure (the check of ``tex_params``, with an output layer), else the reason"""
    L = list(getattr(m, "layers", ()))
    if len(L) < 2 or type(L[-1]) is not torch.nn.Conv2d or type(L[-2]) is not torch.nn.ReplicationPad2d:
        return (f"layers.{len(L) - 1}: {type(L[-1]).__name__ if L else 'nothing'} where the output layer ReplicationPad2d(3) + Conv2d(k 7) "
                "is expected (n_upsample=0)")
    try:
        tex_params(m)
    except NotImplementedError as e:
        return str(e)
    return None


def _tex_ineligible(m, name):
    """None if this ResBlkEncoder has the reference's structure (src/utils.py:199-259, norm = "instance": the check the native encoder
    makes) and every one of its layers is served by its kernel, else the reason it is left alone"""
    why = _tex_structure_error(m)
    if why is not None:
        return why
    L = list(m.layers)
    for n, sub in m.named_modules():
        if type(sub) is torch.nn.InstanceNorm2d:
            why = _norm_ineligible(sub)
        elif _strided_candidate(sub):
            why = _strided_ineligible(sub)
        elif type(sub) is torch.nn.Conv2d:          # behind a ReplicationPad2d: tex_params has checked that
            kind = ops.conv2d_rp_kind(sub.weight.shape)
            why = None
            if sub is L[-1] and kind == kl.RP_STEM7:
                why = f"{sub.in_channels} input channels (conv2d_replicate reads a 7x7 weight with at most 4 as the stem; more than 4)"
            elif kind != kl.RP_STEM7 and sub.out_channels % 4:
                why = f"out_ch {sub.out_channels} (a multiple of 4)" if sub is L[-1] else f"channels {sub.out_channels} (a multiple of 4)"
            elif not ops.conv2d_rp_supported(kind, sub.in_channels, sub.out_channels):
                why = f"channels {sub.in_channels} -> {sub.out_channels} (multiples of 4, at most 1024)"
        else:
            continue
        if why is not None:
            return f"{n}: {why}"
    return None


_TEX_PARTS = ("strided", "norms")


def _fused_tex_plan(m):
    """(convolutions in module order, n_down, n_blocks, n_up, eps) if kpn_res_encoder_* serves this ResBlkEncoder (one that
    _tex_ineligible has passed), else the reason it stays on the per-layer path"""
    _, (ngf, n_down, n_blocks, n_up, out_ch), eps = tex_params(m)
    convs = [c for c in m.modules() if type(c) in (torch.nn.Conv2d, torch.nn.ConvTranspose2d)]
    if any(c.bias is None for c in convs):
        return "a convolution without bias"
    why = ops.res_encoder_refusal(convs[0].in_channels, (ngf, n_down, n_blocks, n_up, out_ch))
    if why is not None:
        return f"the single-operator encoder does not serve it: {why}"
    return convs, n_down, n_blocks, n_up, eps


def install_native_tex(module, fused=False):
    """Opt-in: trains every ResBlkEncoder under ``module`` (``module`` itself included) on the project's kernels.  A ResBlkEncoder whose
    structure is the reference's (src/utils.py:199-259 with ``norm="instance"`` and ``n_upsample`` >= 1: the check of ``tex_params``),
    whose norms have a power of two in 4 .. 1024 channels, whose ``out_ch`` is a multiple of 4 and whose convolutions their kernels
    serve gets ``install_native_strided`` and ``install_native_norms`` on its subtree, and its ``forward`` is rebound to the same walk
    of ``layers``: every ReplicationPad2d + Conv2d pair is torch.ops.kpnerf.conv2d_replicate, every InstanceNorm2d + ReLU pair
    torch.ops.kpnerf.group_norm(relu=True), a ResBlk ``x + group_norm(conv2d_replicate(...), relu=False)`` with the add on torch, and
    the stride-2 and transposed layers run through their rebound modules: no convolution, pad, normalisation or ReLU is left to torch.
    Input that is not a CUDA fp32 (N, 3, H, W) tensor with H and W divisible by 2^n_downsample, or that requires a gradient (the stem
    has no native input gradient), goes to the original forward.  An encoder that fails a check is left alone with its reason, not
    refused.  The module tree, the parameter names and the state_dict are untouched.  Returns {"tex": (served, left), "strided": ...,
    "norms": ...}, the names relative to ``module``.

    ``fused=True``: the rebound forward of every encoder of the reference's structure that kpn_res_encoder_* serves (whether or not the
    per-layer kernels serve each of its layers) is one torch.ops.kpnerf.res_encoder call instead (kpn_res_encoder_forward / _backward): one autograd node per encoder and no aten operator inside it - the norms and the
    ReLUs run in the loads of the convolutions, forward and backward, the residual adds in the kernels - with x, the convolution outputs
    and the ResBlk sums kept for the backward instead of every layer's input and normalised input.  Its forward has the bits of the
    per-layer path.  Such an encoder needs neither of the two installers on its subtree and gets neither.  An encoder that the
    operator does not serve stays on the per-layer path, if that serves it; the report gains "fused": (the names on the operator, {name: reason} of those
    left on the per-layer path).  ``NativeTraining.fused_tex_calls`` counts the operator's calls (``tex_calls`` the per-layer ones)."""
    def make_forward(_prev):
        def forward(self, x):
            nn = torch.nn
            L = list(self.layers)
            f = 1 << sum(type(m) is nn.Conv2d and _pair(m.stride) == (2, 2) for m in L)
            if (not _native_input(x, *self.parameters()) or x.shape[1] != 3 or x.shape[2] % f or x.shape[3] % f
                    or (x.requires_grad and torch.is_grad_enabled())):
                return _prev(x)
            plan = self.__dict__.get("_kpnerf_tex_fused")
            if plan is not None:
                NativeTraining.fused_tex_calls += 1
                convs, n_down, n_blocks, n_up, eps = plan
                return torch.ops.kpnerf.res_encoder(x, [t for c in convs for t in (c.weight, c.bias)], n_down, n_blocks, n_up, eps)
            NativeTraining.tex_calls += 1

            def rp(t, conv):
                return torch.ops.kpnerf.conv2d_replicate(t, conv.weight, conv.bias)

            def inorm(t, norm, relu):
                return torch.ops.kpnerf.group_norm(t, None, None, norm.num_features, norm.eps, relu)

            i = 0
            while i < len(L):
                m = L[i]
                if type(m) is nn.ReplicationPad2d:
                    x, i = rp(x, L[i + 1]), i + 2
                elif type(m) is nn.InstanceNorm2d:              # tex_params has seen the ReLU behind it
                    x, i = inorm(x, m, True), i + 2
                elif type(m).__name__ == "ResBlk":
                    b = m.layers
                    t = inorm(rp(x, b[1]), b[2], True)
                    x, i = x + inorm(rp(t, b[5]), b[6], False), i + 1
                else:                                           # a stride-2 or transposed convolution, rebound
                    x, i = m(x), i + 1
            return x
        return forward

    uninstall_native_tex(module)
    plans = {}

    def ineligible(m, name):
        # the operator first: it serves an encoder whatever the per-layer kernels say of its layers
        if fused:
            why = _tex_structure_error(m)
            if why is not None:
                return why
            plans[name] = _fused_tex_plan(m)
            if not isinstance(plans[name], str):
                return None
        return _tex_ineligible(m, name)

    served, left = _rebind_forward(module, "_kpnerf_tex_saved", lambda m: type(m).__name__ == "ResBlkEncoder", ineligible, make_forward)
    report = {k: ([], {}) for k in _TEX_PARTS}
    subs = dict(module.named_modules())
    if fused:
        report["fused"] = ([], {})
    for name in served:
        if fused:
            if not isinstance(plans[name], str):
                subs[name]._kpnerf_tex_fused = plans[name]
                report["fused"][0].append(name)
                continue
            report["fused"][1][name] = plans[name]
        for part, fn in zip(_TEX_PARTS, (install_native_strided, install_native_norms)):
            s_, l_ = fn(subs[name])
            pre = name + "." if name else ""
            report[part][0].extend(pre + n for n in s_)
            report[part][1].update({pre + n: why for n, why in l_.items()})
    report["tex"] = (served, left)
    return report


def uninstall_native_tex(module):
    """Restores what ``forward`` was on every ResBlkEncoder ``install_native_tex`` rebound, and undoes the two installers on its
    subtree: no attribute it added is left."""
    for m in module.modules():
        if "_kpnerf_tex_saved" in m.__dict__:
            m.__dict__.pop("_kpnerf_tex_fused", None)
            for undo in (uninstall_native_strided, uninstall_native_norms):
                undo(m)
    return _restore_forward(module, "_kpnerf_tex_saved")
