"""PyTorch-facing operators of the gfx950 ray-march library (device tensors in, device tensors out).

Each function mirrors one callable of the reference (names, argument meaning, shapes, error
behaviour) and forwards to the C ABI in include/kpnerf.h on torch's CURRENT HIP stream:

    ray_bbox_intersection  <- KeypointNeRF.ray_bbox_intersection  (reference src/model.py:1178-1237)
    importance_sample      <- KeypointNeRF.importance_sample      (src/model.py:1110-1148)
    rgba2out               <- KeypointNeRF.rgba2out               (src/model.py:1150-1176)
    query                  <- KeypointNeRF.query                  (src/model.py:690-843, eval mode)
    render_rays            <- KeypointNeRF.batch_render_pifu_nerf (src/model.py:942-1108, eval branch)

torch is plumbing here (device memory, streams); the arithmetic is in csrc/*.hip.  Every op raises if
its tensors are not on a HIP device or the library is missing — there is no CPU/eager fallback.
"""
import ctypes
import functools

import numpy as np
import torch

from . import lib as kl
from .weights import CANONICAL_SHAPE, effective_weights, flatten_plain, widen_plain_host

_f32 = torch.float32
_REDUCE_SCRATCH_BYTES = 16392   # include/kpnerf.h, kpn_mse_psnr / kpn_pix_l1_loss: 2048 fp64 block partials and the ticket


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_gpu(t):
    return t.is_cuda


def _dev(t, name, dtype=_f32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not _on_gpu(t):
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); keypointnerf_amd has no CPU path")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------------
class PackedWeights:
    """Hot-path parameters packed for the kernels; built from the reference's state dict / module."""

    def __init__(self, state_dict_or_module, device="cuda", shape=None):
        """shape = (n_kpt, sp_level) of the model the state dict belongs to (None: the shipped 24 / 3): its narrow first layer is
        widened to the kernels' layout on the host (weights.widen_plain_host)."""
        sd = state_dict_or_module.state_dict() if hasattr(state_dict_or_module, "state_dict") else state_dict_or_module
        plain = flatten_plain(effective_weights(sd, shape))
        if shape is not None and tuple(shape) != CANONICAL_SHAPE:
            plain = widen_plain_host(plain, _field_shape(shape, "PackedWeights"))
        packed = self._pack_on_host(plain)
        # the packers' count of weights beyond fp16's range (include/kpnerf.h kpn_packed_f16_range_check).  Nothing to do here:
        # the two-fp16-piece kernels read the same count on the device and leave the work to the fp32-range kernels (range guard)
        self.f16_beyond = int(packed[-4])
        self.tensor = torch.from_numpy(packed).to(device)

    @staticmethod
    def _pack_on_host(plain):
        L = kl.get_library()
        if plain.size != L.kpn_plain_weight_floats():
            raise ValueError("unexpected hot-path parameter count")
        packed = np.zeros(L.kpn_packed_weight_floats(), np.float32)
        L.check(L.kpn_pack_weights(plain.ctypes.data_as(ctypes.c_void_p), packed.ctypes.data_as(ctypes.c_void_p)))
        return packed

    @classmethod
    def wrap(cls, tensor):
        self = cls.__new__(cls)
        self.tensor = tensor
        return self

    @classmethod
    def from_plain(cls, plain, device="cuda"):
        """From the flat effective-parameter vector (weights.flatten_plain / plain_tensor_from_module layout).  A CUDA
        tensor is packed on the device (kpn_pack_weights_device: no host round trip, asynchronous)."""
        L = kl.get_library()
        if isinstance(plain, torch.Tensor) and _on_gpu(plain):
            flat = plain.detach().to(_f32).contiguous()
            if flat.numel() != L.kpn_plain_weight_floats():
                raise ValueError("unexpected hot-path parameter count")
            self = cls.wrap(torch.empty(L.kpn_packed_weight_floats(), dtype=_f32, device=flat.device))
            L.check(L.kpn_pack_weights_device(_p(flat), _p(self.tensor), _stream()))
            self._plain = flat  # keeps the source alive until the stream has consumed it
            return self
        flat = np.ascontiguousarray(plain.detach().float().cpu().numpy() if isinstance(plain, torch.Tensor) else plain, dtype=np.float32)
        return cls.wrap(torch.from_numpy(cls._pack_on_host(flat)).to(device))


def _field_shape(shape, what):
    """(n_kpt, sp_level) checked against the kernels' capacity (KPN_N_KPT, KPN_SP_LEVEL)"""
    n, lv = int(shape[0]), int(shape[1])
    if not (1 <= n <= kl.N_KPT_CAPACITY and 0 <= lv <= kl.SP_LEVEL_CAPACITY):
        raise ValueError(f"{what}: n_kpt must lie in 1..{kl.N_KPT_CAPACITY} and sp_level in 0..{kl.SP_LEVEL_CAPACITY}, got {n} / {lv}")
    return n, lv


def widen_plain(narrow, n_kpt, sp_level):
    """The narrow plain vector of a (n_kpt, sp_level) model -> the kernels' plain vector, one launch (kpn_widen_plain)."""
    L = kl.get_library()
    fs = kl.FieldShape(*_field_shape((n_kpt, sp_level), "widen_plain"))
    flat = _dev(narrow, "narrow").reshape(-1)
    if flat.numel() != L.kpn_plain_weight_floats_shape(ctypes.byref(fs)):
        raise ValueError(f"widen_plain: expected {L.kpn_plain_weight_floats_shape(ctypes.byref(fs))} floats for n_kpt = {n_kpt}, "
                         f"sp_level = {sp_level}, got {flat.numel()}")
    plain = torch.empty(L.kpn_plain_weight_floats(), dtype=_f32, device=flat.device)
    L.check(L.kpn_widen_plain(ctypes.byref(fs), _p(flat), _p(plain), _stream()))
    return plain


def narrow_plain_grad(d_plain, n_kpt, sp_level, out=None, accumulate=False):
    """The adjoint of widen_plain: the gradient of the plain vector -> the gradient of the narrow one (kpn_narrow_plain_grad).
    out: a destination, overwritten or (accumulate=True) added to."""
    L = kl.get_library()
    fs = kl.FieldShape(*_field_shape((n_kpt, sp_level), "narrow_plain_grad"))
    g = _dev(d_plain, "d_plain").reshape(-1)
    if g.numel() != L.kpn_plain_weight_floats():
        raise ValueError("narrow_plain_grad: d_plain has the wrong size")
    n = L.kpn_plain_weight_floats_shape(ctypes.byref(fs))
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs a destination (out)")
        out = torch.empty(n, dtype=_f32, device=g.device)
    elif out.dtype != _f32 or not out.is_contiguous() or out.numel() != n or not _on_gpu(out):
        raise ValueError("narrow_plain_grad: out must be a contiguous float32 GPU tensor of the narrow vector's size")
    L.check(L.kpn_narrow_plain_grad(ctypes.byref(fs), _p(g), _p(out), int(bool(accumulate)), _stream()))
    return out


class PreparedScene:
    """kpn_scene_desc + the prepared (channels-last) device workspace for one set of source views.

    Arguments are the reference's own objects (reference src/model.py:336-355, 653-680):
    img (V,3,H,W); cam dict {KRT,(K),extrin|sp_data['extrin'],width,height,znear,zfar,nml_scale};
    feat_geo [ (V,64,h0,w0), (V,8,h1,w1) ]; feat_tex (V,8,ht,wt); sp_data {kpt3d (1,n,3), extrin (V,4,4)};
    src_foreground_mask (1,V,1,H,W) bool.  n <= 24 keypoints (the model's n_kpt, src/spatial.py:80): the kernels' table holds 24,
    rows n..23 repeat keypoint 0 (kpn_scene_prepare_kpt) and the padded first-layer weights of such a model are zero.
    """

    def __init__(self, img, cam, feat_geo, feat_tex, sp_data, src_foreground_mask, disable_fg_mask=False, sigma=0.1):
        L = kl.get_library()
        self.img = _dev(img, "img")
        V, C, H, W = self.img.shape
        if C != 3:
            raise ValueError("img must be (V,3,H,W)")
        if not isinstance(feat_geo, (list, tuple)) or len(feat_geo) != 2:
            raise ValueError("feat_geo must be the list [ (V,64,h,w), (V,8,h,w) ] of HGFilterV2")
        self.geo0, self.geo1, self.tex = _dev(feat_geo[0], "feat_geo[0]"), _dev(feat_geo[1], "feat_geo[1]"), _dev(feat_tex, "feat_tex")
        if self.geo0.shape[:2] != (V, 64) or self.geo1.shape[:2] != (V, 8) or self.tex.shape[:2] != (V, 8):
            raise ValueError("feature maps must be (V,64,..), (V,8,..), (V,8,..)")
        self.KRT = _dev(cam["KRT"], "cam['KRT']").reshape(V, 4, 4)
        extrin = sp_data["extrin"] if "extrin" in sp_data else cam["extrin"]
        self.extrin = _dev(extrin, "extrin").reshape(V, 4, 4)
        kpt = _dev(sp_data["kpt3d"], "kpt3d")
        n_kpt = kpt.numel() // 3
        if kpt.numel() != 3 * n_kpt or not 1 <= n_kpt <= kl.N_KPT_CAPACITY:
            raise ValueError(f"kpt3d must be (1,n,3) with n in 1..{kl.N_KPT_CAPACITY}: batch size 1 (reference src/model.py:938) and at most "
                             f"the {kl.N_KPT_CAPACITY} keypoints the field kernels hold (configs/zju.json:44), got {tuple(kpt.shape)}")
        self.n_kpt = n_kpt
        self.kpt3d = kpt.reshape(n_kpt, 3)
        if int(cam["width"]) != W or int(cam["height"]) != H:
            raise ValueError("cam width/height must match the source images")
        if disable_fg_mask:
            self.fg = None
        else:
            m = src_foreground_mask
            if not _on_gpu(m):
                raise RuntimeError("src_foreground_mask must live on the GPU")
            self.fg = (m.reshape(V, H, W) != 0).to(torch.uint8).contiguous()
        d = kl.SceneDesc()
        d.n_views, d.src_h, d.src_w = V, H, W
        d.geo0_h, d.geo0_w = self.geo0.shape[-2:]
        d.geo1_h, d.geo1_w = self.geo1.shape[-2:]
        d.tex_h, d.tex_w = self.tex.shape[-2:]
        d.disable_fg_mask = int(bool(disable_fg_mask))
        d.znear, d.zfar = float(cam["znear"]), float(cam["zfar"])
        d.nml_scale, d.sigma = float(cam.get("nml_scale", 100.0)), float(sigma)
        d.KRT, d.extrin, d.kpt3d = self.KRT.data_ptr(), self.extrin.data_ptr(), self.kpt3d.data_ptr()
        d.img, d.geo0, d.geo1, d.tex = self.img.data_ptr(), self.geo0.data_ptr(), self.geo1.data_ptr(), self.tex.data_ptr()
        d.fg_mask = self.fg.data_ptr() if self.fg is not None else None
        self.desc = d
        self.n_views = V
        nbytes = L.kpn_scene_workspace_bytes(ctypes.byref(d))
        if nbytes == 0:
            raise kl.KpnError(L.kpn_last_error().decode())
        self.ws = torch.empty(nbytes // 4, dtype=_f32, device=self.img.device)
        L.check(L.kpn_scene_prepare_kpt(ctypes.byref(d), n_kpt, _p(self.ws), _stream()))

    def as_op_args(self):
        """(scene_ws, scene_dims, scene_scalars) for torch.ops.kpnerf.field_query (keypointnerf_amd/torch_ops.py)."""
        d = self.desc
        return (self.ws, [d.n_views, d.src_h, d.src_w, d.geo0_h, d.geo0_w, d.geo1_h, d.geo1_w, d.tex_h, d.tex_w, d.disable_fg_mask],
                [d.znear, d.zfar, d.nml_scale, d.sigma])


# ------------------------------------------------------------------------------------------------
def ray_bbox_intersection(bounds, orig, direct):
    """bounds (1,2,3), orig (1,1,3), direct (1,R,3) -> near (1,R,1), far (1,R,1), hit (1,R,1) bool."""
    L = kl.get_library()
    b, o, d = _dev(bounds, "bounds").reshape(2, 3), _dev(orig, "orig").reshape(3), _dev(direct, "direct").reshape(-1, 3)
    R = d.shape[0]
    near, far = torch.empty(R, dtype=_f32, device=d.device), torch.empty(R, dtype=_f32, device=d.device)
    hit = torch.empty(R, dtype=torch.uint8, device=d.device)
    L.check(L.kpn_ray_bbox_intersection(_p(b), _p(o), _p(d), R, _p(near), _p(far), _p(hit), _stream()))
    return near.view(1, R, 1), far.view(1, R, 1), hit.view(1, R, 1).bool()


def importance_sample(contrib, z, sample_per_ray, uniform=False, u=None):
    """contrib (B,R,D-2), z (B,R,D-1) -> (B,R,sample_per_ray).  uniform=True uses linspace(0,1,n)
    (reference src/model.py:1126); otherwise `u` (B,R,n) — drawn with torch.rand if not given (:1129)."""
    L = kl.get_library()
    c, zz = _dev(contrib, "contrib"), _dev(z, "z")
    assert c.shape[-1] == zz.shape[-1] - 1  # same assert as the reference, src/model.py:1119
    B, R, Dm2 = c.shape
    n = int(sample_per_ray)
    if uniform:
        uu = None
    else:
        uu = _dev(u, "u").reshape(B * R, n) if u is not None else torch.rand(B * R, n, device=c.device)
    out = torch.empty(B, R, n, dtype=_f32, device=c.device)
    L.check(L.kpn_importance_sample(_p(c), _p(zz), _p(uu), B * R, Dm2, n, _p(out), _stream()))
    return out


class _Rgba2Out(torch.autograd.Function):
    """rgba2out with its hand-written backward (kpn_rgba2out_backward): d_rgba from the upstream gradients of
    color/depth/alpha/sdf; contrib and z carry no gradient, as in the reference (:1038,1118 run under no_grad)."""

    @staticmethod
    def forward(ctx, rgba, z):
        out = _rgba2out_fwd(rgba, z)
        ctx.save_for_backward(rgba.detach(), z.detach())
        ctx.mark_non_differentiable(out[3])
        return out

    @staticmethod
    def backward(ctx, d_color, d_depth, d_alpha, d_contrib, d_sdf):
        return rgba2out_backward(*ctx.saved_tensors, d_color, d_depth, d_alpha, d_sdf), None


def rgba2out_backward(rgba, z, d_color, d_depth, d_alpha, d_sdf):
    """d_rgba from the upstream gradients of rgba2out's color / depth / alpha / sdf, any of them None (kpn_rgba2out_backward)."""
    L = kl.get_library()
    q, zz = _dev(rgba, "rgba"), _dev(z, "z")
    B, R, S = zz.shape
    g = [None if x is None else _dev(x, "grad") for x in (d_color, d_depth, d_alpha, d_sdf)]
    d_rgba = torch.empty_like(q)
    L.check(L.kpn_rgba2out_backward(_p(q), _p(zz), B * R, S, _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), _p(d_rgba), _stream()))
    return d_rgba


def rgba2out(rgba, z):
    """rgba (B,R,S,5), z (B,R,S) -> color (B,R,3), depth (B,R), alpha (B,R), contrib (B,R,S), sdf (B,R).
    Differentiable w.r.t. rgba (hand-written backward kernel)."""
    if torch.is_grad_enabled() and isinstance(rgba, torch.Tensor) and rgba.requires_grad:
        return _Rgba2Out.apply(rgba, z)
    return _rgba2out_fwd(rgba, z)


def _rgba2out_fwd(rgba, z):
    L = kl.get_library()
    q, zz = _dev(rgba, "rgba"), _dev(z, "z")
    B, R, S = zz.shape
    if q.shape != (B, R, S, 5):
        raise ValueError("rgba must be (B,R,S,5)")
    dv = q.device
    color = torch.empty(B, R, 3, dtype=_f32, device=dv)
    depth, alpha, sdf = (torch.empty(B, R, dtype=_f32, device=dv) for _ in range(3))
    contrib = torch.empty(B, R, S, dtype=_f32, device=dv)
    L.check(L.kpn_rgba2out(_p(q), _p(zz), B * R, S, _p(color), _p(depth), _p(alpha), _p(contrib), _p(sdf), _stream()))
    return color, depth, alpha, contrib, sdf


def query(scene, weights, pts, view, mode=0):
    """pts (1,N,3), view (1,N,3) -> out (1,N,5), valid (1,N,1) bool.  mode 0 = KeypointNeRF.query's
    [sdf_raw, rad, rgb]; mode 1 = eval_func(query) = [sigma, sdf, rgb] (reference src/model.py:978-997)."""
    L = kl.get_library()
    p, v = _dev(pts, "pts").reshape(-1, 3), _dev(view, "view").reshape(-1, 3)
    if p.shape != v.shape:
        raise ValueError("pts and view must have the same shape")
    N = p.shape[0]
    out = torch.empty(N, 5, dtype=_f32, device=p.device)
    valid = torch.empty(N, dtype=torch.uint8, device=p.device)
    if N == 0:
        return out.view(1, 0, 5), valid.view(1, 0, 1).bool()
    nb = L.kpn_query_workspace_bytes(N, scene.n_views)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=p.device)
    L.check(L.kpn_query(ctypes.byref(scene.desc), _p(scene.ws), _p(weights.tensor), N, _p(p), _p(v), int(mode), _p(out),
                        _p(valid), _p(ws), nb, _stream()))
    return out.view(1, N, 5), valid.view(1, N, 1).bool()


def _grad_buffers(scene, device, with_tex):
    """zeroed accumulators of a backward call: the flat parameter gradient and the channels-last map gradients"""
    d = scene.desc
    maps = [(d.geo0_h, d.geo0_w, 64), (d.geo1_h, d.geo1_w, 8)] + ([(d.tex_h, d.tex_w, 8)] if with_tex else [])
    return (torch.zeros(kl.get_library().kpn_plain_weight_floats(), dtype=_f32, device=device),
            *(torch.zeros(scene.n_views, h, w, c, dtype=_f32, device=device) for h, w, c in maps))


def _kpt_variant(scene, device, want_kpt):
    """what want_kpt changes in a backward call (the *_kpt entries of include/kpnerf.h): the suffix of the entry points' names, the result
    that follows the others - the zeroed (n_kpt, 3) accumulator of the keypoint gradient as (1, n_kpt, 3) - and the (d_kpt, n_kpt)
    arguments that follow the map gradients"""
    if not want_kpt:
        return "", (), ()
    d_kpt = torch.zeros(scene.n_kpt, 3, dtype=_f32, device=device)
    return "_kpt", (d_kpt.view(1, -1, 3),), (_p(d_kpt), scene.n_kpt)


def _nchw(d_plain, *d_maps):
    """what the backward wrappers return: the map gradients as NCHW views of the channels-last accumulators"""
    return (d_plain, *(m.permute(0, 3, 1, 2) for m in d_maps))


def geo_rows_backward(scene, weights, pts, d_x, keep_mask=0xFFFFFFFF, want_kpt=False):
    """Reverse pass of the per-(point,view) geometry rows (kpn_geo_rows_backward): MLPUNet.layers1 and the
    feat_geo gathers (reference src/utils.py:691-716, src/model.py:763-765).
    pts (1,N,3) or (N,3); d_x (N,V,64) = d loss / d layers1-output.  Returns (d_plain, d_geo0, d_geo1):
    d_plain flat like weights.flatten_plain (feed it to weights.plain_grads_to_state_dict), d_geo* shaped
    like feat_geo[*] (NCHW views of the channels-last accumulators).
    want_kpt: also the gradient with respect to sp_data["kpt3d"] (kpn_geo_rows_backward_kpt; reference src/spatial.py:76-118), as
    (1, n_kpt, 3) after the other results."""
    L = kl.get_library()
    p = _dev(pts, "pts").reshape(-1, 3)
    N, V = p.shape[0], scene.n_views
    g = _dev(d_x, "d_x")
    if tuple(g.shape) != (N, V, 64):
        raise ValueError(f"d_x must be (N, V, 64) = {(N, V, 64)}, got {tuple(g.shape)}")
    d = scene.desc
    d_plain, d_g0, d_g1 = _grad_buffers(scene, p.device, with_tex=False)
    sfx, d_kpt, kpt_args = _kpt_variant(scene, p.device, want_kpt)
    if N > 0:                   # kpn_geo_rows_backward or kpn_geo_rows_backward_kpt, each with its _workspace_bytes
        nb = getattr(L, "kpn_geo_rows_backward_workspace_bytes" + sfx)(N, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=p.device)
        L.check(getattr(L, "kpn_geo_rows_backward" + sfx)(ctypes.byref(d), _p(scene.ws), _p(weights.tensor), N, _p(p), int(keep_mask) & 0xFFFFFFFF,
                                                          _p(g), _p(d_plain), _p(d_g0), _p(d_g1), *kpt_args, _p(ws), nb, _stream()))
    return _nchw(d_plain, d_g0, d_g1) + d_kpt


def query_backward_geometry(scene, weights, pts, d_out, mode=1, keep_mask=0xFFFFFFFF, noise=None, noise_std=0.0):
    """Reverse pass of the field evaluation w.r.t. its two geometry outputs (kpn_query_backward_geometry): pooling,
    layers2, layers1 and the feat_geo gathers.  d_out (N,5) or (1,N,5): columns 0,1 are propagated (mode 1:
    [sigma, sdf] of eval_func, the training path; mode 0: query's raw [sdf_raw, rad]); the colour columns are not yet.
    Returns (d_plain, d_geo0, d_geo1) like geo_rows_backward."""
    L = kl.get_library()
    p = _dev(pts, "pts").reshape(-1, 3)
    N, V = p.shape[0], scene.n_views
    g = _dev(d_out, "d_out").reshape(-1, 5)
    if g.shape[0] != N:
        raise ValueError(f"d_out must have {N} rows")
    nz = None if noise is None else _dev(noise, "noise").reshape(-1)
    if nz is not None and nz.shape[0] != N:
        raise ValueError("noise must have one value per point")
    d = scene.desc
    d_plain, d_g0, d_g1 = _grad_buffers(scene, p.device, with_tex=False)
    if N > 0:
        nb = L.kpn_query_backward_geometry_workspace_bytes(N, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=p.device)
        L.check(L.kpn_query_backward_geometry(ctypes.byref(d), _p(scene.ws), _p(weights.tensor), N, _p(p), int(mode),
                                              int(keep_mask) & 0xFFFFFFFF, None if nz is None else _p(nz), float(noise_std), _p(g),
                                              _p(d_plain), _p(d_g0), _p(d_g1), _p(ws), nb, _stream()))
    return _nchw(d_plain, d_g0, d_g1)


def query_backward(scene, weights, pts, view, d_out, mode=1, keep_mask=0xFFFFFFFF, noise=None, noise_std=0.0, want_kpt=False):
    """Reverse pass of the whole field evaluation incl. the colour head (kpn_query_backward):
    what loss.backward() does for KeypointNeRF.query + eval_func in training_step (reference src/model.py:128-155).
    pts, view (N,3)/(1,N,3); d_out (N,5) = d loss / d [sigma, sdf, r, g, b] (mode 1) or d [sdf_raw, rad, r, g, b] (mode 0).
    Returns (d_plain, d_geo0, d_geo1, d_tex): flat effective-parameter gradient (weights.plain_grads_to_state_dict maps it
    to weight_g / weight_v / bias / ani_al) and the feature-map gradients shaped like feat_geo[0], feat_geo[1], feat_tex.
    want_kpt: also d loss / d sp_data["kpt3d"] as (1, n_kpt, 3), last (kpn_query_backward_kpt)."""
    L = kl.get_library()
    p, vw = _dev(pts, "pts").reshape(-1, 3), _dev(view, "view").reshape(-1, 3)
    N, V = p.shape[0], scene.n_views
    g = _dev(d_out, "d_out").reshape(-1, 5)
    if g.shape[0] != N or vw.shape[0] != N:
        raise ValueError(f"view and d_out must have {N} rows")
    nz = None if noise is None else _dev(noise, "noise").reshape(-1)
    if nz is not None and nz.shape[0] != N:
        raise ValueError("noise must have one value per point")
    d = scene.desc
    d_plain, d_g0, d_g1, d_tx = _grad_buffers(scene, p.device, with_tex=True)
    sfx, d_kpt, kpt_args = _kpt_variant(scene, p.device, want_kpt)
    if N > 0:                   # kpn_query_backward or kpn_query_backward_kpt, each with its _workspace_bytes
        nb = getattr(L, "kpn_query_backward_workspace_bytes" + sfx)(N, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=p.device)
        L.check(getattr(L, "kpn_query_backward" + sfx)(ctypes.byref(d), _p(scene.ws), _p(weights.tensor), N, _p(p), _p(vw), int(mode),
                                                       int(keep_mask) & 0xFFFFFFFF, _p(nz), float(noise_std), _p(g), _p(d_plain),
                                                       _p(d_g0), _p(d_g1), _p(d_tx), *kpt_args, _p(ws), nb, _stream()))
    return _nchw(d_plain, d_g0, d_g1, d_tx) + d_kpt


class RenderPlan:
    """Pre-allocated outputs + workspace for repeated renders of one pixel grid (no per-call allocation)."""

    def __init__(self, scene, grid, n_coarse, n_fine, fine=True, chunk_rays=0, device=None, rows_kernel=None, fuse_kernel=None):
        """rows_kernel / fuse_kernel: the kernels of the calls made with THIS plan ("f32" / "bf16x3" / "f16x2", "f32" / "f16x2";
        None = the process-wide selection of set_geo_rows_mode / set_fuse_mode) — include/kpnerf.h kpn_render_args."""
        L = kl.get_library()
        # grid = (x0, y0, step, nx, ny) as the reference's strided grids, or (x0, y0, step, nx, ny, step_y): rows advance by step_y
        # (a frame's rows dealt round-robin to the ranks of a render job: parallel.rows_of_rank)
        x0, y0, step, nx, ny = (int(g) for g in grid[:5])
        step_y = int(grid[5]) if len(grid) > 5 else 0
        dv = device or scene.ws.device
        self.grid, self.fine = (x0, y0, step, nx, ny, step_y), bool(fine)
        self.out = {"tex_fg": torch.empty(1, 3, ny, nx, dtype=_f32, device=dv), "depth": torch.empty(1, ny, nx, dtype=_f32, device=dv),
                    "alpha": torch.empty(1, ny, nx, dtype=_f32, device=dv)}
        if fine:
            self.out.update({"tex_fg_fine": torch.empty(1, 3, ny, nx, dtype=_f32, device=dv),
                             "depth_fine": torch.empty(1, ny, nx, dtype=_f32, device=dv),
                             "alpha_fine": torch.empty(1, ny, nx, dtype=_f32, device=dv),
                             "sdf": torch.empty(1, ny, nx, dtype=_f32, device=dv)})
        a = kl.RenderArgs()
        a.x0, a.y0, a.step, a.nx, a.ny, a.step_y = x0, y0, step, nx, ny, step_y
        a.n_coarse, a.n_fine, a.fine, a.chunk_rays = int(n_coarse), int(n_fine), int(bool(fine)), int(chunk_rays)
        a.rows_kernel = {None: 0, "f32": 1, "bf16x3": 2, "f16x2": 3}[rows_kernel]
        a.fuse_kernel = {None: 0, "f32": 1, "f16x2": 2}[fuse_kernel]
        for k, v in self.out.items():
            setattr(a, k, v.data_ptr())
        self.args = a
        # K/RT/bounds pointers are filled per call; sizes do not depend on them
        dummy = torch.zeros(16, dtype=_f32, device=dv)
        a.K = a.RT = a.bounds = dummy.data_ptr()
        self.nbytes = L.kpn_render_workspace_bytes(ctypes.byref(scene.desc), ctypes.byref(a))
        if self.nbytes == 0:
            raise kl.KpnError(L.kpn_last_error().decode())
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dv)

    def n_rays(self):
        return self.grid[3] * self.grid[4]


def _set_camera(a, cam_tar, bounds):
    """Fills the target-camera fields of a RenderArgs; returns the three small tensors it points to (keep them alive)."""
    K, RT, b = _dev(cam_tar["K"], "cam_tar['K']").reshape(4, 4), _dev(cam_tar["RT"], "cam_tar['RT']").reshape(4, 4), _dev(bounds, "bounds").reshape(2, 3)
    a.K, a.RT, a.bounds = K.data_ptr(), RT.data_ptr(), b.data_ptr()
    a.znear, a.zfar = float(cam_tar["znear"]), float(cam_tar["zfar"])
    return K, RT, b


def _keep_bits(k):
    """a view-dropout argument as the bit mask the C ABI takes: an int is one already, a (V,) 0/1 vector sets bit i for view i"""
    return int(k) if isinstance(k, int) else int(sum(1 << i for i, x in enumerate(k.reshape(-1).tolist()) if x > 0.5))


def _train_args(R, pix, u_coarse, u_fine, keep_coarse, keep_fine, noise_coarse, noise_fine, rand_noise_std, n_coarse, n_fine):
    """kpn_train_args of the training render and its backward -> (TrainArgs, the tensors it points to)"""
    px = pix.to(torch.int32).contiguous()
    if not _on_gpu(px):
        raise RuntimeError("pix must live on the GPU")
    uc, uf = _dev(u_coarse, "u_coarse").reshape(R, n_coarse), _dev(u_fine, "u_fine").reshape(R, n_fine)
    nc = _dev(noise_coarse, "noise_coarse").reshape(-1) if noise_coarse is not None else None
    nf = _dev(noise_fine, "noise_fine").reshape(-1) if noise_fine is not None else None
    t = kl.TrainArgs()
    t.pix, t.u_coarse, t.u_fine = px.data_ptr(), uc.data_ptr(), uf.data_ptr()
    t.noise_coarse, t.noise_fine = (None if v is None else v.data_ptr() for v in (nc, nf))
    t.keep_coarse, t.keep_fine, t.rand_noise_std = _keep_bits(keep_coarse), _keep_bits(keep_fine), float(rand_noise_std)
    return t, (px, uc, uf, nc, nf)


def render_rays(scene, weights, cam_tar, bounds, grid=None, n_coarse=64, n_fine=64, fine=True, chunk_rays=0, plan=None, stages=False):
    """Eval-mode batch_render_pifu_nerf for the pixel grid (x0, y0, step, nx, ny) of the target camera
    cam_tar {K (1,4,4), RT (1,4,4), znear, zfar}.  Returns the reference's out dict (B=1):
    tex_fg (1,3,ny,nx), depth/alpha (1,ny,nx) [, tex_fg_fine, depth_fine, alpha_fine, sdf].
    stages=True: -> (out, {dirs (R,3), cam_pos (3), z_coarse (R,Sc), rgba_coarse (R,Sc,5) [, z_fine (R,Sc+Sf), rgba_fine (R,Sc+Sf,5)]}), the rays, the per-sample depths
    and eval_func'ed field values of the call in ray order (kpn_render_stages: the conditional parity check of tests/parity_gate.py)."""
    L = kl.get_library()
    if plan is None:
        plan = RenderPlan(scene, grid, n_coarse, n_fine, fine, chunk_rays)
    a = plan.args
    cam = _set_camera(a, cam_tar, bounds)
    st = None
    if stages:
        R, Sc, Sf = plan.n_rays(), int(a.n_coarse), int(a.n_fine) if plan.fine else 0
        st = {"z_coarse": torch.empty(R, Sc, dtype=_f32, device=plan.ws.device), "rgba_coarse": torch.empty(R, Sc, 5, dtype=_f32, device=plan.ws.device),
              "dirs": torch.empty(R, 3, dtype=_f32, device=plan.ws.device), "cam_pos": torch.empty(3, dtype=_f32, device=plan.ws.device)}
        if plan.fine:
            st.update({"z_fine": torch.empty(R, Sc + Sf, dtype=_f32, device=plan.ws.device),
                       "rgba_fine": torch.empty(R, Sc + Sf, 5, dtype=_f32, device=plan.ws.device)})
        cst = kl.RenderStages()
        for k, v in st.items():
            setattr(cst, k, v.data_ptr())
        a.stages = ctypes.pointer(cst)
    try:
        L.check(L.kpn_render_rays(ctypes.byref(scene.desc), _p(scene.ws), _p(weights.tensor), ctypes.byref(a), _p(plan.ws),
                                  plan.nbytes, _stream()))
    finally:
        if stages:
            a.stages = ctypes.POINTER(kl.RenderStages)()
    plan._keep = cam  # keep the small tensors alive until the stream has consumed them
    return (plan.out, st) if stages else plan.out


def render_rays_train(scene, weights, cam_tar, bounds, pix, u_coarse, u_fine, keep_coarse, keep_fine, noise_coarse=None,
                      noise_fine=None, rand_noise_std=0.0, n_coarse=64, n_fine=64, chunk_rays=0, keep_state=False):
    """TRAIN branch of batch_render_pifu_nerf, forward only, with the random draws passed in (reference
    src/model.py:1008-1017,1049-1053,993-994,742-748,1129): pix (R,2) int32 patch pixels (x,y); u_coarse (R,Sc);
    u_fine (R,Sf); keep_* = (V,) 0/1 view-dropout vectors (or bit masks) of the coarse / fine query; noise_* flat
    density noise.  Returns the out dict with (1,3,R) / (1,R) tensors in patch order (reshape to (out_h,out_w))."""
    L = kl.get_library()
    R = pix.shape[0]
    t, draws = _train_args(R, pix, u_coarse, u_fine, keep_coarse, keep_fine, noise_coarse, noise_fine, rand_noise_std, n_coarse, n_fine)
    plan = RenderPlan(scene, (0, 0, 1, R, 1), n_coarse, n_fine, fine=True, chunk_rays=chunk_rays)
    a = plan.args
    cam = _set_camera(a, cam_tar, bounds)  # cam and draws are not read again: they keep the tensors behind a and t alive for the calls below
    state = None
    if keep_state:
        nb = L.kpn_render_rays_train_state_bytes(ctypes.byref(scene.desc), ctypes.byref(a))
        if nb == 0:
            raise kl.KpnError("bad render arguments: " + L.kpn_last_error().decode())
        state = torch.empty(nb, dtype=torch.uint8, device=pix.device)
        L.check(L.kpn_render_rays_train_keep(ctypes.byref(scene.desc), _p(scene.ws), _p(weights.tensor), ctypes.byref(a),
                                             ctypes.byref(t), _p(state), nb, _stream()))
    else:
        L.check(L.kpn_render_rays_train(ctypes.byref(scene.desc), _p(scene.ws), _p(weights.tensor), ctypes.byref(a), ctypes.byref(t),
                                        _p(plan.ws), plan.nbytes, _stream()))
    # no host sync: every launch above is on torch's current stream, and the caching allocator hands a freed block to
    # later work of the SAME stream only, so the argument tensors may be released as soon as this returns
    out = {k: v.reshape(1, *v.shape[1:-2], R) if v.dim() == 4 else v.reshape(1, R) for k, v in plan.out.items()}
    return (out, state) if keep_state else out


def render_rays_train_backward(scene, weights, cam_tar, bounds, pix, u_coarse, u_fine, keep_coarse, keep_fine, grads,
                               noise_coarse=None, noise_fine=None, rand_noise_std=0.0, n_coarse=64, n_fine=64, chunk_rays=0,
                               state=None, want_kpt=False):
    """loss.backward() through render_rays_train (kpn_render_rays_train_backward): `grads` maps output names
    ('tex_fg', 'depth', 'alpha', 'tex_fg_fine', 'depth_fine', 'alpha_fine', 'sdf') to the gradients of those outputs,
    shaped like them ((1,3,R) / (1,R)); missing keys are zero.  Same other arguments as the forward call.
    `state`: the tensor render_rays_train(..., keep_state=True) returned for the SAME arguments (kpn_render_rays_train_
    backward_kept: the forward is not repeated).  Returns (d_plain, d_geo0, d_geo1, d_tex) as ops.query_backward.
    want_kpt: also d loss / d sp_data["kpt3d"] as (1, n_kpt, 3), last (kpn_render_rays_train_backward[_kept]_kpt): the coarse and the
    fine pass both add to it."""
    L = kl.get_library()
    R = pix.shape[0]
    t, draws = _train_args(R, pix, u_coarse, u_fine, keep_coarse, keep_fine, noise_coarse, noise_fine, rand_noise_std, n_coarse, n_fine)
    a = kl.RenderArgs()
    cam = _set_camera(a, cam_tar, bounds)  # cam and draws are not read again: they keep the tensors behind a and t alive for the calls below
    a.x0, a.y0, a.step, a.nx, a.ny = 0, 0, 1, R, 1
    a.n_coarse, a.n_fine, a.fine, a.chunk_rays = int(n_coarse), int(n_fine), 1, int(chunk_rays)
    g, keep_alive = kl.RenderGrads(), []
    for name in ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf"):
        if grads.get(name) is not None:
            gt = _dev(grads[name], "grads['%s']" % name).reshape(-1)
            if gt.numel() != (3 * R if name.startswith("tex") else R):
                raise ValueError(f"grads['{name}'] has the wrong size")
            keep_alive.append(gt)
            setattr(g, "d_" + name, gt.data_ptr())
    d = scene.desc
    dv = pix.device
    d_plain, d_g0, d_g1, d_tx = _grad_buffers(scene, dv, with_tex=True)
    sfx, d_kpt, kpt_args = _kpt_variant(scene, dv, want_kpt)
    nb = getattr(L, "kpn_render_rays_train_backward_workspace_bytes" + sfx)(ctypes.byref(d), ctypes.byref(a))
    if nb == 0:
        raise kl.KpnError("bad render arguments: " + L.kpn_last_error().decode())
    ws = torch.empty(nb, dtype=torch.uint8, device=dv)
    # one of kpn_render_rays_train_backward, kpn_render_rays_train_backward_kpt, kpn_render_rays_train_backward_kept and
    # kpn_render_rays_train_backward_kept_kpt; the _kept entries take (state, state_bytes) in front of the workspace
    kept = state is not None and state.numel() > 0
    backward = getattr(L, "kpn_render_rays_train_backward" + ("_kept" if kept else "") + sfx)
    L.check(backward(ctypes.byref(d), _p(scene.ws), _p(weights.tensor), ctypes.byref(a), ctypes.byref(t), ctypes.byref(g), _p(d_plain),
                     _p(d_g0), _p(d_g1), _p(d_tx), *kpt_args, *((_p(state), state.numel()) if kept else ()), _p(ws), nb, _stream()))
    # no host sync (stream-ordered reuse of freed blocks, see render_rays_train)
    return _nchw(d_plain, d_g0, d_g1, d_tx) + d_kpt


def set_geo_rows_mode(mode):
    """Rows kernel of the field's first MLP (kpn_set_geo_rows_mode): 3 (default) = two fp16 pieces per operand on the fp16 MFMA,
    2 = three bf16 pieces on the bf16 MFMA (fp32's exponent range), both two tiles per wave and one wave per SIMD with fp32-class
    results; 0 = fp32 MFMA.  (1, the earlier one-tile split-bf16 kernel, is not part of the shipped library: DESIGN.md 9.2.)"""
    L = kl.get_library()
    L.check(L.kpn_set_geo_rows_mode(int(mode)))


def set_fuse_mode(mode):
    """Per-point kernel (kpn_set_fuse_mode): 1 (default) = weights as two fp16 pieces on the fp16 MFMA; 0 = fp32 MFMA."""
    L = kl.get_library()
    L.check(L.kpn_set_fuse_mode(int(mode)))


def get_fuse_mode():
    return int(kl.get_library().kpn_get_fuse_mode())


def set_density_first(mode):
    """Render passes: density of every point in the hull first, colour head for the points with relu(rad) > 0 only
    (kpn_set_density_first, include/kpnerf.h): 0 = never, 1 = always, 2 = auto (default); frames bit-identical in every mode."""
    kl.get_library().check(kl.get_library().kpn_set_density_first(int(mode)))


def get_density_first():
    return int(kl.get_library().kpn_get_density_first())


def set_range_guard(on):
    """The range guard of the two-fp16-piece kernels (include/kpnerf.h kpn_set_range_guard): on by default."""
    kl.get_library().check(kl.get_library().kpn_set_range_guard(int(bool(on))))


def range_guard_count():
    """Batches of rows the fp32-range kernels evaluated again since the library was loaded (synchronises the current stream):
    0 = every pass ran on the default (two-fp16-piece) kernels."""
    L = kl.get_library()
    n = ctypes.c_int64(0)
    L.check(L.kpn_range_guard_count(_stream(), ctypes.byref(n)))
    return int(n.value)


def packed_f16_range_check(packed):
    """Number of packed layers1 weights that fp16 cannot hold (rows mode 3 needs 0); synchronises the current stream."""
    L = kl.get_library()
    beyond = ctypes.c_int32(-1)
    L.check(L.kpn_packed_f16_range_check(packed.data_ptr(), _stream(), ctypes.byref(beyond)))
    return int(beyond.value)


def get_geo_rows_mode():
    return int(kl.get_library().kpn_get_geo_rows_mode())


def frame_to_rgb8(img, bgr=False):
    """(3,H,W) or (1,3,H,W) fp32 -> (H,W,3) uint8 on the device: clamp to [0,1] (_arrange_nerf_images, reference
    src/model.py:427-430), x255 and truncate (`.astype(np.uint8)`, :496), optional B,G,R order for cv2.imwrite (:222)."""
    L = kl.get_library()
    x = _dev(img, "img")
    x = x.reshape(3, *x.shape[-2:])
    H, W = x.shape[-2:]
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=x.device)
    L.check(L.kpn_frame_to_rgb8(_p(x), H, W, int(bool(bgr)), _p(out), _stream()))
    return out


def mse_psnr(pred, gt):
    """ZJUEvaluator.compute_score's mse and psnr (reference src/zju_evaluator.py:16-19,63-64) without leaving the
    device: returns a (2,) float64 tensor [mse, psnr]."""
    L = kl.get_library()
    a, b = _dev(pred, "pred"), _dev(gt, "gt")
    if a.shape != b.shape:
        raise ValueError("pred and gt must have the same shape")
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    scratch = torch.empty(_REDUCE_SCRATCH_BYTES, dtype=torch.uint8, device=a.device)
    L.check(L.kpn_mse_psnr(_p(a), _p(b), a.numel(), _p(out), _p(scratch), _stream()))
    return out


def pix_l1_loss(src, tar, lam, want_grad=True):
    """pix_loss(src, tar, {"l1": lam})["l1"] of the reference (src/utils.py:164-168) and d loss / d src: returns
    (loss: 0-dim device tensor, d_src: tensor like src or None)."""
    L = kl.get_library()
    a, b = _dev(src, "src"), _dev(tar, "tar")
    if a.shape != b.shape:
        raise ValueError("src and tar must have the same shape")
    loss = torch.empty(1, dtype=_f32, device=a.device)
    d = torch.empty_like(a) if want_grad else None
    scratch = torch.empty(_REDUCE_SCRATCH_BYTES, dtype=torch.uint8, device=a.device)
    L.check(L.kpn_pix_l1_loss(_p(a), _p(b), a.numel(), float(lam), _p(loss), _p(d), _p(scratch), _stream()))
    return loss.reshape(()), d


_TRAIN_LOSS_WS = {}   # (device, stream handle) -> workspace whose ticket the kernel has left at zero


def train_loss(tex, tex_fine, tar, alpha, alpha_fine, tar_alpha, weights, want_grad=True):
    """The pixel and mask terms of compute_error_nerf (reference src/utils.py:108-171) and their seed gradients in one launch
    (kpn_train_loss).  tex / tex_fine / tar: 3n floats, alpha / alpha_fine / tar_alpha: n floats, any but tar may be None;
    weights = (lambda_l1_c, lambda_l1, lambda_l2, lambda_lp, lambda_mloss).  Returns (terms (6,): e_pix_c, e_pix_l1, e_pix_l2,
    e_pix_lp, mask_loss_c, mask_loss_f, already weighted; d_tex like tex; d_tex_fine (3, *tex_fine.shape): the l1 / l2 / lp
    gradients apart; d_alpha; d_alpha_fine) — a gradient is None without its input or with want_grad=False, and the part of a
    skipped term (weight <= 0, missing input) is left UNWRITTEN."""
    L = kl.get_library()
    t = _dev(tar, "tar")
    if t.numel() == 0 or t.numel() % 3:
        raise ValueError("tar must hold 3 n floats")
    n = t.numel() // 3
    ins = [None if v is None else _dev(v, name) for v, name in ((tex, "tex"), (tex_fine, "tex_fine"), (alpha, "alpha"),
                                                                (alpha_fine, "alpha_fine"), (tar_alpha, "tar_alpha"))]
    for v, name, want in zip(ins, ("tex", "tex_fine", "alpha", "alpha_fine", "tar_alpha"), (3 * n, 3 * n, n, n, n)):
        if v is not None and v.numel() != want:
            raise ValueError(f"{name} has {v.numel()} elements, expected {want}")
    x, xf, a, af, ta = ins
    if len(weights) != 5:
        raise ValueError("weights = (l1_c, l1, l2, lp, mloss)")
    terms = torch.empty(6, dtype=_f32, device=t.device)
    g = lambda v, *lead: torch.empty(*lead, *v.shape, dtype=_f32, device=t.device) if (want_grad and v is not None) else None
    d_x, d_xf, d_a, d_af = g(x), g(xf, 3), g(a), g(af)
    stream = _stream()
    # the kernel leaves its ticket at zero, so a workspace is zeroed only before its first use; per stream, because calls that
    # share one must be ordered.  Under graph capture the workspace is the capture's own (the pool's memory is not ours to keep).
    capturing = t.is_cuda and torch.cuda.is_current_stream_capturing()
    key = (t.device, 0 if stream is None else (stream.value or 0))     # c_void_p(0).value is None: the default stream is 0
    ws = None if capturing else _TRAIN_LOSS_WS.get(key)
    nb = L.kpn_train_loss_workspace_bytes(n)
    fresh = ws is None or ws.numel() < nb
    if fresh:
        ws = torch.empty(nb, dtype=torch.uint8, device=t.device)
    args = kl.TrainLossArgs(tex=_p(x), tex_fine=_p(xf), tar=_p(t), alpha=_p(a), alpha_fine=_p(af), tar_alpha=_p(ta), n=n,
                            l1_c=float(weights[0]), l1=float(weights[1]), l2=float(weights[2]), lp=float(weights[3]),
                            mloss=float(weights[4]), reset_ticket=int(fresh), terms=_p(terms), d_tex=_p(d_x), d_tex_fine=_p(d_xf),
                            d_alpha=_p(d_a), d_alpha_fine=_p(d_af))
    rc = L.kpn_train_loss(ctypes.byref(args), _p(ws), stream)
    if rc != 0:
        _TRAIN_LOSS_WS.pop(key, None)
    L.check(rc)
    if not capturing:
        _TRAIN_LOSS_WS[key] = ws
    return terms, d_x, d_xf, d_a, d_af


def _hot_layout(shape=None):
    """per slot of the 44-tensor list (weights.hot_tensor_names): (kpn_param_table field, layer index or None, shape); shape =
    (n_kpt, sp_level) of the model (None: 24 / 3) sizes the first layer's weight_v"""
    from .synthetic import HOTPATH_LAYERS, hotpath_layers
    slots = []
    for l, (_, _, (o, i), wn) in enumerate(HOTPATH_LAYERS if shape is None else hotpath_layers(*shape)):
        if wn:
            slots.append(("g", l, (o, 1)))
        slots += [("v_or_w", l, (o, i)), ("b", l, (o,))]
    return slots + [("ani_al", None, ())]


def _param_table(tensors, what, shape=None):
    """kpn_param_table over a 44-tensor list in weights.hot_tensor_names order; an entry of `tensors` may be None (a NULL slot)"""
    slots = _hot_layout(shape)
    if len(tensors) != len(slots):
        raise ValueError(f"{what}: expected {len(slots)} tensors (weights.hot_tensor_names), got {len(tensors)}")
    table = kl.ParamTable()
    for t, (field, l, shape) in zip(tensors, slots):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not _on_gpu(t):
            raise RuntimeError(f"{what} must be GPU tensors; keypointnerf_amd has no CPU path")
        if t.dtype != _f32 or not t.is_contiguous() or t.numel() != int(np.prod(shape, dtype=np.int64)):
            raise ValueError(f"{what}: slot {field}[{l}] must be contiguous float32 with {shape} elements, got {t.dtype} {tuple(t.shape)}")
        if l is None:
            table.ani_al = t.data_ptr()
        else:
            getattr(table, field)[l] = t.data_ptr()
    return table


def fold_params(tensors, shape=None):
    """The live hot-path tensors (weights.hot_tensors) -> (plain, norms): the flat effective-parameter vector of
    weights.flatten_plain's layout — weight-norm folded (torch._weight_norm(v, g, 0), reference src/utils.py:542-543), everything
    else copied — and the side buffer fold_params_backward needs, in one launch (kpn_fold_params).  shape = (n_kpt, sp_level) of
    the model (None: 24 / 3): the first layer's weight_v is then the narrow tensor, plain stays the kernels' 24 / 3 vector
    (kpn_fold_params_shape, still one launch)."""
    L = kl.get_library()
    tensors = [t.detach() for t in tensors]
    if shape is not None:
        shape = _field_shape(shape, "fold_params")
    table = _param_table(tensors, "fold_params tensors", shape)
    dev = tensors[0].device
    plain = torch.empty(L.kpn_plain_weight_floats(), dtype=_f32, device=dev)
    norms = torch.empty(L.kpn_fold_norm_floats() // 2, dtype=torch.float64, device=dev).view(_f32)     # 8-byte aligned
    if shape is None:
        L.check(L.kpn_fold_params(ctypes.byref(table), _p(plain), _p(norms), _stream()))
    else:
        L.check(L.kpn_fold_params_shape(ctypes.byref(kl.FieldShape(*shape)), ctypes.byref(table), _p(plain), _p(norms), _stream()))
    return plain, norms


def fold_params_backward(tensors, norms, d_plain, out=None, accumulate=False, shape=None):
    """d_plain -> the gradients of the 44 tensors in one launch (kpn_fold_params_backward).  out=None: returns new tensors.  out = a 44-list of destinations (None entries are skipped): written in place — overwritten, or added to with
    accumulate=True (.grad's semantics) — and returned."""
    L = kl.get_library()
    tensors = [t.detach() for t in tensors]
    if shape is not None:
        shape = _field_shape(shape, "fold_params_backward")
    table = _param_table(tensors, "fold_params tensors", shape)
    g = _dev(d_plain, "d_plain").reshape(-1)
    if g.numel() != L.kpn_plain_weight_floats() or norms.numel() != L.kpn_fold_norm_floats():
        raise ValueError("d_plain / norms have the wrong size")
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs destinations (out)")
        out = [torch.empty_like(t) for t in tensors]      # separate allocations: the outputs of a custom operator may not alias
    grads = _param_table([None if t is None else t.detach() for t in out], "fold_params gradients", shape)
    if shape is None:
        L.check(L.kpn_fold_params_backward(ctypes.byref(table), _p(norms), _p(g), ctypes.byref(grads), int(bool(accumulate)), _stream()))
    else:
        L.check(L.kpn_fold_params_backward_shape(ctypes.byref(kl.FieldShape(*shape)), ctypes.byref(table), _p(norms), _p(g),
                                                 ctypes.byref(grads), int(bool(accumulate)), _stream()))
    return out


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1, beta2, eps, weight_decay):
    """One torch.optim.Adam step (amsgrad=False, maximize=False) of every listed tensor, in place, in one launch per 64 tensors
    (kpn_adam_step).  step: the step number of this update (>= 1), a host integer: nothing is read back from the device.  The
    parameters' version counters are moved, as an in-place torch operation would move them."""
    L = kl.get_library()
    n = len(params)
    if not (n == len(grads) == len(exp_avgs) == len(exp_avg_sqs)) or n == 0:
        raise ValueError("adam_step needs as many grads, exp_avgs and exp_avg_sqs as params (at least one)")
    segs = (kl.AdamSegment * n)()
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        for t, name in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            if not _on_gpu(t):
                raise RuntimeError(f"adam_step: {name} must live on the GPU; keypointnerf_amd has no CPU path")
            if t.dtype != _f32 or not t.is_contiguous() or t.numel() != p.numel():
                raise ValueError(f"adam_step: {name} must be contiguous float32 of the parameter's size")
        segs[i].param, segs[i].grad, segs[i].exp_avg, segs[i].exp_avg_sq, segs[i].count = (p.data_ptr(), g.data_ptr(), m.data_ptr(),
                                                                                         v.data_ptr(), p.numel())
    args = kl.AdamArgs(segments_host=segs, n_segments=n, step=int(step), lr=float(lr), beta1=float(beta1), beta2=float(beta2),
                       eps=float(eps), weight_decay=float(weight_decay))
    L.check(L.kpn_adam_step(ctypes.byref(args), _stream()))
    torch.autograd.graph.increment_version(list(params))


def vgg_pack(plain):
    """Packs the nine convolutions of vgg19.features[0:21] (flat device fp32: each OIHW weight then its bias, in features
    order; vgg.plain_from_module) on the device into the layout kpn_vgg_loss reads (reference src/utils.py:750-805)."""
    L = kl.get_library()
    w = _dev(plain, "plain").reshape(-1)
    if w.numel() != L.kpn_vgg_plain_floats():
        raise ValueError(f"expected {L.kpn_vgg_plain_floats()} VGG parameters, got {w.numel()}")
    packed = torch.empty(L.kpn_vgg_packed_floats(), dtype=_f32, device=w.device)
    L.check(L.kpn_vgg_pack_device(_p(w), _p(packed), _stream()))
    return packed


def vgg_loss(x, y, packed, mean, std, tap_w, lam=1.0, want_grad=True, want_stages=False):
    """VGGLoss.forward(x, y) of the reference (src/utils.py:795-805) times lam, and d loss / d x (y detached, VGG frozen).
    x, y: (B, 3, H, W) device fp32; packed: vgg_pack(...); mean, std (3 floats), tap_w (4 floats): VGGLoss.normalize and
    VGGLoss.weights.  Returns (loss: 0-dim tensor, d_x like x or None, stages or None); stages (kpn_vgg_stage_floats, flat):
    the post-ReLU output of every convolution for x and y (include/kpnerf.h)."""
    L = kl.get_library()
    a, b = _dev(x, "x"), _dev(y, "y")
    if a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError(f"x and y must both be (B, 3, H, W), got {tuple(a.shape)} and {tuple(b.shape)}")
    B, _, H, W = a.shape
    nb = L.kpn_vgg_workspace_bytes(B, H, W)
    if nb == 0:
        raise ValueError(f"VGG loss needs H, W >= 8 (got {H} x {W})")
    hmean, hstd, hw = (np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)) for v in (mean, std, tap_w))
    if hmean.size != 3 or hstd.size != 3 or hw.size != 4:
        raise ValueError("mean / std need 3 values, tap_w 4")
    loss = torch.empty(1, dtype=_f32, device=a.device)
    d = torch.empty_like(a) if want_grad else None
    st = torch.empty(L.kpn_vgg_stage_floats(B, H, W), dtype=_f32, device=a.device) if want_stages else None
    ws = torch.empty(nb, dtype=torch.uint8, device=a.device)
    L.check(L.kpn_vgg_loss(_p(a), _p(b), B, H, W, _p(packed), hmean.ctypes.data_as(ctypes.c_void_p),
                           hstd.ctypes.data_as(ctypes.c_void_p), hw.ctypes.data_as(ctypes.c_void_p), float(lam), _p(loss), _p(d),
                           _p(st), _p(ws), nb, _stream()))
    return loss.reshape(()), d, st


def ssim(pred, gt, mask_at_box=None):
    """SSIM of ZJUEvaluator._compute_ssim (reference src/zju_evaluator.py:21-45): pred, gt (3,H,W) or (1,3,H,W) in [0,1];
    mask_at_box (H,W): the images are cropped to its bounding rectangle (cv2.boundingRect) first.  Returns a float."""
    L = kl.get_library()
    a, b = _dev(pred, "pred").reshape(3, *pred.shape[-2:]), _dev(gt, "gt").reshape(3, *gt.shape[-2:])
    H, W = a.shape[-2:]
    x0, y0, w, h = 0, 0, W, H
    if mask_at_box is not None:
        ys, xs = torch.nonzero(mask_at_box.reshape(H, W) != 0, as_tuple=True)
        if ys.numel() == 0:
            raise ValueError("empty mask")
        x0, y0 = int(xs.min()), int(ys.min())
        w, h = int(xs.max()) - x0 + 1, int(ys.max()) - y0 + 1
    nb = L.kpn_ssim_scratch_bytes(w, h)
    if nb == 0:
        raise ValueError("crop smaller than the 7x7 SSIM window")
    scratch = torch.empty(nb, dtype=torch.uint8, device=a.device)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    L.check(L.kpn_ssim(_p(a), _p(b), H, W, x0, y0, w, h, _p(out), _p(scratch), _stream()))
    return float(out.item())


def selftest_mfma():
    """Checks on the device that v_mfma_f32_32x32x2_f32 has the operand/result lane maps the kernels assume."""
    L = kl.get_library()
    scratch = torch.zeros(65536, dtype=_f32, device="cuda")
    err = ctypes.c_float(0.0)
    torch.cuda.synchronize()
    rc = L.kpn_selftest_mfma(_p(scratch), _stream(), ctypes.byref(err))
    if rc != 0:
        print("selftest_mfma:", L.kpn_last_error().decode())
    return rc, err.value


def _encoder_stages(info_fn, args, flat):
    """{name: (V, H, W, C) view} of a stage buffer, from kpn_*_encoder_stage_info."""
    out, name = {}, ctypes.create_string_buffer(64)
    off, dims = ctypes.c_int64(0), (ctypes.c_int32 * 4)()
    i = 0
    while info_fn(*args, i, name, 64, ctypes.byref(off), dims) == 0:
        n = dims[0] * dims[1] * dims[2] * dims[3]
        out[name.value.decode()] = flat[off.value:off.value + n].reshape(*dims)
        i += 1
    return out


def geo_encoder_pack(plain, out_ch, out_ch_hd=8):
    """Packs the parameters of an HGFilterV2 (flat device fp32 in the order of include/kpnerf.h; encoders.flat_plain(encoders.geo_params(module)[0]))
    into the layout kpn_geo_encode reads (reference src/utils.py:313-414)."""
    L = kl.get_library()
    w = _dev(plain, "plain").reshape(-1)
    want = L.kpn_geo_encoder_plain_floats(out_ch, out_ch_hd)
    if w.numel() != want or want == 0:
        raise ValueError(f"expected {want} geometry encoder parameters, got {w.numel()}")
    packed = torch.empty(L.kpn_geo_encoder_packed_floats(out_ch, out_ch_hd), dtype=_f32, device=w.device)
    L.check(L.kpn_geo_encoder_pack_device(_p(w), _p(packed), out_ch, out_ch_hd, _stream()))
    return packed


def geo_encode(img, packed, ds=1, out_ch=64, out_ch_hd=8, eps=1e-5, want_stages=False):
    """HGFilterV2.forward(2 * avg_pool2d^ds(img) - 1) as attach_geo_feat calls it (reference src/model.py:653-666,
    src/utils.py:370-414; n_stack = 1, hd = False, norm = "group").  img: (V, 3, H, W) device fp32 in [0, 1].  Returns
    (feat (V, h/4, w/4, out_ch), feat_hd (V, h, w, out_ch_hd), stages or None), channels-last (NHWC), h = H >> ds.
    Forward only: raises on an input that requires a gradient."""
    L = kl.get_library()
    if isinstance(img, torch.Tensor) and img.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("geo_encode has no backward: the native encoders are forward only")
    a = _dev(img, "img")
    if a.dim() != 4 or a.shape[1] != 3:
        raise ValueError(f"img must be (V, 3, H, W), got {tuple(a.shape)}")
    V, _, H, W = a.shape
    args = (V, H, W, int(ds), int(out_ch), int(out_ch_hd))
    nb = L.kpn_geo_encoder_workspace_bytes(*args)
    if nb == 0:
        raise ValueError(f"the geometry encoder needs a network input whose height and width are multiples of 64 (got {H >> ds} x {W >> ds})")
    h, w = H >> ds, W >> ds
    feat = torch.empty(V, h // 4, w // 4, out_ch, dtype=_f32, device=a.device)
    feat_hd = torch.empty(V, h, w, out_ch_hd, dtype=_f32, device=a.device)
    st = torch.empty(L.kpn_geo_encoder_stage_floats(*args), dtype=_f32, device=a.device) if want_stages else None
    ws = torch.empty(nb, dtype=torch.uint8, device=a.device)
    L.check(L.kpn_geo_encode(_p(a), *args, _p(packed), float(eps), _p(feat), _p(feat_hd), _p(st), _p(ws), nb, _stream()))
    return feat, feat_hd, (_encoder_stages(L.kpn_geo_encoder_stage_info, args, st) if want_stages else None)


def tex_encoder_pack(plain, ngf=64, n_downsample=3, n_blocks=4, n_upsample=2, out_ch=8):
    """Packs the parameters of a ResBlkEncoder (flat device fp32: each convolution's weight then bias, in `layers` order;
    encoders.flat_plain(encoders.tex_params(module)[0])) into the layout kpn_tex_encode reads (reference src/utils.py:216-247)."""
    L = kl.get_library()
    cfg = (int(ngf), int(n_downsample), int(n_blocks), int(n_upsample), int(out_ch))
    w = _dev(plain, "plain").reshape(-1)
    want = L.kpn_tex_encoder_plain_floats(*cfg)
    if w.numel() != want or want == 0:
        raise ValueError(f"expected {want} texture encoder parameters, got {w.numel()}")
    packed = torch.empty(L.kpn_tex_encoder_packed_floats(*cfg), dtype=_f32, device=w.device)
    L.check(L.kpn_tex_encoder_pack_device(_p(w), _p(packed), *cfg, _stream()))
    return packed


def tex_encode(img, packed, ds=1, ngf=64, n_downsample=3, n_blocks=4, n_upsample=2, out_ch=8, eps=1e-5, want_stages=False):
    """ResBlkEncoder.forward(2 * avg_pool2d^ds(img) - 1) as attach_tex_feat calls it (reference src/model.py:668-680,
    src/utils.py:216-247; norm = "instance").  Returns (feat (V, ht, wt, out_ch) channels-last, stages or None).
    Forward only: raises on an input that requires a gradient."""
    L = kl.get_library()
    if isinstance(img, torch.Tensor) and img.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("tex_encode has no backward: the native encoders are forward only")
    a = _dev(img, "img")
    if a.dim() != 4 or a.shape[1] != 3:
        raise ValueError(f"img must be (V, 3, H, W), got {tuple(a.shape)}")
    V, _, H, W = a.shape
    args = (V, H, W, int(ds), int(ngf), int(n_downsample), int(n_blocks), int(n_upsample), int(out_ch))
    nb = L.kpn_tex_encoder_workspace_bytes(*args)
    if nb == 0:
        raise ValueError(f"texture encoder: unsupported size or arguments {args}")
    h, w = H >> ds, W >> ds
    for _ in range(n_downsample):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    feat = torch.empty(V, h << n_upsample, w << n_upsample, out_ch, dtype=_f32, device=a.device)
    st = torch.empty(L.kpn_tex_encoder_stage_floats(*args), dtype=_f32, device=a.device) if want_stages else None
    ws = torch.empty(nb, dtype=torch.uint8, device=a.device)
    L.check(L.kpn_tex_encode(_p(a), *args, _p(packed), float(eps), _p(feat), _p(st), _p(ws), nb, _stream()))
    return feat, (_encoder_stages(L.kpn_tex_encoder_stage_info, args, st) if want_stages else None)


# ------------------------------------------------------------------------------------------------
# Shared by the three families of differentiable layers below (kpn_conv2d_*, kpn_group_norm_*, the resampling steps): the check of
# their activations and the error path of a descriptor the library does not serve.
def _channels_last(t, name, channels=None):
    """a CUDA fp32 (N, C, H, W) tensor that is dense in channels_last (NHWC) memory, as it is"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not _on_gpu(t):
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); keypointnerf_amd has no CPU path")
    if t.dtype != _f32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.dim() != 4 or (channels is not None and t.shape[1] != channels):
        raise ValueError(f"{name} must be (N, {channels if channels is not None else 'C'}, H, W), got {tuple(t.shape)}")
    if not t.permute(0, 2, 3, 1).is_contiguous():
        raise ValueError(f"{name} must be dense in channels_last memory (x.contiguous(memory_format=torch.channels_last))")
    return t


def _desc_size(L, d, size_fn, probe_fn, label):
    """getattr(L, size_fn)(d): floats or bytes.  0 means the library does not serve the descriptor: its reason is fetched by calling
    ``probe_fn`` with nothing but the descriptor (validation fails before anything is read) and raised behind ``label``."""
    n = getattr(L, size_fn)(ctypes.byref(d))
    if n == 0:
        probe = getattr(L, probe_fn)
        probe(ctypes.byref(d), *(0 if t is kl.c_sz else None for t in probe.argtypes[1:]))
        raise ValueError(f"{label}: {L.kpn_last_error().decode()}")
    return n


def _desc_workspace(L, d, device, size_fn, probe_fn, label):
    nb = _desc_size(L, d, size_fn, probe_fn, label)
    return torch.empty(nb, dtype=torch.uint8, device=device), nb


_NORM_WORKSPACE = ("kpn_group_norm_workspace_bytes", "kpn_group_norm_forward", "group_norm: unsupported normalisation")


# ------------------------------------------------------------------------------------------------
# The three families of single convolution layers and their gradients, one description behind them as in the library (enc::Layer,
# csrc/api_layer.hip): a cached plan per layer shape (_layer_plan) and one body each for pack, forward and backward.  The public
# functions of a family, further down, say which layer theirs is: the family ("conv2d", "conv2d_s2", "conv2d_rp": kpn_<family>_*) and
# ``what``, (k, padding) of the stride-1 family or the kind of the other two.

# The arithmetic of the stride-1 convolution's GEMMs (include/kpnerf.h): ``arith`` = kl.CONV_F32 (0, the default: v_mfma_f32_32x32x2_f32)
# or kl.CONV_BF16X3 (1: three bf16 pieces per operand on v_mfma_f32_32x32x16_bf16, csrc/encoder_split_kernels.hip).  A packed weight, a
# workspace and a block's packed legs belong to one arithmetic.
class _ArithLibrary:
    """kpn_conv2d_<f> and kpn_conv_block_<f> of the library as their _ex forms with one arith; everything else is the library's"""

    def __init__(self, L, arith):
        self._L, self._arith = L, arith

    def __getattr__(self, name):
        for fam in ("kpn_conv2d_", "kpn_conv_block_"):
            if name.startswith(fam) and not name[len(fam):].startswith(("s2_", "rp_", "ex_")):
                fn, arith = getattr(self._L, fam + "ex_" + name[len(fam):]), self._arith

                def call(desc, *a):
                    return fn(desc, arith, *a)
                call.argtypes = [fn.argtypes[0]] + list(fn.argtypes[2:])
                setattr(self, name, call)       # looked up once per library and name
                return call
        return getattr(self._L, name)


_ARITH_LIBRARIES = {}


def _conv_library(arith):
    """the library whose kpn_conv2d_* / kpn_conv_block_* run in ``arith``: the plain entry points for CONV_F32"""
    if arith not in (kl.CONV_F32, kl.CONV_BF16X3):
        raise ValueError(f"arith must be CONV_F32 ({kl.CONV_F32}) or CONV_BF16X3 ({kl.CONV_BF16X3}), got {arith!r}")
    L = kl.get_library()
    if arith == kl.CONV_F32:
        return L
    key = (id(L), arith)
    if key not in _ARITH_LIBRARIES:
        _ARITH_LIBRARIES[key] = _ArithLibrary(L, arith)
    return _ARITH_LIBRARIES[key]


def _conv_weight(w):
    if not isinstance(w, torch.Tensor) or not _on_gpu(w):
        raise RuntimeError("weight must be a tensor on the GPU; keypointnerf_amd has no CPU path")
    if w.dtype != _f32 or w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"weight must be float32 (cout, cin, k, k), got {w.dtype} {tuple(w.shape)}")
    return w.contiguous()


_LAYER_DESCS = {"conv2d": kl.Conv2dDesc, "conv2d_s2": kl.Conv2dS2Desc, "conv2d_rp": kl.Conv2dRpDesc}
_NCHW_STEMS = (("conv2d_s2", kl.S2_STEM7), ("conv2d_rp", kl.RP_STEM7))      # read x as a contiguous NCHW tensor, have no input gradient


@functools.lru_cache(maxsize=4096)      # a training loop has one per layer shape and arithmetic: the encoders together stay below 200
def _layer_plan(L, fam, what, cin, cout, N=None, H=None, W=None, has_bias=False):
    """Everything about a layer that its key decides, built once: ``L`` is the library the calls run on (_conv_library(arith): the
    arithmetic is part of the key through it), N to has_bias the descriptor's fields.  Callers pass them by position.
    -> (byref of the descriptor, forward, backward, pack_device, workspace bytes, packed floats, Ho, Wo, shape of dw in the layer's own
    layout (IOHW for the transposed layer), x is read as contiguous NCHW, the layer has an input gradient, the descriptor).
    Without N, H, W it is the packer's plan, which depends on the weight alone: it has no workspace and no output size.
    Raises the library's reason for a descriptor it does not serve (nothing is kept then: the next call asks again)."""
    weight_only = N is None
    if weight_only:
        N, H, W = 1, 2, 2
    d = _LAYER_DESCS[fam]()
    d.N, d.H, d.W, d.cin, d.cout, d.has_bias = int(N), int(H), int(W), int(cin), int(cout), int(has_bias)
    if fam == "conv2d":
        k, pad = what
        d.k, d.pad = int(k), int(pad)
        Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    elif fam == "conv2d_s2":
        d.kind, k = int(what), 7 if what == kl.S2_STEM7 else 3
        Ho, Wo = (2 * H, 2 * W) if what == kl.S2_DECONV3 else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    else:
        d.kind, k = int(what), 3 if what == kl.RP_CONV3 else 7
        Ho, Wo = H, W
    dw_shape = (cin, cout, k, k) if (fam, what) == ("conv2d_s2", kl.S2_DECONV3) else (cout, cin, k, k)
    pre = f"kpn_{fam}_"
    if weight_only:
        nb, pf = 0, _desc_size(L, d, pre + "packed_floats", pre + "pack_device", f"{fam}: unsupported weight {dw_shape}")
    else:
        nb = _desc_size(L, d, pre + "workspace_bytes", pre + "forward", f"{fam}: unsupported convolution")
        pf = getattr(L, pre + "packed_floats")(ctypes.byref(d))
    nchw = (fam, what) in _NCHW_STEMS
    return (ctypes.byref(d), getattr(L, pre + "forward"), getattr(L, pre + "backward"), getattr(L, pre + "pack_device"), nb, pf, Ho, Wo,
            dw_shape, nchw, not nchw, d)


def _layer_supported(L, fam, what, cin, cout):
    try:
        _layer_plan(L, fam, what, cin, cout)
    except ValueError:
        return False
    return True


def _layer_input(t, name, nchw, channels=None):
    """x as the layer reads it: dense in channels_last memory, or (the stems) a contiguous NCHW tensor"""
    if not nchw:
        return _channels_last(t, name, channels)
    t = _dev(t, name)
    if t.dim() != 4 or not t.is_contiguous() or (channels is not None and t.shape[1] != channels):
        raise ValueError(f"{name} must be a contiguous NCHW (N, {channels if channels is not None else 'C'}, H, W) tensor, got {tuple(t.shape)}")
    return t


def _layer_pack(L, fam, what, w, cin, cout):
    ref, _, _, pack, _, n, _, _, _, _, _, _ = _layer_plan(L, fam, what, cin, cout)
    packed = torch.empty(n, dtype=_f32, device=w.device)
    L.check(pack(ref, _p(w), _p(packed), _stream()))
    return packed


def _layer_forward(L, fam, what, x, packed, bias, cout):
    try:
        N, cin, H, W = x.shape
    except (AttributeError, ValueError):    # no (N, C, H, W) to plan with: the refusal of the layout the layer reads
        _layer_input(x, "x", (fam, what) in _NCHW_STEMS)
        raise
    ref, forward, _, _, nb, n, Ho, Wo, _, nchw, _, _ = _layer_plan(L, fam, what, cin, cout, N, H, W, bias is not None)
    x = _layer_input(x, "x", nchw)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    if packed.numel() != n or packed.dtype != _f32 or packed.device != x.device:
        raise ValueError(f"packed does not belong to this convolution ({fam}_pack)")
    b = None if bias is None else _dev(bias.detach(), "bias")
    if b is not None and tuple(b.shape) != (cout,):
        raise ValueError(f"bias must be ({cout},), got {tuple(b.shape)}")
    y = torch.empty(N, Ho, Wo, cout, dtype=_f32, device=x.device)
    L.check(forward(ref, _p(x), _p(packed), _p(b), _p(y), _p(ws), nb, _stream()))
    return y.permute(0, 3, 1, 2)


def _layer_backward(L, fam, what, x, dy, packed, x_shape, has_bias, want_dx, want_dw, want_db):
    """dy: checked by the caller (_channels_last)"""
    N, cin, H, W = x_shape
    cout = dy.shape[1]
    ref, _, backward, _, nb, n, Ho, Wo, dw_shape, nchw, has_dx, _ = _layer_plan(L, fam, what, cin, cout, N, H, W, has_bias)
    if want_dx and not has_dx:
        raise ValueError(f"{fam}: the stem has no input gradient")
    if tuple(dy.shape) != (N, cout, Ho, Wo):
        raise ValueError(f"dy must be {(N, cout, Ho, Wo)}, got {tuple(dy.shape)}")
    want_db = bool(want_db and has_bias)
    ws = torch.empty(nb, dtype=torch.uint8, device=dy.device)
    if want_dw:
        x = _layer_input(x, "x", nchw, cin)
        if tuple(x.shape) != (N, cin, H, W):
            raise ValueError(f"x must be {(N, cin, H, W)}, got {tuple(x.shape)}")
    if want_dx and (packed is None or packed.numel() != n or packed.device != dy.device):
        raise ValueError(f"packed does not belong to this convolution ({fam}_pack)")
    dx = torch.empty(N, H, W, cin, dtype=_f32, device=dy.device) if want_dx else None
    dw = torch.empty(dw_shape, dtype=_f32, device=dy.device) if want_dw else None
    db = torch.empty(cout, dtype=_f32, device=dy.device) if want_db else None
    if want_dx or want_dw or want_db:
        L.check(backward(ref, _p(x) if want_dw else None, _p(dy), _p(packed) if want_dx else None, _p(dx), _p(dw), _p(db), _p(ws), nb,
                         _stream()))
    return (None if dx is None else dx.permute(0, 3, 1, 2)), dw, db


# ------------------------------------------------------------------------------------------------
# One stride-1 convolution and its gradients (kpn_conv2d_*; torch.nn.functional.conv2d and its autograd, reference
# src/utils.py:416-474, 261-309, 322-414).  Activations are channels_last tensors of logical shape (N, C, H, W).
def conv2d_supported(cin, cout, k, arith=0):
    """whether kpn_conv2d_* serves a stride-1 convolution of these channel counts and this square kernel"""
    return _layer_supported(_conv_library(arith), "conv2d", (k, 0), cin, cout)


def conv2d_pack(weight, arith=0):
    """The two packed copies of an OIHW weight that conv2d_forward (first) and the input gradient of conv2d_backward (second:
    transposed and flipped) read (kpn_conv2d_pack_device), for the calls with the same ``arith``."""
    L = _conv_library(arith)
    w = _conv_weight(weight.detach())
    return _layer_pack(L, "conv2d", (w.shape[2], 0), w, w.shape[1], w.shape[0])


def conv2d_forward(x, packed, bias, cout, k, padding, arith=0):
    """conv2d(x, w, bias, stride=1, padding=padding) for packed = conv2d_pack(w, arith) (kpn_conv2d_forward).  x: (N, cin, H, W)
    channels_last; returns (N, cout, Ho, Wo) channels_last."""
    return _layer_forward(_conv_library(arith), "conv2d", (k, padding), x, packed, bias, cout)


def conv2d_backward(x, dy, packed, cin, k, padding, has_bias, want_dx=True, want_dw=True, want_db=True, arith=0):
    """(dx, dw, db) of conv2d_forward for the output gradient dy (N, cout, Ho, Wo) channels_last (kpn_conv2d_backward); a
    gradient that is not wanted is None and its leg is not launched.  x (channels_last) is read for dw only and packed for dx
    only: either may be None when its leg is off.  dx is channels_last, dw OIHW."""
    L = _conv_library(arith)
    dy = _channels_last(dy, "dy")
    N, _, Ho, Wo = dy.shape
    return _layer_backward(L, "conv2d", (k, padding), x, dy, packed, (N, cin, Ho - 2 * padding + k - 1, Wo - 2 * padding + k - 1), has_bias,
                           want_dx, want_dw, want_db)


# ------------------------------------------------------------------------------------------------
# The resolution-changing layers and their gradients (kpn_conv2d_s2_*): Conv2d(k 3, stride 2, pad 1), the stem Conv2d(k 7, stride 2,
# pad 3) and ConvTranspose2d(k 3, stride 2, pad 1, output_padding 1), reference src/utils.py:199-247, 322-414.  ``kind`` is one of
# lib.S2_CONV3 / S2_STEM7 / S2_DECONV3.  Activations are channels_last tensors of logical shape (N, C, H, W); the stem's input alone
# is a contiguous NCHW tensor, read as it is.
def conv2d_s2_supported(kind, cin, cout):
    """whether kpn_conv2d_s2_* serves a layer of this kind and these channel counts"""
    return _layer_supported(kl.get_library(), "conv2d_s2", kind, cin, cout)


def conv2d_s2_pack(weight, kind):
    """The packed copies of a weight in the layer's own layout that conv2d_s2_forward (first) and the input gradient of
    conv2d_s2_backward (second; the stem has none) read (kpn_conv2d_s2_pack_device)."""
    L = kl.get_library()
    w = _conv_weight(weight.detach())
    if w.shape[2] != (7 if kind == kl.S2_STEM7 else 3):
        raise ValueError(f"conv2d_s2: a weight {tuple(w.shape)} does not belong to kind {kind}")
    # (cin, cout) of a weight in the layer's own layout: OIHW, or (cin, cout, 3, 3) for the transposed layer
    cin, cout = (w.shape[0], w.shape[1]) if kind == kl.S2_DECONV3 else (w.shape[1], w.shape[0])
    return _layer_pack(L, "conv2d_s2", kind, w, cin, cout)


def conv2d_s2_forward(x, packed, bias, cout, kind):
    """The layer's forward for packed = conv2d_s2_pack(w, kind) (kpn_conv2d_s2_forward).  x: (N, cin, H, W) channels_last, or
    contiguous NCHW for the stem; returns (N, cout, Ho, Wo) channels_last."""
    return _layer_forward(kl.get_library(), "conv2d_s2", kind, x, packed, bias, cout)


def conv2d_s2_backward(x, dy, packed, x_shape, kind, has_bias, want_dx=True, want_dw=True, want_db=True):
    """(dx, dw, db) of conv2d_s2_forward for the output gradient dy (N, cout, Ho, Wo) channels_last (kpn_conv2d_s2_backward); a
    gradient that is not wanted is None and its leg is not launched.  x (of shape x_shape, in the forward's layout) is read for dw
    only and packed for dx only: either may be None when its leg is off.  dx is channels_last, dw has the weight's own layout.  The
    stem has no input gradient."""
    return _layer_backward(kl.get_library(), "conv2d_s2", kind, x, _channels_last(dy, "dy"), packed, x_shape, has_bias, want_dx, want_dw,
                           want_db)


# ------------------------------------------------------------------------------------------------
# The replication-padded stride-1 convolutions and their gradients (kpn_conv2d_rp_*): ReplicationPad2d(k // 2) + Conv2d(k) for k = 3,
# k = 7 and the 7x7 stem, reference src/utils.py:199-259.  ``kind`` is one of lib.RP_CONV3 / RP_CONV7 / RP_STEM7.  Activations are
# channels_last tensors of logical shape (N, C, H, W); the stem's input alone is a contiguous NCHW tensor, read as it is.  The output
# has the input's size.
def conv2d_rp_kind(weight_shape):
    """the kind a (cout, cin, k, k) weight belongs to: k = 3, k = 7, or the stem (k = 7 with at most 4 input channels)"""
    k = weight_shape[-1]
    if len(weight_shape) != 4 or k not in (3, 7) or weight_shape[-2] != k:
        raise ValueError(f"conv2d_rp: a weight {tuple(weight_shape)} (3x3 under ReplicationPad2d(1) or 7x7 under ReplicationPad2d(3))")
    return kl.RP_CONV3 if k == 3 else (kl.RP_STEM7 if weight_shape[1] <= 4 else kl.RP_CONV7)


def conv2d_rp_supported(kind, cin, cout):
    """whether kpn_conv2d_rp_* serves a layer of this kind and these channel counts"""
    return _layer_supported(kl.get_library(), "conv2d_rp", kind, cin, cout)


def conv2d_rp_pack(weight, kind):
    """The packed copies of an OIHW weight that conv2d_rp_forward (first) and the input gradient of conv2d_rp_backward (second:
    transposed and flipped; the stem has none) read (kpn_conv2d_rp_pack_device)."""
    L = kl.get_library()
    w = _conv_weight(weight.detach())
    if w.shape[2] != (3 if kind == kl.RP_CONV3 else 7):
        raise ValueError(f"conv2d_rp: a weight {tuple(w.shape)} does not belong to kind {kind}")
    return _layer_pack(L, "conv2d_rp", kind, w, w.shape[1], w.shape[0])


def conv2d_rp_forward(x, packed, bias, cout, kind):
    """The layer's forward for packed = conv2d_rp_pack(w, kind) (kpn_conv2d_rp_forward).  x: (N, cin, H, W) channels_last, or
    contiguous NCHW for the stem; returns (N, cout, H, W) channels_last."""
    return _layer_forward(kl.get_library(), "conv2d_rp", kind, x, packed, bias, cout)


def conv2d_rp_backward(x, dy, packed, x_shape, kind, has_bias, want_dx=True, want_dw=True, want_db=True):
    """(dx, dw, db) of conv2d_rp_forward for the output gradient dy (N, cout, H, W) channels_last (kpn_conv2d_rp_backward); a gradient
    that is not wanted is None and its leg is not launched.  x (of shape x_shape, in the forward's layout) is read for dw only and
    packed for dx only: either may be None when its leg is off.  dx is channels_last, dw OIHW.  The stem has no input gradient."""
    return _layer_backward(kl.get_library(), "conv2d_rp", kind, x, _channels_last(dy, "dy"), packed, x_shape, has_bias, want_dx, want_dw,
                           want_db)


# ------------------------------------------------------------------------------------------------
# GroupNorm / InstanceNorm2d [+ ReLU] and its gradients (kpn_group_norm_*; torch.nn.functional.group_norm [+ relu] and their autograd,
# reference src/utils.py:416-474, 199-247).  Activations are channels_last tensors of logical shape (N, C, H, W).
def _norm_desc(N, H, W, C, groups, affine, relu, eps):
    d = kl.GroupNormDesc()
    d.N, d.H, d.W, d.C, d.G, d.affine, d.relu, d.eps = int(N), int(H), int(W), int(C), int(groups), int(affine), int(relu), float(eps)
    return d


def group_norm_supported(C, groups):
    """whether kpn_group_norm_* serves this channel count and grouping"""
    return kl.get_library().kpn_group_norm_workspace_bytes(ctypes.byref(_norm_desc(1, 1, 1, C, groups, 0, 0, 1e-5))) > 0


def _norm_vec(t, name, C):
    t = _dev(t.detach(), name)
    if tuple(t.shape) != (C,):
        raise ValueError(f"{name} must be ({C},), got {tuple(t.shape)}")
    return t


def group_norm_forward(x, weight, bias, groups, eps, relu):
    """[relu](group_norm(x, groups, weight, bias, eps)) (kpn_group_norm_forward).  x: (N, C, H, W) channels_last; weight and bias
    both (C,) or both None (groups = C without them is InstanceNorm2d).  Returns (y channels_last, stats): stats holds the scale and
    shift per (image, channel) and the mean and rstd per (image, group) that group_norm_backward reads."""
    L = kl.get_library()
    x = _channels_last(x, "x")
    N, C, H, W = x.shape
    if (weight is None) != (bias is None):
        raise ValueError("weight and bias must both be given or both be None")
    d = _norm_desc(N, H, W, C, groups, weight is not None, relu, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_NORM_WORKSPACE)
    w = None if weight is None else _norm_vec(weight, "weight", C)
    b = None if bias is None else _norm_vec(bias, "bias", C)
    # y is no view of another tensor: autograd refuses an in-place ReLU on a view that a two-output operator returned
    y = torch.empty(N, C, H, W, dtype=_f32, device=x.device, memory_format=torch.channels_last)
    stats = torch.empty(L.kpn_group_norm_stats_floats(ctypes.byref(d)), dtype=_f32, device=x.device)
    L.check(L.kpn_group_norm_forward(ctypes.byref(d), _p(x), _p(w), _p(b), _p(y), _p(stats), _p(ws), nb, _stream()))
    return y, stats


def group_norm_backward(x, dy, weight, stats, groups, eps, relu, want_dx=True, want_dw=True, want_db=True):
    """(dx, dweight, dbias) of group_norm_forward for the output gradient dy (N, C, H, W) channels_last (kpn_group_norm_backward);
    stats is what the forward returned for this x and weight.  A gradient that is not wanted is None and nothing is computed for
    it; dweight and dbias exist only with a weight.  dx is channels_last."""
    L = kl.get_library()
    x, dy = _channels_last(x, "x"), _channels_last(dy, "dy")
    N, C, H, W = x.shape
    if tuple(dy.shape) != tuple(x.shape):
        raise ValueError(f"dy must be {tuple(x.shape)}, got {tuple(dy.shape)}")
    affine = weight is not None
    want_dw, want_db = bool(want_dw and affine), bool(want_db and affine)
    d = _norm_desc(N, H, W, C, groups, affine, relu, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_NORM_WORKSPACE)
    if stats.numel() != L.kpn_group_norm_stats_floats(ctypes.byref(d)) or stats.dtype != _f32 or stats.device != x.device:
        raise ValueError("stats does not belong to this normalisation (group_norm_forward)")
    w = _norm_vec(weight, "weight", C) if affine else None
    dx = torch.empty(N, H, W, C, dtype=_f32, device=x.device) if want_dx else None
    dw = torch.empty(C, dtype=_f32, device=x.device) if want_dw else None
    db = torch.empty(C, dtype=_f32, device=x.device) if want_db else None
    if want_dx or want_dw or want_db:
        L.check(L.kpn_group_norm_backward(ctypes.byref(d), _p(x), _p(dy), _p(w), _p(stats.contiguous()), _p(dx), _p(dw), _p(db), _p(ws), nb,
                                          _stream()))
    return (None if dx is None else dx.permute(0, 3, 1, 2)), dw, db


# ------------------------------------------------------------------------------------------------
# A whole ConvBlock and its gradients as one call each (kpn_conv_block_*; reference src/utils.py:416-474, norm = "group").  Activations
# are channels_last tensors of logical shape (N, C, H, W).  ``norms`` is [(gamma, beta)] and ``packed`` [conv2d_pack(weight)] per leg:
# bn1 / conv1, bn2 / conv2, bn3 / conv3 and, for cin != cout, bn4 / the 1x1 downsample convolution.
_BLOCK_WORKSPACE = ("kpn_conv_block_workspace_bytes", "kpn_conv_block_forward", "conv_block: unsupported block")


def _block_desc(N, H, W, cin, cout, eps):
    d = kl.ConvBlockDesc()
    d.N, d.H, d.W, d.cin, d.cout, d.eps = int(N), int(H), int(W), int(cin), int(cout), float(eps)
    return d


def conv_block_supported(cin, cout, arith=0):
    """whether kpn_conv_block_* serves a ConvBlock of these widths"""
    return _conv_library(arith).kpn_conv_block_workspace_bytes(ctypes.byref(_block_desc(1, 1, 1, cin, cout, 1e-5))) > 0


def _block_widths(cin, cout):
    legs = 4 if cin != cout else 3
    return legs, (cin, cout // 2, cout // 4, cin)[:legs], (cout // 2, cout // 4, cout // 4, cout)[:legs]


def _block_params(L, cin, cout, norms, packed, device, keep):
    """kpn_conv_block_params of the legs; the tensors it points to are appended to ``keep``"""
    legs, win, wout = _block_widths(cin, cout)
    if len(norms) != legs or len(packed) != legs:
        raise ValueError(f"a ConvBlock({cin}, {cout}) has {legs} legs, got {len(norms)} norms and {len(packed)} packed weights")
    pr = kl.ConvBlockParams()
    for i in range(legs):
        g, b = (_norm_vec(t, f"bn{i + 1}.{n}", win[i]) for t, n in zip(norms[i], ("weight", "bias")))
        pk = packed[i]
        if pk.numel() != _layer_plan(L, "conv2d", (3 if i < 3 else 1, 0), win[i], wout[i])[5] or pk.dtype != _f32 or pk.device != device:
            raise ValueError(f"packed[{i}] does not belong to this block's convolution {win[i]} -> {wout[i]} (conv2d_pack)")
        keep += [g, b, pk]
        pr.gamma[i], pr.beta[i], pr.packed[i] = g.data_ptr(), b.data_ptr(), pk.data_ptr()
    return pr


def conv_block_forward(x, norms, packed, cout, eps, arith=0):
    """ConvBlock(cin, cout)(x) (kpn_conv_block_forward).  x: (N, cin, H, W) channels_last.  Returns (y (N, cout, H, W) channels_last,
    state): state holds the outputs of conv1 and conv2 and the statistics of every norm, which conv_block_backward reads.  ``packed``
    is [conv2d_pack(weight, arith)] with the same ``arith``."""
    L = _conv_library(arith)
    x = _channels_last(x, "x")
    N, cin, H, W = x.shape
    d = _block_desc(N, H, W, cin, cout, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_BLOCK_WORKSPACE)
    keep = []
    pr = _block_params(L, cin, cout, norms, packed, x.device, keep)
    y = torch.empty(N, cout, H, W, dtype=_f32, device=x.device, memory_format=torch.channels_last)
    state = torch.empty(L.kpn_conv_block_state_floats(ctypes.byref(d)), dtype=_f32, device=x.device)
    L.check(L.kpn_conv_block_forward(ctypes.byref(d), _p(x), ctypes.byref(pr), _p(y), _p(state), _p(ws), nb, _stream()))
    return y, state


def conv_block_backward(x, dy, norms, packed, state, eps, want_dx=True, want=None, arith=0):
    """(dx, [(dgamma, dbeta, dw)] per leg) of conv_block_forward for the output gradient dy (N, cout, H, W) channels_last
    (kpn_conv_block_backward).  ``want`` is [(dgamma, dbeta, dw) wanted] per leg (default: all); what is not wanted is None, and a leg
    that nothing wanted needs is not launched.  dx is channels_last, dw OIHW."""
    L = _conv_library(arith)
    x, dy = _channels_last(x, "x"), _channels_last(dy, "dy")
    N, cin, H, W = x.shape
    cout = dy.shape[1]
    if tuple(dy.shape) != (N, cout, H, W):
        raise ValueError(f"dy must be {(N, cout, H, W)}, got {tuple(dy.shape)}")
    d = _block_desc(N, H, W, cin, cout, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_BLOCK_WORKSPACE)
    keep = []
    pr = _block_params(L, cin, cout, norms, packed, x.device, keep)
    if state.numel() != L.kpn_conv_block_state_floats(ctypes.byref(d)) or state.dtype != _f32 or state.device != x.device:
        raise ValueError("state does not belong to this block (conv_block_forward)")
    legs, win, wout = _block_widths(cin, cout)
    want = [(True, True, True)] * legs if want is None else want
    new = lambda *shape: torch.empty(*shape, dtype=_f32, device=x.device)  # noqa: E731
    dx = new(N, H, W, cin) if want_dx else None
    gr, out = kl.ConvBlockGrads(), []
    for i in range(legs):
        k = 3 if i < 3 else 1
        t = (new(win[i]) if want[i][0] else None, new(win[i]) if want[i][1] else None, new(wout[i], win[i], k, k) if want[i][2] else None)
        gr.dgamma[i], gr.dbeta[i], gr.dw[i] = (None if v is None else v.data_ptr() for v in t)
        out.append(t)
    if want_dx or any(any(w) for w in want):
        L.check(L.kpn_conv_block_backward(ctypes.byref(d), _p(x), _p(dy), ctypes.byref(pr), _p(state.contiguous()), _p(dx), ctypes.byref(gr),
                                          _p(ws), nb, _stream()))
    return (None if dx is None else dx.permute(0, 3, 1, 2)), out


# ------------------------------------------------------------------------------------------------
# A whole ResBlkEncoder and its parameter gradients as one call each (kpn_res_encoder_*; reference src/utils.py:199-259,
# norm = "instance").  x is the contiguous NCHW image, read as it is; y is a channels_last tensor of logical shape (N, out_ch, Ho, Wo).
# ``cfg`` is (ngf, n_down, n_blocks, n_up, out_ch); the layers are the convolutions in module order: the stem, the stride-2 layers, two
# per ResBlk, the transposed layers, the output layer.
_RES_ENCODER_WORKSPACE = ("kpn_res_encoder_workspace_bytes", "kpn_res_encoder_forward", "res_encoder: unsupported encoder")


def _res_encoder_desc(N, H, W, in_ch, cfg, eps):
    d = kl.ResEncoderDesc()
    d.N, d.H, d.W, d.in_ch, d.eps = int(N), int(H), int(W), int(in_ch), float(eps)
    d.ngf, d.n_down, d.n_blocks, d.n_up, d.out_ch = (int(v) for v in cfg)
    return d


def res_encoder_supported(in_ch, cfg, N=1, H=None, W=None):
    """whether kpn_res_encoder_* serves an encoder of this configuration (and, when given, of this input size)"""
    return res_encoder_refusal(in_ch, cfg, N, H, W) is None


def res_encoder_refusal(in_ch, cfg, N=1, H=None, W=None):
    """None if kpn_res_encoder_* serves the encoder, else the library's reason"""
    L = kl.get_library()
    f = 1 << max(0, min(int(cfg[1]), 16))
    d = _res_encoder_desc(N, f if H is None else H, f if W is None else W, in_ch, cfg, 1e-5)
    if L.kpn_res_encoder_workspace_bytes(ctypes.byref(d)) > 0:
        return None
    L.kpn_res_encoder_forward(ctypes.byref(d), None, None, None, None, None, None, 0, None)
    return L.kpn_last_error().decode()


def _pointer_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def res_encoder_layer_shapes(in_ch, cfg):
    """[(weight shape, bias length)] of the layers in module order"""
    ngf, n_down, n_blocks, n_up, out_ch = (int(v) for v in cfg)
    out, C = [((ngf, in_ch, 7, 7), ngf)], ngf
    for _ in range(n_down):
        out.append(((2 * C, C, 3, 3), 2 * C))
        C *= 2
    out += [((C, C, 3, 3), C)] * (2 * n_blocks)
    for _ in range(n_up):
        out.append(((C, C // 2, 3, 3), C // 2))        # ConvTranspose2d: (cin, cout, k, k)
        C //= 2
    out.append(((out_ch, C, 7, 7), out_ch))
    return out


def _res_encoder_vectors(tensors, in_ch, cfg, what):
    shapes = res_encoder_layer_shapes(in_ch, cfg)
    if len(tensors) != len(shapes):
        raise ValueError(f"res_encoder: {len(shapes)} layers, got {len(tensors)} {what}")
    return shapes


def res_encoder_pack(weights, in_ch, cfg):
    """The packed weights of every layer in one buffer (kpn_res_encoder_pack_device): per layer what its own packer gives
    (conv2d_rp_pack / conv2d_s2_pack)."""
    L = kl.get_library()
    shapes = _res_encoder_vectors(weights, in_ch, cfg, "weights")
    ws = [_conv_weight(w.detach()) for w in weights]
    for i, (w, (shape, _)) in enumerate(zip(ws, shapes)):
        if tuple(w.shape) != shape:
            raise ValueError(f"res_encoder: the weight of layer {i} must be {shape}, got {tuple(w.shape)}")
    d = _res_encoder_desc(1, 1 << int(cfg[1]), 1 << int(cfg[1]), in_ch, cfg, 1e-5)
    n = _desc_size(L, d, "kpn_res_encoder_packed_floats", "kpn_res_encoder_pack_device", "res_encoder: unsupported encoder")
    packed = torch.empty(n, dtype=_f32, device=ws[0].device)
    L.check(L.kpn_res_encoder_pack_device(ctypes.byref(d), _pointer_array(ws), _p(packed), _stream()))
    return packed


def _res_encoder_x(x):
    x = _dev(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous NCHW (N, C, H, W) tensor, got {tuple(x.shape)}")
    return x


def res_encoder_forward(x, packed, biases, cfg, eps):
    """ResBlkEncoder(x) for packed = res_encoder_pack(weights, ...) and the layers' biases (kpn_res_encoder_forward).  x: contiguous NCHW
    (N, in_ch, H, W).  Returns (y (N, out_ch, Ho, Wo) channels_last, state): state holds every convolution output, every a_k and every
    norm's statistics, which res_encoder_backward reads."""
    L = kl.get_library()
    x = _res_encoder_x(x)
    N, in_ch, H, W = x.shape
    shapes = _res_encoder_vectors(biases, in_ch, cfg, "biases")
    d = _res_encoder_desc(N, H, W, in_ch, cfg, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_RES_ENCODER_WORKSPACE)
    if packed.numel() != L.kpn_res_encoder_packed_floats(ctypes.byref(d)) or packed.dtype != _f32 or packed.device != x.device:
        raise ValueError("packed does not belong to this encoder (res_encoder_pack)")
    bs = [_norm_vec(b, f"bias of layer {i}", n) for i, (b, (_, n)) in enumerate(zip(biases, shapes))]
    f = int(cfg[1]) - int(cfg[3])
    y = torch.empty(N, H >> f, W >> f, int(cfg[4]), dtype=_f32, device=x.device)
    state = torch.empty(L.kpn_res_encoder_state_floats(ctypes.byref(d)), dtype=_f32, device=x.device)
    L.check(L.kpn_res_encoder_forward(ctypes.byref(d), _p(x), _p(packed), _pointer_array(bs), _p(y), _p(state), _p(ws), nb, _stream()))
    return y.permute(0, 3, 1, 2), state


def res_encoder_backward(x, dy, packed, state, cfg, eps, want=None):
    """[(dw, db)] per layer of res_encoder_forward for the output gradient dy (N, out_ch, Ho, Wo) channels_last
    (kpn_res_encoder_backward).  ``want`` is [(dw, db) wanted] per layer (default: all); what is not wanted is None, and the layers below
    the lowest wanted weight gradient are not walked.  The db of every layer but the last is exactly zero (a bias in front of an
    InstanceNorm2d without parameters does not reach the output)."""
    L = kl.get_library()
    x, dy = _res_encoder_x(x), _channels_last(dy, "dy")
    N, in_ch, H, W = x.shape
    shapes = res_encoder_layer_shapes(in_ch, cfg)
    want = [(True, True)] * len(shapes) if want is None else want
    if len(want) != len(shapes):
        raise ValueError(f"res_encoder: {len(shapes)} layers, got {len(want)} entries of want")
    f = int(cfg[1]) - int(cfg[3])
    if tuple(dy.shape) != (N, int(cfg[4]), H >> f, W >> f):
        raise ValueError(f"dy must be {(N, int(cfg[4]), H >> f, W >> f)}, got {tuple(dy.shape)}")
    d = _res_encoder_desc(N, H, W, in_ch, cfg, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_RES_ENCODER_WORKSPACE)
    if packed.numel() != L.kpn_res_encoder_packed_floats(ctypes.byref(d)) or packed.dtype != _f32 or packed.device != x.device:
        raise ValueError("packed does not belong to this encoder (res_encoder_pack)")
    if state.numel() != L.kpn_res_encoder_state_floats(ctypes.byref(d)) or state.dtype != _f32 or state.device != x.device:
        raise ValueError("state does not belong to this encoder (res_encoder_forward)")
    new = lambda *shape: torch.empty(*shape, dtype=_f32, device=x.device)  # noqa: E731
    out = [(new(*shape) if w_[0] else None, new(n) if w_[1] else None) for (shape, n), w_ in zip(shapes, want)]
    if any(any(w_) for w_ in want):
        L.check(L.kpn_res_encoder_backward(ctypes.byref(d), _p(x), _p(dy), _p(packed), _p(state.contiguous()), _pointer_array([o[0] for o in out]),
                                           _pointer_array([o[1] for o in out]), _p(ws), nb, _stream()))
    return out


# ------------------------------------------------------------------------------------------------
# A whole HGFilterV2 (n_stack = 1, hd = False, norm = "group") and its parameter gradients as one call each (kpn_hg_filter_*; reference
# src/utils.py:322-414).  x is the contiguous NCHW image, read as it is; out and x_hd are channels_last tensors of logical shape
# (N, out_ch, H / 4, W / 4) and (N, out_ch_hd, H, W).  ``cfg`` is (in_ch, c_stem, c2, c3, c4, depth, c_hd, out_ch_hd, out_ch).  ``tensors``
# in the order of include/kpnerf.h: conv1 w, b; bn1 w, b; per ConvBlock in dataflow order (conv2, conv3, conv4, the HourGlass's b1_d, b2_d,
# b1_{d-1}, ..., b2_plus_1, b3_1, ..., b3_d - its module order - and top_m_0) the 9 or 12 tensors of conv_block; unpack1.conv w;
# unpack1.norm w, b; conv_out w, b; conv_last0 w, b; bn_end0 w, b; l0 w, b.
_HG_FILTER_WORKSPACE = ("kpn_hg_filter_workspace_bytes", "kpn_hg_filter_forward", "hg_filter: unsupported network")
_HG_FILTER_FIELDS = ("in_ch", "c_stem", "c2", "c3", "c4", "depth", "c_hd", "out_ch_hd", "out_ch")


def _hg_filter_desc(N, H, W, cfg, eps):
    d = kl.HgFilterDesc()
    d.N, d.H, d.W, d.eps = int(N), int(H), int(W), float(eps)
    for n, v in zip(_HG_FILTER_FIELDS, cfg):
        setattr(d, n, int(v))
    return d


def hg_filter_refusal(cfg, N=1, H=None, W=None):
    """None if kpn_hg_filter_* serves the network (and, when given, the input size), else the library's reason"""
    L = kl.get_library()
    f = 4 << max(1, min(int(cfg[5]), 8))
    d = _hg_filter_desc(N, f if H is None else H, f if W is None else W, cfg, 1e-5)
    if L.kpn_hg_filter_workspace_bytes(ctypes.byref(d)) > 0:
        return None
    L.kpn_hg_filter_forward(ctypes.byref(d), None, None, None, None, None, None, 0, None)
    return L.kpn_last_error().decode()


def hg_filter_supported(cfg, N=1, H=None, W=None):
    """whether kpn_hg_filter_* serves an HGFilterV2 of these widths and this depth (and, when given, of this input size)"""
    return hg_filter_refusal(cfg, N, H, W) is None


def hg_filter_block_widths(cfg):
    """[(cin, cout)] of the ConvBlocks in tensor order"""
    _, c_stem, c2, c3, c4, depth = (int(v) for v in cfg[:6])
    return [(c_stem, c2), (c2, c3), (c3, c4)] + [(c4, c4)] * (3 * depth + 2)


def hg_filter_shapes(cfg):
    """the shapes of ``tensors`` in order"""
    in_ch, c_stem, c2, c3, c4, depth, c_hd, out_ch_hd, out_ch = (int(v) for v in cfg)
    out = [(c_stem, in_ch, 7, 7), (c_stem,), (c_stem,), (c_stem,)]
    for cin, cout in hg_filter_block_widths(cfg):
        legs, win, wout = _block_widths(cin, cout)
        for i in range(legs):
            k = 3 if i < 3 else 1
            out += [(win[i],), (win[i],), (wout[i], win[i], k, k)]
    out += [(c2, c_hd, 3, 3), (c_hd,), (c_hd,), (out_ch_hd, c_hd, 5, 5), (out_ch_hd,), (c4, c4, 1, 1), (c4,), (c4,), (c4,), (out_ch, c4, 1, 1), (out_ch,)]
    return out


def hg_filter_state_floats(N, H, W, cfg):
    """the floats of hg_filter_forward's state for this input size: the library's own answer (kpn_hg_filter_state_floats, a host-only
    query; 0 for a network it does not serve).  The layout is documented in include/kpnerf.h."""
    return kl.get_library().kpn_hg_filter_state_floats(ctypes.byref(_hg_filter_desc(N, H, W, cfg, 1e-5)))


def _hg_filter_tensors(tensors, cfg, device):
    shapes = hg_filter_shapes(cfg)
    if len(tensors) != len(shapes):
        raise ValueError(f"hg_filter: {len(shapes)} tensors, got {len(tensors)}")
    out = []
    for i, (t, shape) in enumerate(zip(tensors, shapes)):
        t = _dev(t.detach(), f"tensors[{i}]")
        if tuple(t.shape) != shape or t.device != device:
            raise ValueError(f"hg_filter: tensors[{i}] must be {shape} on {device}, got {tuple(t.shape)} on {t.device}")
        out.append(t)
    return out


def hg_filter_pack(tensors, cfg):
    """The packed copies of every convolution weight in one buffer (kpn_hg_filter_pack_device): per weight, in tensor order, what its
    layer's own packer gives (conv2d_s2_pack for conv1 and unpack1.conv, conv2d_pack for the others)."""
    L = kl.get_library()
    ts = _hg_filter_tensors(tensors, cfg, tensors[0].device)
    f = 4 << int(cfg[5])
    d = _hg_filter_desc(1, f, f, cfg, 1e-5)
    n = _desc_size(L, d, "kpn_hg_filter_packed_floats", "kpn_hg_filter_pack_device", "hg_filter: unsupported network")
    packed = torch.empty(n, dtype=_f32, device=ts[0].device)
    L.check(L.kpn_hg_filter_pack_device(ctypes.byref(d), _pointer_array(ts), _p(packed), _stream()))
    return packed


def _hg_filter_check(L, d, packed, state, device):
    if packed.numel() != L.kpn_hg_filter_packed_floats(ctypes.byref(d)) or packed.dtype != _f32 or packed.device != device:
        raise ValueError("packed does not belong to this network (hg_filter_pack)")
    if state is not None and (state.numel() != L.kpn_hg_filter_state_floats(ctypes.byref(d)) or state.dtype != _f32 or state.device != device):
        raise ValueError("state does not belong to this network (hg_filter_forward)")


def hg_filter_forward(x, tensors, packed, cfg, eps):
    """HGFilterV2(x) for packed = hg_filter_pack(tensors, cfg) (kpn_hg_filter_forward).  x: contiguous NCHW (N, in_ch, H, W).  Returns
    (out (N, out_ch, H / 4, W / 4) channels_last, x_hd (N, out_ch_hd, H, W) channels_last, state): state holds what hg_filter_backward
    reads - the layout of include/kpnerf.h."""
    L = kl.get_library()
    x = _res_encoder_x(x)
    N, in_ch, H, W = x.shape
    if in_ch != int(cfg[0]):
        raise ValueError(f"x must have {int(cfg[0])} channels, got {in_ch}")
    d = _hg_filter_desc(N, H, W, cfg, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_HG_FILTER_WORKSPACE)
    ts = _hg_filter_tensors(tensors, cfg, x.device)
    _hg_filter_check(L, d, packed, None, x.device)
    out = torch.empty(N, H // 4, W // 4, int(cfg[8]), dtype=_f32, device=x.device)
    x_hd = torch.empty(N, H, W, int(cfg[7]), dtype=_f32, device=x.device)
    state = torch.empty(L.kpn_hg_filter_state_floats(ctypes.byref(d)), dtype=_f32, device=x.device)
    pr = kl.HgFilterParams()
    ptrs = _pointer_array(ts)
    pr.tensors, pr.packed = ptrs, packed.data_ptr()
    L.check(L.kpn_hg_filter_forward(ctypes.byref(d), _p(x), ctypes.byref(pr), _p(out), _p(x_hd), _p(state), _p(ws), nb, _stream()))
    return out.permute(0, 3, 1, 2), x_hd.permute(0, 3, 1, 2), state


def hg_filter_backward(x, d_out, d_x_hd, tensors, packed, state, cfg, eps, want=None):
    """[gradient or None] per tensor of hg_filter_forward for the output gradients d_out (N, out_ch, H / 4, W / 4) and d_x_hd
    (N, out_ch_hd, H, W), channels_last; either may be None (that branch contributes nothing), not both (kpn_hg_filter_backward).
    ``want`` has one flag per tensor (default: all); what is not wanted is None, and only the legs a wanted gradient needs are launched."""
    L = kl.get_library()
    x = _res_encoder_x(x)
    N, _, H, W = x.shape
    shapes = hg_filter_shapes(cfg)
    want = [True] * len(shapes) if want is None else [bool(w) for w in want]
    if len(want) != len(shapes):
        raise ValueError(f"hg_filter: {len(shapes)} tensors, got {len(want)} entries of want")
    if d_out is None and d_x_hd is None:
        raise ValueError("hg_filter: d_out and d_x_hd are both None")
    for g, name, shape in ((d_out, "d_out", (N, int(cfg[8]), H // 4, W // 4)), (d_x_hd, "d_x_hd", (N, int(cfg[7]), H, W))):
        if g is not None and tuple(_channels_last(g, name).shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(g.shape)}")
    d = _hg_filter_desc(N, H, W, cfg, eps)
    ws, nb = _desc_workspace(L, d, x.device, *_HG_FILTER_WORKSPACE)
    ts = _hg_filter_tensors(tensors, cfg, x.device)
    _hg_filter_check(L, d, packed, state, x.device)
    out = [torch.empty(shape, dtype=_f32, device=x.device) if w else None for shape, w in zip(shapes, want)]
    if any(want):
        pr, gr = kl.HgFilterParams(), kl.HgFilterGrads()
        ptrs, gptrs = _pointer_array(ts), _pointer_array(out)
        pr.tensors, pr.packed, gr.tensors = ptrs, packed.data_ptr(), gptrs
        L.check(L.kpn_hg_filter_backward(ctypes.byref(d), _p(x), _p(d_out), _p(d_x_hd), ctypes.byref(pr), _p(state.contiguous()), ctypes.byref(gr),
                                         _p(ws), nb, _stream()))
    return out


# ------------------------------------------------------------------------------------------------
# The two resampling steps of an HourGlass and their gradients (kpn_avg_pool2_* / kpn_upsample2x_add_*; avg_pool2d(x, 2, stride=2)
# and skip + interpolate(low, scale_factor=2, mode="bicubic", align_corners=True) with their autograd, reference
# src/utils.py:287-306).  Activations are channels_last tensors of logical shape (N, C, H, W).
def _resample_desc(N, h, w, C):
    if C % 4:
        raise ValueError(f"channels must be a multiple of 4, got {C}")
    d = kl.ResampleDesc()
    d.N, d.h, d.w, d.C = int(N), int(h), int(w), int(C)
    return d


def _resample_out(N, C, H, W, device):
    return torch.empty(N, C, H, W, dtype=_f32, device=device, memory_format=torch.channels_last)


def avg_pool2_forward(x):
    """avg_pool2d(x, 2, stride=2) (kpn_avg_pool2_forward).  x: (N, C, 2h, 2w) channels_last; returns (N, C, h, w) channels_last."""
    L = kl.get_library()
    x = _channels_last(x, "x")
    N, C, H, W = x.shape
    if H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"x must have even, positive height and width, got {tuple(x.shape)}")
    d = _resample_desc(N, H // 2, W // 2, C)
    y = _resample_out(N, C, H // 2, W // 2, x.device)
    L.check(L.kpn_avg_pool2_forward(ctypes.byref(d), _p(x), _p(y), _stream()))
    return y


def avg_pool2_backward(dy):
    """dx of avg_pool2_forward for the output gradient dy (N, C, h, w) channels_last (kpn_avg_pool2_backward): (N, C, 2h, 2w)
    channels_last, 0.25 dy under every pixel of a window."""
    L = kl.get_library()
    dy = _channels_last(dy, "dy")
    N, C, h, w = dy.shape
    d = _resample_desc(N, h, w, C)
    dx = _resample_out(N, C, 2 * h, 2 * w, dy.device)
    L.check(L.kpn_avg_pool2_backward(ctypes.byref(d), _p(dy), _p(dx), _stream()))
    return dx


def upsample2x_add_forward(low, skip=None, out=None):
    """skip + interpolate(low, scale_factor=2, mode="bicubic", align_corners=True), or the interpolation alone for skip = None
    (kpn_upsample2x_add_forward).  low: (N, C, h, w), skip: (N, C, 2h, 2w), both channels_last.  out: None (a new tensor) or a
    channels_last (N, C, 2h, 2w) tensor to write, which may be skip itself.  Returns (N, C, 2h, 2w) channels_last."""
    L = kl.get_library()
    low = _channels_last(low, "low")
    N, C, h, w = low.shape
    high = (N, C, 2 * h, 2 * w)
    if skip is not None:
        skip = _channels_last(skip, "skip")
        if tuple(skip.shape) != high:
            raise ValueError(f"skip must be {high}, got {tuple(skip.shape)}")
    if out is not None:
        out = _channels_last(out, "out")
        if tuple(out.shape) != high:
            raise ValueError(f"out must be {high}, got {tuple(out.shape)}")
    d = _resample_desc(N, h, w, C)
    y = _resample_out(N, C, 2 * h, 2 * w, low.device) if out is None else out
    L.check(L.kpn_upsample2x_add_forward(ctypes.byref(d), _p(low), _p(skip), _p(y), _stream()))
    return y


def upsample2x_add_backward(dy):
    """d_low of upsample2x_add_forward for the output gradient dy (N, C, 2h, 2w) channels_last (kpn_upsample2x_add_backward):
    (N, C, h, w) channels_last, a gather in a fixed order - bit-identical from run to run.  The gradient of skip is dy itself."""
    L = kl.get_library()
    dy = _channels_last(dy, "dy")
    N, C, H, W = dy.shape
    if H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"dy must have even, positive height and width, got {tuple(dy.shape)}")
    d = _resample_desc(N, H // 2, W // 2, C)
    d_low = _resample_out(N, C, H // 2, W // 2, dy.device)
    L.check(L.kpn_upsample2x_add_backward(ctypes.byref(d), _p(dy), _p(d_low), _stream()))
    return d_low
