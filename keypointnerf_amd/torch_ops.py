"""PyTorch custom operators (``torch.ops.kpnerf.*``) over the gfx950 library.

BASELINE.json's north star asks for the kernels to be "exposed to Python through PyTorch-ROCm custom ops";
these are thin ``torch.library.custom_op`` registrations (device type "cuda" = HIP on ROCm) around
``keypointnerf_amd.ops`` with shape-only fake implementations, so the ops compose with torch.compile /
FakeTensor tracing and show up in profiler traces under their own names.  There is no CPU kernel registered:
calling them on CPU tensors raises NotImplementedError from the dispatcher.

    torch.ops.kpnerf.rgba2out(rgba, z)                       -> (color, depth, alpha, contrib, sdf)
    torch.ops.kpnerf.importance_sample(contrib, z, n, u?)    -> samples           (u=None: uniform linspace)
    torch.ops.kpnerf.ray_bbox_intersection(bounds, orig, d)  -> (near, far, hit)
    torch.ops.kpnerf.field_query(scene_ws, scene_dims, scene_scalars, weights, pts, view, mode) -> (out, valid)

    torch.ops.kpnerf.render_rays(scene_ws, scene_dims, scene_scalars, weights, K, RT, bounds, znear, zfar, grid,
                                 n_coarse, n_fine, fine) -> (tex_fg, depth, alpha, tex_fg_fine, depth_fine, alpha_fine, sdf)
    torch.ops.kpnerf.render_rays_train(plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask?, scene_scalars, K, RT,
                                       bounds, znear, zfar, pix, u_c, u_f, noise_c?, noise_f?, keep_c, keep_f, noise_std,
                                       n_coarse, n_fine) -> the same seven outputs, DIFFERENTIABLE

    torch.ops.kpnerf.fold_params(tensors) -> plain   the 44 live hot-path tensors (weights.hot_tensors) -> the flat effective
                                 parameters in one launch, DIFFERENTIABLE w.r.t. every tensor (one more launch in the backward)

    torch.ops.kpnerf.fold_params_shape(tensors, n_kpt, sp_level) -> plain   the same for a model with n_kpt <= 24 keypoints and
                                 sp_level <= 3 octaves, whose first weight_v is (128, (1 + 2 sp_level) n_kpt + 64): plain is the
                                 kernels' 24 / 3 vector, zeros in the padded columns; one launch each way
    torch.ops.kpnerf.widen_plain(narrow, n_kpt, sp_level) -> plain   the narrow plain vector of such a model (torch's own weight-norm
                                 fold + cat) -> the kernels' vector, DIFFERENTIABLE (the backward gathers: kpn_narrow_plain_grad)

``scene_ws / scene_dims / scene_scalars`` come from ``ops.PreparedScene.as_op_args()``.

    torch.ops.kpnerf.pix_l1_loss(src, tar, lam) -> (loss, d loss / d src)   the L1 terms of the training loss, DIFFERENTIABLE
    torch.ops.kpnerf.vgg_loss(x, y, packed, consts, lam) -> (loss, d loss / d x)   the perceptual term, DIFFERENTIABLE w.r.t. x
    torch.ops.kpnerf.train_loss(tex?, tex_fine?, tar, alpha?, alpha_fine?, tar_alpha?, [l1_c, l1, l2, lp, mloss])
                                 -> (terms (6,), d_tex, d_tex_fine (3, ...), d_alpha, d_alpha_fine)   every pixel and mask term of
                                 the training loss in one launch, DIFFERENTIABLE w.r.t. tex, tex_fine, alpha, alpha_fine

    torch.ops.kpnerf.geo_encode(img, packed, [ds, out_ch, out_ch_hd], eps) -> (feat, feat_hd)   the geometry encoder, channels-last,
    torch.ops.kpnerf.tex_encode(img, packed, [ds, ngf, n_down, n_blocks, n_up, out_ch], eps) -> feat   the texture encoder; FORWARD ONLY

    torch.ops.kpnerf.conv2d(x, weight, bias?, padding) -> y   one stride-1 convolution (k in {1, 3, 5}, zero padding, channels multiples
                                 of 4), channels-last result, DIFFERENTIABLE w.r.t. x, weight and bias (kpn_conv2d_forward / _backward)
    torch.ops.kpnerf.conv2d_down2(x, weight, bias?) -> y   Conv2d(k 3, stride 2, pad 1) or, for a 7x7 weight, the stem Conv2d(k 7,
                                 stride 2, pad 3) on an NCHW tensor; DIFFERENTIABLE (the stem w.r.t. weight and bias only)
    torch.ops.kpnerf.conv_transpose2d_up2(x, weight, bias?) -> y   ConvTranspose2d(k 3, stride 2, pad 1, output_padding 1),
                                 DIFFERENTIABLE w.r.t. x, weight and bias (kpn_conv2d_s2_forward / _backward)
    torch.ops.kpnerf.conv2d_replicate(x, weight, bias?) -> y   ReplicationPad2d(k // 2) + Conv2d(k) for a 3x3 or 7x7 weight (a 7x7 weight
                                 with at most 4 input channels: the stem, on an NCHW tensor); DIFFERENTIABLE (the stem w.r.t. weight and
                                 bias only) (kpn_conv2d_rp_forward / _backward); the input gradient is a gather without atomics
    torch.ops.kpnerf.group_norm(x, weight?, bias?, groups, eps, relu) -> y   GroupNorm / InstanceNorm2d [+ ReLU] (C a power of two in
                                 4 .. 1024), channels-last result, DIFFERENTIABLE w.r.t. x, weight and bias (kpn_group_norm_forward /
                                 _backward); y is not kept for the backward and may be overwritten in place
    torch.ops.kpnerf.conv2d_arith(x, weight, bias?, padding, arith) / conv_block_arith(x, tensors, eps, arith)   conv2d / conv_block
                                 (below) with the arithmetic of the convolutions' GEMMs as an argument: 0 = fp32 MFMA (the same
                                 bits), 1 = three bf16 pieces per operand (kpn_conv2d_ex_* / kpn_conv_block_ex_*)
    torch.ops.kpnerf.conv_block(x, tensors, eps) -> y   a whole ConvBlock(cin, cout, norm="group") as ONE autograd node: tensors =
                                 [bn1.weight, bn1.bias, conv1.weight, ... bn3 ..., conv3.weight (, bn4.weight, bn4.bias, downsample
                                 weight)]; channels-last result, DIFFERENTIABLE w.r.t. x and every tensor (kpn_conv_block_forward /
                                 _backward); keeps x and 3/4 of a y-sized tensor for the backward, never y or a normalised tensor
    torch.ops.kpnerf.res_encoder(x, tensors, n_down, n_blocks, n_up, eps) -> y   a whole ResBlkEncoder(norm="instance") as ONE autograd
                                 node: tensors = [weight, bias] per convolution in module order; x is the NCHW image; channels-last
                                 result, DIFFERENTIABLE w.r.t. every tensor, not x (kpn_res_encoder_forward / _backward); keeps x, the
                                 convolution outputs and the ResBlk sums for the backward, never a normalised or padded tensor
    torch.ops.kpnerf.hg_filter(x, tensors, depth, eps) -> [out, x_hd]   a whole HGFilterV2(n_stack=1, hd=False, norm="group") as ONE
                                 autograd node: tensors in the order of include/kpnerf.h; x is the NCHW image; channels-last results,
                                 DIFFERENTIABLE w.r.t. every tensor, not x (kpn_hg_filter_forward / _backward); keeps x, the block
                                 inputs and states, the pooled tensors and two convolution outputs, never a normalised tensor but
                                 relu(bn1(conv1 x)); the fan-in sums of the backward run in its kernels
    torch.ops.kpnerf.avg_pool2(x) -> y   avg_pool2d(x, 2, stride=2) (C a multiple of 4, even H and W), channels-last result,
                                 DIFFERENTIABLE w.r.t. x (kpn_avg_pool2_forward / _backward)
    torch.ops.kpnerf.upsample2x_add(low, skip?) -> y   skip + bicubic x2 of low (align_corners=True; C a multiple of 4), channels-last
                                 result, DIFFERENTIABLE w.r.t. low and skip (kpn_upsample2x_add_forward / _backward); the backward is a
                                 gather without atomics: bit-identical from run to run

``rgba2out`` and ``render_rays_train`` carry ``register_autograd`` formulas whose backward is itself a registered op
(``kpnerf::rgba2out_backward``, ``kpnerf::render_rays_train_backward`` = kpn_render_rays_train_backward): gradients reach
the flat effective-parameter vector ``plain`` (and from there ``weight_g`` / ``weight_v`` / ``bias`` / ``ani_al`` through
``weights.plain_tensor_from_module``) and the three encoder feature maps.  This is the op the training drop-in calls.
"""
import collections
import ctypes
from typing import List, Optional, Tuple

import torch

from . import lib as kl
from . import ops

_lib = torch.library


# An operator returns tensors only: a gradient that is not wanted (or lacks its input) travels as an empty tensor, and the autograd
# formula turns what its mask did not ask for back into None.
def _empty_for_none(like, *grads):
    return tuple(like.new_empty(0) if g is None else g for g in grads)


def _none_unless(mask, *grads):
    return tuple(g if m else None for g, m in zip(grads, mask))


@_lib.custom_op("kpnerf::rgba2out", mutates_args=(), device_types="cuda")
def rgba2out(rgba: torch.Tensor, z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.rgba2out(rgba, z)


@rgba2out.register_fake
def _(rgba, z):
    B, R, S = z.shape
    f = lambda *s: rgba.new_empty(s)
    return f(B, R, 3), f(B, R), f(B, R), f(B, R, S), f(B, R)


@_lib.custom_op("kpnerf::rgba2out_backward", mutates_args=(), device_types="cuda")
def rgba2out_backward(rgba: torch.Tensor, z: torch.Tensor, d_color: Optional[torch.Tensor], d_depth: Optional[torch.Tensor],
                      d_alpha: Optional[torch.Tensor], d_sdf: Optional[torch.Tensor]) -> torch.Tensor:
    return ops.rgba2out_backward(rgba, z, d_color, d_depth, d_alpha, d_sdf)


@rgba2out_backward.register_fake
def _(rgba, z, d_color, d_depth, d_alpha, d_sdf):
    return torch.empty_like(rgba)


def _rgba2out_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)
    ctx.set_materialize_grads(False)


def _rgba2out_bwd(ctx, d_color, d_depth, d_alpha, d_contrib, d_sdf):
    # contrib and z carry no gradient in the reference (the sampler runs under no_grad, src/model.py:1038,1118)
    rgba, z = ctx.saved_tensors
    return torch.ops.kpnerf.rgba2out_backward(rgba, z, d_color, d_depth, d_alpha, d_sdf), None


rgba2out.register_autograd(_rgba2out_bwd, setup_context=_rgba2out_setup)


@_lib.custom_op("kpnerf::importance_sample", mutates_args=(), device_types="cuda")
def importance_sample(contrib: torch.Tensor, z: torch.Tensor, n: int, u: Optional[torch.Tensor] = None) -> torch.Tensor:
    return ops.importance_sample(contrib, z, n, uniform=u is None, u=u)


@importance_sample.register_fake
def _(contrib, z, n, u=None):
    return contrib.new_empty(contrib.shape[0], contrib.shape[1], n)


@_lib.custom_op("kpnerf::ray_bbox_intersection", mutates_args=(), device_types="cuda")
def ray_bbox_intersection(bounds: torch.Tensor, orig: torch.Tensor, direct: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.ray_bbox_intersection(bounds, orig, direct)


@ray_bbox_intersection.register_fake
def _(bounds, orig, direct):
    R = direct.shape[-2]
    return direct.new_empty(1, R, 1), direct.new_empty(1, R, 1), direct.new_empty(1, R, 1, dtype=torch.bool)


class _SceneView:
    """A PreparedScene rebuilt from op arguments (workspace tensor + plain ints/floats)."""

    def __init__(self, ws, dims, scalars):
        d = kl.SceneDesc()
        (d.n_views, d.src_h, d.src_w, d.geo0_h, d.geo0_w, d.geo1_h, d.geo1_w, d.tex_h, d.tex_w, d.disable_fg_mask) = dims
        d.znear, d.zfar, d.nml_scale, d.sigma = scalars
        # the raw NCHW inputs are only read by kpn_scene_prepare; the query reads the prepared workspace
        for k in ("KRT", "extrin", "kpt3d", "img", "fg_mask", "geo0", "geo1", "tex"):
            setattr(d, k, ws.data_ptr())
        self.desc, self.ws, self.n_views = d, ws, dims[0]


@_lib.custom_op("kpnerf::field_query", mutates_args=(), device_types="cuda")
def field_query(scene_ws: torch.Tensor, scene_dims: List[int], scene_scalars: List[float], weights: torch.Tensor,
                pts: torch.Tensor, view: torch.Tensor, mode: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.query(_SceneView(scene_ws, list(scene_dims), list(scene_scalars)), ops.PackedWeights.wrap(weights), pts, view, mode=mode)


@field_query.register_fake
def _(scene_ws, scene_dims, scene_scalars, weights, pts, view, mode):
    N = pts.shape[-2]
    return pts.new_empty(1, N, 5), pts.new_empty(1, N, 1, dtype=torch.bool)


_OUT7 = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]
_OUT8 = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]
_OUT_KEYS = ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf")


@_lib.custom_op("kpnerf::render_rays", mutates_args=(), device_types="cuda")
def render_rays(scene_ws: torch.Tensor, scene_dims: List[int], scene_scalars: List[float], weights: torch.Tensor,
                K: torch.Tensor, RT: torch.Tensor, bounds: torch.Tensor, znear: float, zfar: float, grid: List[int],
                n_coarse: int, n_fine: int, fine: bool) -> _OUT7:
    """Eval branch of batch_render_pifu_nerf (kpn_render_rays) for the pixel grid (x0, y0, step, nx, ny).  With
    fine=False the four fine outputs are empty tensors."""
    sv = _SceneView(scene_ws, list(scene_dims), list(scene_scalars))
    out = ops.render_rays(sv, ops.PackedWeights.wrap(weights), {"K": K, "RT": RT, "znear": znear, "zfar": zfar}, bounds, grid=tuple(grid),
                          n_coarse=n_coarse, n_fine=n_fine, fine=fine)
    return tuple(out[k] if k in out else scene_ws.new_empty(0) for k in _OUT_KEYS)


@render_rays.register_fake
def _(scene_ws, scene_dims, scene_scalars, weights, K, RT, bounds, znear, zfar, grid, n_coarse, n_fine, fine):
    nx, ny = grid[3], grid[4]
    f = lambda *s: scene_ws.new_empty(s)
    e = lambda *s: f(*s) if fine else f(0)
    return f(1, 3, ny, nx), f(1, ny, nx), f(1, ny, nx), e(1, 3, ny, nx), e(1, ny, nx), e(1, ny, nx), e(1, ny, nx)


def _raw_scene(geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scal):
    V, _, H, W = img.shape
    cam = {"KRT": KRT, "width": W, "height": H, "znear": scal[0], "zfar": scal[1], "nml_scale": scal[2]}
    return ops.PreparedScene(img, cam, [geo0, geo1], tex, {"kpt3d": kpt3d, "extrin": extrin}, fg_mask,
                             disable_fg_mask=fg_mask is None, sigma=scal[3])


# One training iteration calls the forward op and then the backward op with the SAME parameters and maps: the packed weights
# (weight-norm fold + operand order + fp16 / bf16 streams) and the prepared scene (NCHW -> NHWC of every map) of the forward call
# are kept for the backward call instead of being built twice.  Autograd hands the backward op NEW tensor objects over the same
# storage, so the key is (storage address, version counter, shape, device) per tensor — and the entry HOLDS the forward call's
# input tensors: while it lives their storage cannot be freed, so an equal address means the same storage, and an in-place change
# in between moves the version counter: a miss, never a stale hit.  The backward op drops the entry when it is done: nothing of
# an iteration stays resident after it.
# ONE entry for the process, behind a lock (round 5; an advisor finding): for CUDA tensors autograd runs the backward op on its
# device worker thread, not on the thread that ran the forward — a thread-local entry was never found by the backward (which then
# built the scene and the packed weights a second time, the very work the cache exists to avoid) and never cleared on the forward's
# thread.  Two threads training different models in one process take turns at the single entry: a miss, never a wrong hit.
import threading


class _IterCache:
    lock = threading.Lock()
    key = scene = w = pinned = None
    seed = None            # (key of plain, plain, packed operands) left by seed_packed for the next miss
    hits = misses = 0      # observable by the tests


def _tensor_key(t):
    if t is None:
        return None
    return (t.data_ptr(), t._version if not t.is_inference() else -1, tuple(t.shape), str(t.device), t.dtype)


def _iter_cache_clear():
    with _IterCache.lock:
        _IterCache.key = _IterCache.scene = _IterCache.w = _IterCache.pinned = _IterCache.seed = None


def seed_packed(plain, w):
    """The drop-in with native_params=True holds the packed operands of the current parameter version: it leaves them in the
    iteration cache for the render_rays_train call it makes next with this very `plain`, which then prepares only the scene.  The
    seed holds `plain`, so an equal (storage address, version) key means the same values; any other call drops it."""
    with _IterCache.lock:
        _IterCache.seed = (_tensor_key(plain), plain, w)


def _take_seed(plain):
    with _IterCache.lock:
        seed, _IterCache.seed = _IterCache.seed, None
    return seed[2] if seed is not None and seed[0] == _tensor_key(plain) else None


def _scene_and_weights(plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scal):
    tensors = (plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask)
    key = tuple(_tensor_key(t) for t in tensors) + (tuple(scal),)
    with _IterCache.lock:
        if not any(t is not None and t.is_inference() for t in tensors) and key == _IterCache.key:
            _IterCache.hits += 1
            return _IterCache.scene, _IterCache.w
    scene = _raw_scene(geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scal)
    w = _take_seed(plain)
    if w is None:
        w = ops.PackedWeights.from_plain(plain, device=geo0.device)
    with _IterCache.lock:
        _IterCache.misses += 1
        _IterCache.key, _IterCache.scene, _IterCache.w, _IterCache.pinned = key, scene, w, tensors
    return scene, w


@_lib.custom_op("kpnerf::render_rays_train", mutates_args=(), device_types="cuda")
def render_rays_train(plain: torch.Tensor, geo0: torch.Tensor, geo1: torch.Tensor, tex: torch.Tensor, img: torch.Tensor,
                      KRT: torch.Tensor, extrin: torch.Tensor, kpt3d: torch.Tensor, fg_mask: Optional[torch.Tensor],
                      scene_scalars: List[float], K: torch.Tensor, RT: torch.Tensor, bounds: torch.Tensor, znear: float,
                      zfar: float, pix: torch.Tensor, u_c: torch.Tensor, u_f: torch.Tensor, noise_c: Optional[torch.Tensor],
                      noise_f: Optional[torch.Tensor], keep_c: int, keep_f: int, noise_std: float, n_coarse: int,
                      n_fine: int, keep_state: bool = False) -> _OUT8:
    """The stochastic (`uniform=False`) branch of batch_render_pifu_nerf with every draw an input (kpn_render_rays_train).
    plain: flat effective parameters (weights.flatten_plain layout); geo0/geo1/tex: the encoders' NCHW maps; fg_mask None =
    disable_fg_mask; scene_scalars = [znear, zfar, nml_scale, sigma] of the SOURCE cameras / spatial encoder.
    Outputs: (1,3,R) / (1,R) tensors in the order of `pix`, then the pass state (uint8; empty unless keep_state): with it
    the backward op starts from the forward's rays, depths, field values, valid lists and rows instead of repeating the
    forward (kpn_render_rays_train_keep / kpn_render_rays_train_backward_kept)."""
    scene, w = _scene_and_weights(plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, list(scene_scalars))
    res = ops.render_rays_train(scene, w, {"K": K, "RT": RT, "znear": znear, "zfar": zfar}, bounds, pix, u_c, u_f, keep_c, keep_f,
                                noise_coarse=noise_c, noise_fine=noise_f, rand_noise_std=noise_std, n_coarse=n_coarse,
                                n_fine=n_fine, keep_state=keep_state)
    out, state = res if keep_state else (res, torch.empty(0, dtype=torch.uint8, device=geo0.device))
    return tuple(out[k].clone() for k in _OUT_KEYS) + (state,)


@render_rays_train.register_fake
def _(plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scene_scalars, K, RT, bounds, znear, zfar, pix, u_c, u_f, noise_c,
      noise_f, keep_c, keep_f, noise_std, n_coarse, n_fine, keep_state=False):
    R = pix.shape[0]
    f = lambda *s: geo0.new_empty(s)
    return f(1, 3, R), f(1, R), f(1, R), f(1, 3, R), f(1, R), f(1, R), f(1, R), geo0.new_empty(0, dtype=torch.uint8)


def _train_backward(want_kpt, *args):
    """the body of the two backward operators below over their 33 arguments: the 25 of the forward, the seven output gradients, the pass state"""
    (plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scene_scalars, K, RT, bounds, znear, zfar, pix, u_c, u_f, noise_c, noise_f,
     keep_c, keep_f, noise_std, n_coarse, n_fine), d_outs, state = args[:25], args[25:32], args[32]
    scene, w = _scene_and_weights(plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, list(scene_scalars))
    d_plain, d_g0, d_g1, d_tx, *d_kpt = ops.render_rays_train_backward(
        scene, w, {"K": K, "RT": RT, "znear": znear, "zfar": zfar}, bounds, pix, u_c, u_f, keep_c, keep_f, dict(zip(_OUT_KEYS, d_outs)),
        noise_coarse=noise_c, noise_fine=noise_f, rand_noise_std=noise_std, n_coarse=n_coarse, n_fine=n_fine, state=state,
        want_kpt=want_kpt)
    _iter_cache_clear()   # stream-ordered: the launches above hold nothing but device pointers the allocator keeps valid for them
    return (d_plain, d_g0.contiguous(), d_g1.contiguous(), d_tx.contiguous()) + tuple(g.reshape(kpt3d.shape).to(kpt3d.dtype) for g in d_kpt)


def _train_backward_fake(n_results):
    def fake(plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, *rest, **named):
        return tuple(torch.empty_like(t) for t in (plain, geo0, geo1, tex, kpt3d)[:n_results])
    return fake


@_lib.custom_op("kpnerf::render_rays_train_backward", mutates_args=(), device_types="cuda")
def render_rays_train_backward(plain: torch.Tensor, geo0: torch.Tensor, geo1: torch.Tensor, tex: torch.Tensor, img: torch.Tensor,
                               KRT: torch.Tensor, extrin: torch.Tensor, kpt3d: torch.Tensor, fg_mask: Optional[torch.Tensor],
                               scene_scalars: List[float], K: torch.Tensor, RT: torch.Tensor, bounds: torch.Tensor,
                               znear: float, zfar: float, pix: torch.Tensor, u_c: torch.Tensor, u_f: torch.Tensor,
                               noise_c: Optional[torch.Tensor], noise_f: Optional[torch.Tensor], keep_c: int, keep_f: int,
                               noise_std: float, n_coarse: int, n_fine: int, d_tex_fg: Optional[torch.Tensor],
                               d_depth: Optional[torch.Tensor], d_alpha: Optional[torch.Tensor],
                               d_tex_fg_fine: Optional[torch.Tensor], d_depth_fine: Optional[torch.Tensor],
                               d_alpha_fine: Optional[torch.Tensor], d_sdf: Optional[torch.Tensor],
                               state: Optional[torch.Tensor] = None
                               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """loss.backward() through render_rays_train (kpn_render_rays_train_backward) -> (d_plain, d_geo0, d_geo1, d_tex),
    the map gradients NCHW like the maps."""
    return _train_backward(False, plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scene_scalars, K, RT, bounds, znear, zfar, pix,
                           u_c, u_f, noise_c, noise_f, keep_c, keep_f, noise_std, n_coarse, n_fine, d_tex_fg, d_depth, d_alpha,
                           d_tex_fg_fine, d_depth_fine, d_alpha_fine, d_sdf, state)


render_rays_train_backward.register_fake(_train_backward_fake(4))


@_lib.custom_op("kpnerf::render_rays_train_backward_kpt", mutates_args=(), device_types="cuda")
def render_rays_train_backward_kpt(plain: torch.Tensor, geo0: torch.Tensor, geo1: torch.Tensor, tex: torch.Tensor, img: torch.Tensor,
                                   KRT: torch.Tensor, extrin: torch.Tensor, kpt3d: torch.Tensor, fg_mask: Optional[torch.Tensor],
                                   scene_scalars: List[float], K: torch.Tensor, RT: torch.Tensor, bounds: torch.Tensor,
                                   znear: float, zfar: float, pix: torch.Tensor, u_c: torch.Tensor, u_f: torch.Tensor,
                                   noise_c: Optional[torch.Tensor], noise_f: Optional[torch.Tensor], keep_c: int, keep_f: int,
                                   noise_std: float, n_coarse: int, n_fine: int, d_tex_fg: Optional[torch.Tensor],
                                   d_depth: Optional[torch.Tensor], d_alpha: Optional[torch.Tensor],
                                   d_tex_fg_fine: Optional[torch.Tensor], d_depth_fine: Optional[torch.Tensor],
                                   d_alpha_fine: Optional[torch.Tensor], d_sdf: Optional[torch.Tensor],
                                   state: Optional[torch.Tensor] = None
                                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """render_rays_train_backward with a fifth result, d loss / d kpt3d shaped like kpt3d (kpn_render_rays_train_backward[_kept]_kpt;
    what autograd derives through SpatialEncoder.forward, reference src/spatial.py:76-118)."""
    return _train_backward(True, plain, geo0, geo1, tex, img, KRT, extrin, kpt3d, fg_mask, scene_scalars, K, RT, bounds, znear, zfar, pix,
                           u_c, u_f, noise_c, noise_f, keep_c, keep_f, noise_std, n_coarse, n_fine, d_tex_fg, d_depth, d_alpha,
                           d_tex_fg_fine, d_depth_fine, d_alpha_fine, d_sdf, state)


render_rays_train_backward_kpt.register_fake(_train_backward_fake(5))


def _train_setup(ctx, inputs, output):
    # tensors go through save_for_backward, so that autograd's version-counter check raises if one of them (feature maps, the
    # flat parameters, the draws) or the kept pass state is modified in place between forward and backward — the state is only
    # valid for the values it was computed from; scalars stay on ctx
    args = list(inputs[:25])
    ctx.tensor_slots = [i for i, a in enumerate(args) if isinstance(a, torch.Tensor)]
    ctx.scalars = [None if isinstance(a, torch.Tensor) else a for a in args]
    ctx.save_for_backward(*[args[i] for i in ctx.tensor_slots], output[7])   # ... and the pass state (empty unless keep_state)
    ctx.n_inputs = len(inputs)
    ctx.set_materialize_grads(False)


def _train_bwd(ctx, *grads):
    saved = ctx.saved_tensors
    args = list(ctx.scalars)
    for i, t in zip(ctx.tensor_slots, saved[:-1]):
        args[i] = t
    state = saved[-1] if saved[-1].numel() > 0 else None
    # kpt3d needs a gradient (reference: autograd through src/spatial.py:76-118): the operator with the fifth result
    op = torch.ops.kpnerf.render_rays_train_backward_kpt if ctx.needs_input_grad[7] else torch.ops.kpnerf.render_rays_train_backward
    d_plain, d_g0, d_g1, d_tx, *d_kpt = op(*args, *[None if g is None else g.contiguous() for g in grads[:7]], state)
    return (d_plain, d_g0, d_g1, d_tx, None, None, None, *d_kpt) + (None,) * (ctx.n_inputs - 7 - len(d_kpt))


render_rays_train.register_autograd(_train_bwd, setup_context=_train_setup)


@_lib.custom_op("kpnerf::pix_l1_loss", mutates_args=(), device_types="cuda")
def pix_l1_loss(src: torch.Tensor, tar: torch.Tensor, lam: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lam * mean|src - tar|, d loss / d src) = the L1 term of the reference's pix_loss (src/utils.py:164-168) and the seed
    gradient autograd derives for it (kpn_pix_l1_loss).  Differentiable w.r.t. src."""
    loss, d = ops.pix_l1_loss(src, tar, lam, want_grad=True)
    return loss, d.reshape(src.shape)


@pix_l1_loss.register_fake
def _(src, tar, lam):
    return src.new_empty(()), torch.empty_like(src)


def _l1_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _l1_bwd(ctx, d_loss, _d_grad):
    (g,) = ctx.saved_tensors
    return g * d_loss, None, None


pix_l1_loss.register_autograd(_l1_bwd, setup_context=_l1_setup)


@_lib.custom_op("kpnerf::train_loss", mutates_args=(), device_types="cuda")
def train_loss(tex: Optional[torch.Tensor], tex_fine: Optional[torch.Tensor], tar: torch.Tensor, alpha: Optional[torch.Tensor],
               alpha_fine: Optional[torch.Tensor], tar_alpha: Optional[torch.Tensor], weights: List[float]
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The pixel and mask terms of compute_error_nerf (reference src/utils.py:108-171; kpn_train_loss), weights = [lambda_l1_c,
    lambda_l1, lambda_l2, lambda_lp, lambda_mloss]: terms (6,) = e_pix_c, e_pix_l1, e_pix_l2, e_pix_lp, mask_loss_c, mask_loss_f
    (0 for a term that is switched off or lacks an input) and the seed gradients autograd derives for them — d_tex, d_tex_fine
    (3, ...: l1 / l2 / lp apart), d_alpha, d_alpha_fine; an absent input's gradient is an empty tensor, a skipped term's part is
    uninitialised.  Differentiable w.r.t. tex, tex_fine, alpha, alpha_fine; the backward launches no kernel of the library."""
    terms, d_x, d_xf, d_a, d_af = ops.train_loss(tex, tex_fine, tar, alpha, alpha_fine, tar_alpha, weights, want_grad=True)
    return (terms,) + _empty_for_none(terms, d_x, d_xf, d_a, d_af)


@train_loss.register_fake
def _(tex, tex_fine, tar, alpha, alpha_fine, tar_alpha, weights):
    like = lambda v, *lead: tar.new_empty(0) if v is None else tar.new_empty(*lead, *v.shape)
    return tar.new_empty(6), like(tex), like(tex_fine, 3), like(alpha), like(alpha_fine)


def _train_loss_active(inputs):
    """which of the six terms the kernel evaluated (kpn_train_loss's rule: weight > 0 and every input present)"""
    tex, tex_fine, tar, alpha, alpha_fine, tar_alpha, w = inputs
    return (tex is not None and w[0] > 0.0, tex_fine is not None and w[1] > 0.0, tex_fine is not None and w[2] > 0.0,
            tex_fine is not None and w[3] > 0.0, alpha is not None and tar_alpha is not None and w[4] > 0.0,
            alpha_fine is not None and tar_alpha is not None and w[4] > 0.0)


def _train_loss_setup(ctx, inputs, output):
    ctx.active = _train_loss_active(inputs)
    ctx.save_for_backward(*output[1:])


def _train_loss_bwd(ctx, d_terms, *_d_grads):
    d_x, d_xf, d_a, d_af = ctx.saved_tensors
    on = ctx.active
    g = d_terms.unbind(0)
    g_x = d_x * g[0] if on[0] else None
    g_xf = None
    for k in range(3):                                   # the three fine pixel terms, each by its own upstream gradient
        if on[1 + k]:
            g_xf = d_xf[k] * g[1 + k] if g_xf is None else torch.addcmul(g_xf, d_xf[k], g[1 + k])
    g_a = d_a * g[4] if on[4] else None
    g_af = d_af * g[5] if on[5] else None
    return g_x, g_xf, None, g_a, g_af, None, None


train_loss.register_autograd(_train_loss_bwd, setup_context=_train_loss_setup)


@_lib.custom_op("kpnerf::vgg_loss", mutates_args=(), device_types="cuda")
def vgg_loss(x: torch.Tensor, y: torch.Tensor, packed: torch.Tensor, consts: List[float], lam: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lam * VGGLoss(x, y), d loss / d x) (reference src/utils.py:750-805, kpn_vgg_loss).  consts = mean[3] + std[3] + the four
    tap weights of the module; packed = ops.vgg_pack(...).  Differentiable w.r.t. x (y detached, VGG parameters frozen)."""
    loss, d, _ = ops.vgg_loss(x, y, packed, consts[0:3], consts[3:6], consts[6:10], lam, want_grad=True)
    return loss, d


@vgg_loss.register_fake
def _(x, y, packed, consts, lam):
    return x.new_empty(()), torch.empty_like(x)


def _vgg_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _vgg_bwd(ctx, d_loss, _d_grad):
    (g,) = ctx.saved_tensors
    return g * d_loss, None, None, None, None


vgg_loss.register_autograd(_vgg_bwd, setup_context=_vgg_setup)


@_lib.custom_op("kpnerf::fold_params_norms", mutates_args=(), device_types="cuda")
def fold_params_norms(tensors: List[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(plain, norms) of the 44 live hot-path tensors (kpn_fold_params): what torch.ops.kpnerf.fold_params returns, and the row
    norms its backward reads.  Differentiable w.r.t. every tensor through plain."""
    return ops.fold_params(tensors)


# The fake kernels, the setup context and the autograd backward serve the (n_kpt, sp_level) twins further down as well: ``shape`` is
# their two trailing arguments, or nothing.
def _fold_norms_fake(tensors, n_kpt=None, sp_level=None):
    L = kl.get_library()
    return tensors[0].new_empty(L.kpn_plain_weight_floats()), tensors[0].new_empty(L.kpn_fold_norm_floats())


fold_params_norms.register_fake(_fold_norms_fake)


@_lib.custom_op("kpnerf::fold_params_backward", mutates_args=(), device_types="cuda")
def fold_params_backward(tensors: List[torch.Tensor], norms: torch.Tensor, d_plain: torch.Tensor) -> List[torch.Tensor]:
    """One gradient per tensor of fold_params' input from d_plain (kpn_fold_params_backward, overwrite mode)."""
    return ops.fold_params_backward(tensors, norms, d_plain)


def _fold_backward_fake(tensors, norms, d_plain, n_kpt=None, sp_level=None):
    return [torch.empty_like(t) for t in tensors]


fold_params_backward.register_fake(_fold_backward_fake)


def _fold_setup(ctx, inputs, output):
    tensors, *ctx.shape = inputs
    ctx.save_for_backward(*tensors, output[1])
    ctx.set_materialize_grads(False)


def _fold_autograd(backward_op):
    def bwd(ctx, d_plain, _d_norms):
        *tensors, norms = ctx.saved_tensors
        nothing = (None,) * len(ctx.shape)
        if d_plain is None:
            return (None,) + nothing
        return (backward_op(list(tensors), norms, d_plain.contiguous(), *ctx.shape),) + nothing
    return bwd


fold_params_norms.register_autograd(_fold_autograd(torch.ops.kpnerf.fold_params_backward), setup_context=_fold_setup)

# torch.ops.kpnerf.fold_params(tensors) -> plain: fold_params_norms without the side buffer; it decomposes into that operator,
# whose autograd formula serves it
_fragment = torch.library.Library("kpnerf", "FRAGMENT")
_fragment.define("fold_params(Tensor[] tensors) -> Tensor")
_fragment.impl("fold_params", lambda tensors: torch.ops.kpnerf.fold_params_norms(tensors)[0], "CompositeImplicitAutograd")


# ---- keypoint sets: models with fewer keypoints / octaves than the kernels' 24 / 3 (include/kpnerf.h, "Keypoint sets") ----
@_lib.custom_op("kpnerf::widen_plain", mutates_args=(), device_types="cuda")
def widen_plain(narrow: torch.Tensor, n_kpt: int, sp_level: int) -> torch.Tensor:
    """The narrow plain vector of a (n_kpt, sp_level) model -> the kernels' plain vector (kpn_widen_plain, one launch): the first
    layer's columns scattered to their 24 / 3 places, zeros in the padded ones, everything else copied."""
    return ops.widen_plain(narrow, n_kpt, sp_level)


@widen_plain.register_fake
def _(narrow, n_kpt, sp_level):
    return narrow.new_empty(kl.get_library().kpn_plain_weight_floats())


@_lib.custom_op("kpnerf::narrow_plain_grad", mutates_args=(), device_types="cuda")
def narrow_plain_grad(d_plain: torch.Tensor, n_kpt: int, sp_level: int) -> torch.Tensor:
    """widen_plain's adjoint: the gradient of the plain vector gathered into the narrow one's (kpn_narrow_plain_grad)."""
    return ops.narrow_plain_grad(d_plain, n_kpt, sp_level)


@narrow_plain_grad.register_fake
def _(d_plain, n_kpt, sp_level):
    return d_plain.new_empty(kl.get_library().kpn_plain_weight_floats_shape(ctypes.byref(kl.FieldShape(n_kpt, sp_level))))


def _widen_setup(ctx, inputs, output):
    ctx.shape = (inputs[1], inputs[2])


def _widen_bwd(ctx, d_plain):
    return torch.ops.kpnerf.narrow_plain_grad(d_plain.contiguous(), *ctx.shape), None, None


widen_plain.register_autograd(_widen_bwd, setup_context=_widen_setup)


@_lib.custom_op("kpnerf::fold_params_norms_shape", mutates_args=(), device_types="cuda")
def fold_params_norms_shape(tensors: List[torch.Tensor], n_kpt: int, sp_level: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fold_params_norms for a (n_kpt, sp_level) model: tensors[1] is its narrow first weight_v (kpn_fold_params_shape)."""
    return ops.fold_params(tensors, shape=(n_kpt, sp_level))


fold_params_norms_shape.register_fake(_fold_norms_fake)


@_lib.custom_op("kpnerf::fold_params_backward_shape", mutates_args=(), device_types="cuda")
def fold_params_backward_shape(tensors: List[torch.Tensor], norms: torch.Tensor, d_plain: torch.Tensor, n_kpt: int,
                               sp_level: int) -> List[torch.Tensor]:
    """fold_params_backward for a (n_kpt, sp_level) model (kpn_fold_params_backward_shape, overwrite mode)."""
    return ops.fold_params_backward(tensors, norms, d_plain, shape=(n_kpt, sp_level))


fold_params_backward_shape.register_fake(_fold_backward_fake)
fold_params_norms_shape.register_autograd(_fold_autograd(torch.ops.kpnerf.fold_params_backward_shape), setup_context=_fold_setup)
_fragment.define("fold_params_shape(Tensor[] tensors, int n_kpt, int sp_level) -> Tensor")
_fragment.impl("fold_params_shape", lambda tensors, n_kpt, sp_level: torch.ops.kpnerf.fold_params_norms_shape(tensors, n_kpt, sp_level)[0],
               "CompositeImplicitAutograd")


def _encoder_no_autograd(ctx, inputs, output):
    raise RuntimeError("kpnerf::geo_encode / kpnerf::tex_encode are forward only: an input requires a gradient "
                       "(training runs the caller's encoder modules)")


def _encoder_bwd(ctx, *grads):
    raise RuntimeError("kpnerf::geo_encode / kpnerf::tex_encode have no backward")


@_lib.custom_op("kpnerf::geo_encode", mutates_args=(), device_types="cuda")
def geo_encode(img: torch.Tensor, packed: torch.Tensor, cfg: List[int], eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """HGFilterV2.forward(2 * avg_pool2d^ds(img) - 1) (reference src/utils.py:370-414, src/model.py:653-666; kpn_geo_encode).
    cfg = [ds, out_ch, out_ch_hd]; packed = ops.geo_encoder_pack(...).  Returns channels-last (V, h/4, w/4, out_ch) and
    (V, h, w, out_ch_hd).  No autograd formula: raises on inputs that require a gradient."""
    f, fhd, _ = ops.geo_encode(img, packed, cfg[0], cfg[1], cfg[2], eps)
    return f, fhd


@geo_encode.register_fake
def _(img, packed, cfg, eps):
    V, h, w = img.shape[0], img.shape[2] >> cfg[0], img.shape[3] >> cfg[0]
    return img.new_empty(V, h // 4, w // 4, cfg[1]), img.new_empty(V, h, w, cfg[2])


geo_encode.register_autograd(_encoder_bwd, setup_context=_encoder_no_autograd)


@_lib.custom_op("kpnerf::tex_encode", mutates_args=(), device_types="cuda")
def tex_encode(img: torch.Tensor, packed: torch.Tensor, cfg: List[int], eps: float) -> torch.Tensor:
    """ResBlkEncoder.forward(2 * avg_pool2d^ds(img) - 1) (reference src/utils.py:216-247, src/model.py:668-680; kpn_tex_encode).
    cfg = [ds, ngf, n_downsample, n_blocks, n_upsample, out_ch]; packed = ops.tex_encoder_pack(...).  Returns channels-last
    (V, ht, wt, out_ch).  No autograd formula: raises on inputs that require a gradient."""
    return ops.tex_encode(img, packed, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], eps)[0]


@tex_encode.register_fake
def _(img, packed, cfg, eps):
    h, w = img.shape[2] >> cfg[0], img.shape[3] >> cfg[0]
    for _ in range(cfg[2]):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return img.new_empty(img.shape[0], h << cfg[4], w << cfg[4], cfg[5])


tex_encode.register_autograd(_encoder_bwd, setup_context=_encoder_no_autograd)


# ---- torch.ops.kpnerf.conv2d: one stride-1 convolution, DIFFERENTIABLE w.r.t. x, weight and bias ----
# The two packed copies of a weight (forward order; transposed + flipped for the input gradient) are kept per weight: the key is
# _tensor_key (storage address, version counter, shape, device) and the entry holds the weight it was packed from, so an equal
# address means the same storage and an in-place update (an optimizer step) moves the version: a miss and a re-pack, never a stale
# hit.  Inference tensors have no version counter: they are packed on every call and not kept.  At most _ConvPackCache.limit
# weights stay resident (least recently used first out); conv2d_cache_clear() drops them all.
class _ConvPackCache:
    lock = threading.Lock()
    entries = collections.OrderedDict()     # data_ptr -> (key, weights, packed)
    limit = 512
    hits = misses = 0                       # observable by the tests


def conv2d_cache_clear():
    with _ConvPackCache.lock:
        _ConvPackCache.entries.clear()


def _packed(C, weights, tag, pack):
    """``pack()``, the packed copies of ``weights``, kept in the cache ``C`` (this one and the one of kpnerf::res_encoder below) in the
    slot of the first weight's storage address.  _tensor_key of every weight and ``tag`` (hashable: the family, its kind or arithmetic,
    a network's configuration) decide hit or miss; the entry holds the weights it was packed from."""
    key = [tag]                         # a plain loop: for one weight it costs what the per-weight lookup it replaced did
    for w in weights:
        if w.is_inference():
            return pack()
        key.append(_tensor_key(w))
    slot = key[1][0]
    with C.lock:
        e = C.entries.get(slot)
        if e is not None and e[0] == key:
            C.entries.move_to_end(slot)
            C.hits += 1
            return e[2]
    packed = pack()
    with C.lock:
        C.misses += 1
        C.entries[slot] = (key, weights, packed)
        C.entries.move_to_end(slot)
        while len(C.entries) > C.limit:
            C.entries.popitem(last=False)
    return packed


def _packed_conv(weight, arith=0):
    """the packed copies of a stride-1 weight for ``arith``: the arithmetic is part of the cache key, so a weight used under both has two
    entries' worth of packs, one resident at a time per weight"""
    return _packed(_ConvPackCache, (weight,), ("conv", arith), lambda: ops.conv2d_pack(weight, arith))


def _packed_s2(weight, kind):
    return _packed(_ConvPackCache, (weight,), ("s2", kind), lambda: ops.conv2d_s2_pack(weight, kind))


def _packed_rp(weight, kind):
    return _packed(_ConvPackCache, (weight,), ("rp", kind), lambda: ops.conv2d_rp_pack(weight, kind))


# What the three families' backward operators (kpnerf::conv2d_backward, conv2d_s2_backward, conv2d_rp_backward) and the autograd
# backward of the four forward operators share.
def _layer_backward(backward, x, dy, packed, args, has_bias, mask, **arith):
    """the body of a backward operator: ``backward`` is the family's ops.*_backward, ``packed`` the packed copies (None without dx) and
    ``args`` what that function takes between them and has_bias"""
    dy = dy.contiguous(memory_format=torch.channels_last)
    dx, dw, db = backward(x, dy, packed, *args, has_bias, want_dx=mask[0], want_dw=mask[1], want_db=mask[2], **arith)
    return _empty_for_none(dy, dx, dw, db)


def _layer_backward_fake(x, weight, has_bias, mask, cout, dx_format=torch.channels_last):
    e = x.new_empty(0)
    return (torch.empty_like(x, memory_format=dx_format) if mask[0] else e, torch.empty_like(weight) if mask[1] else e,
            x.new_empty(cout) if mask[2] and has_bias else e)


def _layer_autograd(backward_op, n_inputs):
    """the autograd backward of a forward operator over (x, weight, bias, ...n_inputs in all): only the legs whose inputs need a gradient
    run, through ``backward_op`` with the tuple ctx.what (the padding, the kind, the arithmetic) between dy and has_bias"""
    nothing = (None,) * n_inputs

    def bwd(ctx, dy):
        if dy is None:
            return nothing
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        mask = [bool(need[0]), bool(need[1]), bool(ctx.has_bias and need[2])]
        if not any(mask):
            return nothing
        dx, dw, db = backward_op(x, weight, dy, *ctx.what, ctx.has_bias, mask)
        return _none_unless(mask, dx, dw, db) + nothing[3:]
    return bwd


# One implementation each of the forward, the backward, the fake kernels and the setup context serves kpnerf::conv2d and, further down,
# kpnerf::conv2d_arith: the plain operators are its arith = 0 registration.
def _conv2d_forward(x, weight, bias, padding, arith=0):
    return ops.conv2d_forward(x, _packed_conv(weight, arith), bias, weight.shape[0], weight.shape[2], padding, arith=arith)


def _conv2d_fake(x, weight, bias, padding, arith=0):
    N, _, H, W = x.shape
    cout, _, k, _ = weight.shape
    return x.new_empty(N, H + 2 * padding - k + 1, W + 2 * padding - k + 1, cout).permute(0, 3, 1, 2)


def _conv2d_backward(x, weight, dy, padding, has_bias, mask, arith=0):
    return _layer_backward(ops.conv2d_backward, x, dy, _packed_conv(weight, arith) if mask[0] else None,
                           (weight.shape[1], weight.shape[2], padding), has_bias, mask, arith=arith)


def _conv2d_backward_fake(x, weight, dy, padding, has_bias, mask, arith=0):
    return _layer_backward_fake(x, weight, has_bias, mask, weight.shape[0], torch.preserve_format)


def _conv2d_setup(ctx, inputs, output):
    x, weight, bias, *ctx.what = inputs                         # (padding,) or (padding, arith)
    ctx.save_for_backward(x, weight)
    ctx.has_bias = bias is not None
    ctx.set_materialize_grads(False)


@_lib.custom_op("kpnerf::conv2d_cl", mutates_args=(), device_types="cuda")
def conv2d_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], padding: int) -> torch.Tensor:
    """conv2d(x, weight, bias, stride=1, padding=padding) for a channels_last x (kpn_conv2d_forward): what torch.ops.kpnerf.conv2d
    runs after its memory-format conversion.  weight (cout, cin, k, k), k in {1, 3, 5}, 0 <= padding < k, cin and cout multiples of 4.
    Returns (N, cout, Ho, Wo) channels_last."""
    return _conv2d_forward(x, weight, bias, padding)


conv2d_cl.register_fake(_conv2d_fake)


@_lib.custom_op("kpnerf::conv2d_backward", mutates_args=(), device_types="cuda")
def conv2d_backward(x: torch.Tensor, weight: torch.Tensor, dy: torch.Tensor, padding: int, has_bias: bool,
                    mask: List[bool]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of kpnerf::conv2d_cl for the output gradient dy (kpn_conv2d_backward); mask = [dx, dweight, dbias]
    wanted: a leg that is not wanted is not launched and its result is an empty tensor."""
    return _conv2d_backward(x, weight, dy, padding, has_bias, mask)


conv2d_backward.register_fake(_conv2d_backward_fake)
conv2d_cl.register_autograd(_layer_autograd(torch.ops.kpnerf.conv2d_backward, 4), setup_context=_conv2d_setup)


# torch.ops.kpnerf.conv2d(x, weight, bias, padding): x in any memory format.  A contiguous NCHW input is converted to channels_last
# ONCE here (one copy, differentiable: its backward is the reverse copy); the operator behind it and its backward then both read the
# converted tensor.  A channels_last input passes through as it is.  The result is channels_last.
def _conv2d(x, weight, bias, padding):
    return torch.ops.kpnerf.conv2d_cl(x.contiguous(memory_format=torch.channels_last), weight, bias, padding)


_fragment.define("conv2d(Tensor x, Tensor weight, Tensor? bias, int padding) -> Tensor")
_fragment.impl("conv2d", _conv2d, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.conv2d_down2 / conv_transpose2d_up2: the resolution-changing layers, DIFFERENTIABLE ----
# Conv2d(k 3, stride 2, pad 1) and the stem Conv2d(k 7, stride 2, pad 3) share one operator, the kind following the weight's kernel
# size; ConvTranspose2d(k 3, stride 2, pad 1, output_padding 1) has its own.  One backward operator serves the three kinds
# (kpn_conv2d_s2_backward).  The packed copies live in the cache of kpnerf::conv2d, keyed by weight and kind.  The stem reads a
# contiguous NCHW tensor as it is and has no input gradient: it raises on an x that requires one.
def _down2_kind(weight):
    k = weight.shape[-1]
    if k not in (3, 7):
        raise ValueError(f"conv2d_down2: kernel size {k} (3: stride 2, padding 1; 7: the stem, stride 2, padding 3)")
    return kl.S2_STEM7 if k == 7 else kl.S2_CONV3


@_lib.custom_op("kpnerf::conv2d_down2_cl", mutates_args=(), device_types="cuda")
def conv2d_down2_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """conv2d(x, weight, bias, stride=2, padding=k // 2) for weight (cout, cin, k, k), k = 3 (x channels_last, H and W even, cin and
    cout multiples of 4) or k = 7 (x contiguous NCHW, cin <= 4) (kpn_conv2d_s2_forward): what torch.ops.kpnerf.conv2d_down2 runs
    after its memory-format conversion.  Returns (N, cout, Ho, Wo) channels_last."""
    kind = _down2_kind(weight)
    return ops.conv2d_s2_forward(x, _packed_s2(weight, kind), bias, weight.shape[0], kind)


@conv2d_down2_cl.register_fake
def _(x, weight, bias):
    N, _, H, W = x.shape
    return x.new_empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, weight.shape[0]).permute(0, 3, 1, 2)


@_lib.custom_op("kpnerf::conv_transpose2d_up2_cl", mutates_args=(), device_types="cuda")
def conv_transpose2d_up2_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """conv_transpose2d(x, weight, bias, stride=2, padding=1, output_padding=1) for a channels_last x and weight (cin, cout, 3, 3), cin
    and cout multiples of 4 (kpn_conv2d_s2_forward): what torch.ops.kpnerf.conv_transpose2d_up2 runs after its memory-format
    conversion.  Returns (N, cout, 2H, 2W) channels_last."""
    if weight.shape[-1] != 3:
        raise ValueError(f"conv_transpose2d_up2: kernel size {weight.shape[-1]} (3 only)")
    return ops.conv2d_s2_forward(x, _packed_s2(weight, kl.S2_DECONV3), bias, weight.shape[1], kl.S2_DECONV3)


@conv_transpose2d_up2_cl.register_fake
def _(x, weight, bias):
    N, _, H, W = x.shape
    return x.new_empty(N, 2 * H, 2 * W, weight.shape[1]).permute(0, 3, 1, 2)


@_lib.custom_op("kpnerf::conv2d_s2_backward", mutates_args=(), device_types="cuda")
def conv2d_s2_backward(x: torch.Tensor, weight: torch.Tensor, dy: torch.Tensor, kind: int, has_bias: bool,
                       mask: List[bool]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of kpnerf::conv2d_down2_cl / conv_transpose2d_up2_cl for the output gradient dy (kpn_conv2d_s2_backward);
    kind is the KPN_S2_* value; mask = [dx, dweight, dbias] wanted: a leg that is not wanted is not launched and its result is an
    empty tensor."""
    return _layer_backward(ops.conv2d_s2_backward, x, dy, _packed_s2(weight, kind) if mask[0] else None, (x.shape, kind), has_bias, mask)


@conv2d_s2_backward.register_fake
def _(x, weight, dy, kind, has_bias, mask):
    return _layer_backward_fake(x, weight, has_bias, mask, weight.shape[1 if kind == kl.S2_DECONV3 else 0])


def _s2_setup(kind_of):
    def setup(ctx, inputs, output):
        x, weight, bias = inputs
        ctx.what, ctx.has_bias = (kind_of(weight),), bias is not None
        if ctx.what[0] == kl.S2_STEM7 and ctx.needs_input_grad[0]:
            raise RuntimeError("kpnerf::conv2d_down2: the 7x7 stem has no input gradient (x.requires_grad is set)")
        ctx.save_for_backward(x, weight)
        ctx.set_materialize_grads(False)
    return setup


_s2_bwd = _layer_autograd(torch.ops.kpnerf.conv2d_s2_backward, 3)
conv2d_down2_cl.register_autograd(_s2_bwd, setup_context=_s2_setup(_down2_kind))
conv_transpose2d_up2_cl.register_autograd(_s2_bwd, setup_context=_s2_setup(lambda w: kl.S2_DECONV3))


# torch.ops.kpnerf.conv2d_down2(x, weight, bias) / conv_transpose2d_up2(x, weight, bias): x in any memory format, converted once (as
# kpnerf::conv2d does) - to channels_last, or to contiguous NCHW for the stem, which reads that layout as it is.
def _conv2d_down2(x, weight, bias):
    stem = _down2_kind(weight) == kl.S2_STEM7
    return torch.ops.kpnerf.conv2d_down2_cl(x.contiguous() if stem else x.contiguous(memory_format=torch.channels_last), weight, bias)


def _conv_transpose2d_up2(x, weight, bias):
    return torch.ops.kpnerf.conv_transpose2d_up2_cl(x.contiguous(memory_format=torch.channels_last), weight, bias)


_fragment.define("conv2d_down2(Tensor x, Tensor weight, Tensor? bias) -> Tensor")
_fragment.impl("conv2d_down2", _conv2d_down2, "CompositeImplicitAutograd")
_fragment.define("conv_transpose2d_up2(Tensor x, Tensor weight, Tensor? bias) -> Tensor")
_fragment.impl("conv_transpose2d_up2", _conv_transpose2d_up2, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.conv2d_replicate: ReplicationPad2d(k // 2) + Conv2d(k), DIFFERENTIABLE ----
# One operator for the three kinds of kpn_conv2d_rp_*, the kind following the weight: 3x3, 7x7, or - a 7x7 weight with at most 4 input
# channels - the stem, which reads a contiguous NCHW tensor as it is and has no input gradient: it raises on an x that requires one.
# The packed copies live in the cache of kpnerf::conv2d, keyed by weight and kind.
@_lib.custom_op("kpnerf::conv2d_replicate_cl", mutates_args=(), device_types="cuda")
def conv2d_replicate_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """conv2d(pad(x, k // 2, mode="replicate"), weight, bias) for weight (cout, cin, k, k), k = 3 or 7 (x channels_last, cin and cout
    multiples of 4) or k = 7 with cin <= 4 (x contiguous NCHW) (kpn_conv2d_rp_forward): what torch.ops.kpnerf.conv2d_replicate runs
    after its memory-format conversion.  Returns (N, cout, H, W) channels_last."""
    kind = ops.conv2d_rp_kind(weight.shape)
    return ops.conv2d_rp_forward(x, _packed_rp(weight, kind), bias, weight.shape[0], kind)


@conv2d_replicate_cl.register_fake
def _(x, weight, bias):
    N, _, H, W = x.shape
    return x.new_empty(N, H, W, weight.shape[0]).permute(0, 3, 1, 2)


@_lib.custom_op("kpnerf::conv2d_rp_backward", mutates_args=(), device_types="cuda")
def conv2d_rp_backward(x: torch.Tensor, weight: torch.Tensor, dy: torch.Tensor, kind: int, has_bias: bool,
                       mask: List[bool]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of kpnerf::conv2d_replicate_cl for the output gradient dy (kpn_conv2d_rp_backward); kind is the KPN_RP_*
    value; mask = [dx, dweight, dbias] wanted: a leg that is not wanted is not launched and its result is an empty tensor."""
    return _layer_backward(ops.conv2d_rp_backward, x, dy, _packed_rp(weight, kind) if mask[0] else None, (x.shape, kind), has_bias, mask)


@conv2d_rp_backward.register_fake
def _(x, weight, dy, kind, has_bias, mask):
    return _layer_backward_fake(x, weight, has_bias, mask, weight.shape[0])


def _rp_setup(ctx, inputs, output):
    x, weight, bias = inputs
    ctx.what, ctx.has_bias = (ops.conv2d_rp_kind(weight.shape),), bias is not None
    if ctx.what[0] == kl.RP_STEM7 and ctx.needs_input_grad[0]:
        raise RuntimeError("kpnerf::conv2d_replicate: the 7x7 stem has no input gradient (x.requires_grad is set)")
    ctx.save_for_backward(x, weight)
    ctx.set_materialize_grads(False)


conv2d_replicate_cl.register_autograd(_layer_autograd(torch.ops.kpnerf.conv2d_rp_backward, 3), setup_context=_rp_setup)


# torch.ops.kpnerf.conv2d_replicate(x, weight, bias): x in any memory format, converted once (as kpnerf::conv2d does) - to channels_last,
# or to contiguous NCHW for the stem, which reads that layout as it is.
def _conv2d_replicate(x, weight, bias):
    stem = ops.conv2d_rp_kind(weight.shape) == kl.RP_STEM7
    return torch.ops.kpnerf.conv2d_replicate_cl(x.contiguous() if stem else x.contiguous(memory_format=torch.channels_last), weight, bias)


_fragment.define("conv2d_replicate(Tensor x, Tensor weight, Tensor? bias) -> Tensor")
_fragment.impl("conv2d_replicate", _conv2d_replicate, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.group_norm: GroupNorm / InstanceNorm2d [+ ReLU], DIFFERENTIABLE w.r.t. x, weight and bias ----
# The backward reads x, weight and the statistics the forward kept; it never reads y (the mask of a fused ReLU is recomputed from x and
# the kept scale / shift), so the caller may overwrite y in place - the reference's nl is ReLU(inplace=True).
@_lib.custom_op("kpnerf::group_norm_cl", mutates_args=(), device_types="cuda")
def group_norm_cl(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], groups: int, eps: float,
                  relu: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, stats) of [relu](group_norm(x, groups, weight, bias, eps)) for a channels_last x (kpn_group_norm_forward): what
    torch.ops.kpnerf.group_norm runs after its memory-format conversion.  C a power of two in 4 .. 1024; weight and bias both (C,)
    or both None.  y is (N, C, H, W) channels_last; stats is the side buffer of the backward."""
    return ops.group_norm_forward(x, weight, bias, groups, eps, relu)


@group_norm_cl.register_fake
def _(x, weight, bias, groups, eps, relu):
    N, C, H, W = x.shape
    return torch.empty_like(x, memory_format=torch.channels_last), x.new_empty(2 * N * C + 2 * N * groups)


@_lib.custom_op("kpnerf::group_norm_backward", mutates_args=(), device_types="cuda")
def group_norm_backward(x: torch.Tensor, weight: Optional[torch.Tensor], stats: torch.Tensor, dy: torch.Tensor, groups: int, eps: float,
                        relu: bool, mask: List[bool]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of kpnerf::group_norm_cl for the output gradient dy (kpn_group_norm_backward); mask = [dx, dweight, dbias]
    wanted: what is not wanted is not computed and its result is an empty tensor."""
    dy = dy.contiguous(memory_format=torch.channels_last)
    dx, dw, db = ops.group_norm_backward(x, dy, weight, stats, groups, eps, relu, want_dx=mask[0], want_dw=mask[1], want_db=mask[2])
    return _empty_for_none(dy, dx, dw, db)


@group_norm_backward.register_fake
def _(x, weight, stats, dy, groups, eps, relu, mask):
    e, affine = x.new_empty(0), weight is not None
    return (torch.empty_like(x) if mask[0] else e, x.new_empty(x.shape[1]) if mask[1] and affine else e,
            x.new_empty(x.shape[1]) if mask[2] and affine else e)


def _group_norm_setup(ctx, inputs, output):
    x, weight, bias, groups, eps, relu = inputs
    ctx.affine = weight is not None
    ctx.save_for_backward(x, output[1], *([weight] if ctx.affine else []))       # never y
    ctx.groups, ctx.eps, ctx.relu = groups, eps, relu
    ctx.set_materialize_grads(False)


def _group_norm_bwd(ctx, dy, _d_stats):
    if dy is None:
        return None, None, None, None, None, None
    x, stats, *w = ctx.saved_tensors
    need = ctx.needs_input_grad
    mask = [bool(need[0]), bool(ctx.affine and need[1]), bool(ctx.affine and need[2])]
    if not any(mask):
        return None, None, None, None, None, None
    dx, dw, db = torch.ops.kpnerf.group_norm_backward(x, w[0] if w else None, stats, dy, ctx.groups, ctx.eps, ctx.relu, mask)
    return _none_unless(mask, dx, dw, db) + (None, None, None)


group_norm_cl.register_autograd(_group_norm_bwd, setup_context=_group_norm_setup)


# torch.ops.kpnerf.group_norm(x, weight, bias, groups, eps, relu): x in any memory format, converted to channels_last once (as
# kpnerf::conv2d does); the result is channels_last.
def _group_norm(x, weight, bias, groups, eps, relu):
    return torch.ops.kpnerf.group_norm_cl(x.contiguous(memory_format=torch.channels_last), weight, bias, groups, eps, relu)[0]


_fragment.define("group_norm(Tensor x, Tensor? weight, Tensor? bias, int groups, float eps, bool relu) -> Tensor")
_fragment.impl("group_norm", _group_norm, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.conv_block: a whole ConvBlock, DIFFERENTIABLE w.r.t. x and every parameter, one autograd node ----
# tensors: per leg (norm weight, norm bias, convolution weight) - bn1 / conv1, bn2 / conv2, bn3 / conv3 and, for cin != cout, bn4 / the
# 1x1 downsample convolution: 9 or 12 tensors.  The packed copies of the weights come from the cache of kpnerf::conv2d.  The backward
# reads x, the parameters and `state` (the outputs of conv1 and conv2 and every norm's statistics); it never reads y.
def _block_legs(tensors):
    if len(tensors) not in (9, 12):
        raise ValueError(f"conv_block takes 9 tensors (cin == cout) or 12 (with the downsample leg), got {len(tensors)}")
    return [tensors[i:i + 3] for i in range(0, len(tensors), 3)]


# One implementation each of the forward, the backward, the fake kernels, the setup context and the autograd backward serves
# kpnerf::conv_block and, further down, kpnerf::conv_block_arith: the plain operators are its arith = 0 registration.
def _conv_block_forward(x, tensors, eps, arith=0):
    legs = _block_legs(tensors)
    return ops.conv_block_forward(x, [(g, b) for g, b, _ in legs], [_packed_conv(w, arith) for _, _, w in legs], 2 * legs[0][2].shape[0], eps,
                                  arith=arith)


def _conv_block_fake(x, tensors, eps, arith=0):
    # the state size is the library's answer for a descriptor of plain ints: a symbolic N, H or W is specialised here (as in the fake
    # kernels of hg_filter_cl and fold_params_norms)
    N, cin, H, W = x.shape
    cout = 2 * tensors[2].shape[0]
    d = ops._block_desc(N, H, W, cin, cout, eps)
    return x.new_empty(N, H, W, cout).permute(0, 3, 1, 2), x.new_empty(ops._conv_library(arith).kpn_conv_block_state_floats(ctypes.byref(d)))


def _conv_block_backward(x, tensors, state, dy, eps, mask, arith=0):
    legs = _block_legs(tensors)
    dy = dy.contiguous(memory_format=torch.channels_last)
    want = [tuple(mask[1 + 3 * i:4 + 3 * i]) for i in range(len(legs))]
    dx, grads = ops.conv_block_backward(x, dy, [(g, b) for g, b, _ in legs], [_packed_conv(w, arith) for _, _, w in legs], state, eps,
                                        want_dx=mask[0], want=want, arith=arith)
    return list(_empty_for_none(dy, dx, *[g for leg in grads for g in leg]))


def _conv_block_backward_fake(x, tensors, state, dy, eps, mask, arith=0):
    # one empty tensor per gradient that is not wanted, as the operator returns them: no two results share memory
    return [torch.empty_like(x) if mask[0] else x.new_empty(0)] + [torch.empty_like(t) if m else x.new_empty(0) for t, m in zip(tensors, mask[1:])]


def _conv_block_setup(ctx, inputs, output):
    x, tensors, *ctx.what = inputs                                               # (eps,) or (eps, arith)
    ctx.save_for_backward(x, output[1], *tensors)                                # never y, never a normalised tensor
    ctx.set_materialize_grads(False)


def _conv_block_autograd(backward_op):
    def bwd(ctx, dy, _d_state):
        x, state, *tensors = ctx.saved_tensors
        none = (None, [None] * len(tensors)) + (None,) * len(ctx.what)
        if dy is None:
            return none
        mask = [bool(ctx.needs_input_grad[0])] + [bool(b) for b in ctx.needs_input_grad[1]]
        if not any(mask):
            return none
        out = _none_unless(mask, *backward_op(x, list(tensors), state, dy, *ctx.what, mask))
        return (out[0], list(out[1:])) + none[2:]
    return bwd


@_lib.custom_op("kpnerf::conv_block_cl", mutates_args=(), device_types="cuda")
def conv_block_cl(x: torch.Tensor, tensors: List[torch.Tensor], eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, state) of a ConvBlock for a channels_last x (kpn_conv_block_forward): what torch.ops.kpnerf.conv_block runs after its
    memory-format conversion.  y is (N, cout, H, W) channels_last with cout = 2 * conv1.weight.shape[0]; state is the side buffer of the
    backward."""
    return _conv_block_forward(x, tensors, eps)


conv_block_cl.register_fake(_conv_block_fake)


@_lib.custom_op("kpnerf::conv_block_backward", mutates_args=(), device_types="cuda")
def conv_block_backward(x: torch.Tensor, tensors: List[torch.Tensor], state: torch.Tensor, dy: torch.Tensor, eps: float,
                        mask: List[bool]) -> List[torch.Tensor]:
    """[dx] + one gradient per tensor of kpnerf::conv_block_cl for the output gradient dy (kpn_conv_block_backward); mask = [dx wanted]
    + one flag per tensor: what is not wanted is not computed and its result is an empty tensor."""
    return _conv_block_backward(x, tensors, state, dy, eps, mask)


conv_block_backward.register_fake(_conv_block_backward_fake)
conv_block_cl.register_autograd(_conv_block_autograd(torch.ops.kpnerf.conv_block_backward), setup_context=_conv_block_setup)


# torch.ops.kpnerf.conv_block(x, tensors, eps): x in any memory format, converted to channels_last once (as kpnerf::conv2d does); the
# result is channels_last.
def _conv_block(x, tensors, eps):
    return torch.ops.kpnerf.conv_block_cl(x.contiguous(memory_format=torch.channels_last), tensors, eps)[0]


_fragment.define("conv_block(Tensor x, Tensor[] tensors, float eps) -> Tensor")
_fragment.impl("conv_block", _conv_block, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.conv2d_arith / conv_block_arith: the two operators above with the arithmetic of their GEMMs as an argument ----
# arith = 0 (CONV_F32) computes what kpnerf::conv2d / kpnerf::conv_block compute, bit for bit; arith = 1 (CONV_BF16X3) runs the
# convolutions on three bf16 pieces per operand (kpn_conv2d_ex_*, kpn_conv_block_ex_*).  The existing schemas stay as they are; these
# are operators of their own over the same bodies (_conv2d_* / _conv_block_* above) and the same pack cache (arith is in its key).
@_lib.custom_op("kpnerf::conv2d_arith_cl", mutates_args=(), device_types="cuda")
def conv2d_arith_cl(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], padding: int, arith: int) -> torch.Tensor:
    """kpnerf::conv2d_cl in the arithmetic ``arith`` (kpn_conv2d_ex_forward)"""
    return _conv2d_forward(x, weight, bias, padding, arith)


conv2d_arith_cl.register_fake(_conv2d_fake)


@_lib.custom_op("kpnerf::conv2d_arith_backward", mutates_args=(), device_types="cuda")
def conv2d_arith_backward(x: torch.Tensor, weight: torch.Tensor, dy: torch.Tensor, padding: int, arith: int, has_bias: bool,
                          mask: List[bool]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """kpnerf::conv2d_backward in the arithmetic ``arith`` (kpn_conv2d_ex_backward)"""
    return _conv2d_backward(x, weight, dy, padding, has_bias, mask, arith)


@conv2d_arith_backward.register_fake
def _(x, weight, dy, padding, arith, has_bias, mask):
    return _conv2d_backward_fake(x, weight, dy, padding, has_bias, mask)


conv2d_arith_cl.register_autograd(_layer_autograd(torch.ops.kpnerf.conv2d_arith_backward, 5), setup_context=_conv2d_setup)


def _conv2d_arith(x, weight, bias, padding, arith):
    return torch.ops.kpnerf.conv2d_arith_cl(x.contiguous(memory_format=torch.channels_last), weight, bias, padding, arith)


_fragment.define("conv2d_arith(Tensor x, Tensor weight, Tensor? bias, int padding, int arith) -> Tensor")
_fragment.impl("conv2d_arith", _conv2d_arith, "CompositeImplicitAutograd")


@_lib.custom_op("kpnerf::conv_block_arith_cl", mutates_args=(), device_types="cuda")
def conv_block_arith_cl(x: torch.Tensor, tensors: List[torch.Tensor], eps: float, arith: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kpnerf::conv_block_cl with every convolution in the arithmetic ``arith`` (kpn_conv_block_ex_forward)"""
    return _conv_block_forward(x, tensors, eps, arith)


conv_block_arith_cl.register_fake(_conv_block_fake)


@_lib.custom_op("kpnerf::conv_block_arith_backward", mutates_args=(), device_types="cuda")
def conv_block_arith_backward(x: torch.Tensor, tensors: List[torch.Tensor], state: torch.Tensor, dy: torch.Tensor, eps: float, arith: int,
                              mask: List[bool]) -> List[torch.Tensor]:
    """kpnerf::conv_block_backward with every convolution in the arithmetic ``arith`` (kpn_conv_block_ex_backward)"""
    return _conv_block_backward(x, tensors, state, dy, eps, mask, arith)


@conv_block_arith_backward.register_fake
def _(x, tensors, state, dy, eps, arith, mask):
    return _conv_block_backward_fake(x, tensors, state, dy, eps, mask)


conv_block_arith_cl.register_autograd(_conv_block_autograd(torch.ops.kpnerf.conv_block_arith_backward), setup_context=_conv_block_setup)


def _conv_block_arith(x, tensors, eps, arith):
    return torch.ops.kpnerf.conv_block_arith_cl(x.contiguous(memory_format=torch.channels_last), tensors, eps, arith)[0]


_fragment.define("conv_block_arith(Tensor x, Tensor[] tensors, float eps, int arith) -> Tensor")
_fragment.impl("conv_block_arith", _conv_block_arith, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.res_encoder: a whole ResBlkEncoder, DIFFERENTIABLE w.r.t. every parameter, one autograd node ----
# tensors: [weight, bias] per convolution in module order - the stem, the stride-2 layers, two per ResBlk, the transposed layers, the
# output layer.  The packed copies of all weights are one buffer, packed once per parameter version (the key is _tensor_key of every
# weight, as in the cache of kpnerf::conv2d).  The backward reads x, `state` (every convolution output, every a_k and every norm's
# statistics) and the packed weights; it never reads y.  There is no input gradient: an x that requires one raises.
def _res_cfg(tensors, n_down, n_blocks, n_up):
    n = 2 + n_down + 2 * n_blocks + n_up
    if len(tensors) != 2 * n or n_down < 0 or n_blocks < 0 or n_up < 0:
        raise ValueError(f"res_encoder takes [weight, bias] for each of its {n} convolutions, got {len(tensors)} tensors")
    return (tensors[0].shape[0], n_down, n_blocks, n_up, tensors[-2].shape[0])


class _ResPackCache:
    lock = threading.Lock()
    entries = collections.OrderedDict()     # data_ptr of the stem's weight -> (key, weights, packed)
    limit = 16
    hits = misses = 0                       # observable by the tests


def res_encoder_cache_clear():
    with _ResPackCache.lock:
        _ResPackCache.entries.clear()


def _res_packed(weights, in_ch, cfg):
    return _packed(_ResPackCache, weights, tuple(cfg), lambda: ops.res_encoder_pack(weights, in_ch, cfg))


@_lib.custom_op("kpnerf::res_encoder_cl", mutates_args=(), device_types="cuda")
def res_encoder_cl(x: torch.Tensor, tensors: List[torch.Tensor], n_down: int, n_blocks: int, n_up: int,
                   eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, state) of a ResBlkEncoder for a contiguous NCHW x (kpn_res_encoder_forward): what torch.ops.kpnerf.res_encoder runs after its
    memory-format conversion.  y is (N, out_ch, H >> (n_down - n_up), W >> (n_down - n_up)) channels_last; state is the side buffer of the
    backward."""
    cfg = _res_cfg(tensors, n_down, n_blocks, n_up)
    return ops.res_encoder_forward(x, _res_packed(tensors[0::2], x.shape[1], cfg), tensors[1::2], cfg, eps)


@res_encoder_cl.register_fake
def _(x, tensors, n_down, n_blocks, n_up, eps):
    cfg = _res_cfg(tensors, n_down, n_blocks, n_up)
    N, in_ch, H, W = x.shape
    f = n_down - n_up
    d = ops._res_encoder_desc(N, H, W, in_ch, cfg, eps)       # plain ints: a symbolic N, H or W is specialised here
    return x.new_empty(N, H >> f, W >> f, cfg[4]).permute(0, 3, 1, 2), x.new_empty(kl.get_library().kpn_res_encoder_state_floats(ctypes.byref(d)))


@_lib.custom_op("kpnerf::res_encoder_backward", mutates_args=(), device_types="cuda")
def res_encoder_backward(x: torch.Tensor, tensors: List[torch.Tensor], state: torch.Tensor, dy: torch.Tensor, n_down: int, n_blocks: int,
                         n_up: int, eps: float, mask: List[bool]) -> List[torch.Tensor]:
    """one gradient per tensor of kpnerf::res_encoder_cl for the output gradient dy (kpn_res_encoder_backward); mask has one flag per
    tensor: what is not wanted is not computed and its result is an empty tensor."""
    cfg = _res_cfg(tensors, n_down, n_blocks, n_up)
    dy = dy.contiguous(memory_format=torch.channels_last)
    want = [(bool(mask[2 * i]), bool(mask[2 * i + 1])) for i in range(len(tensors) // 2)]
    grads = ops.res_encoder_backward(x, dy, _res_packed(tensors[0::2], x.shape[1], cfg), state, cfg, eps, want=want)
    return list(_empty_for_none(dy, *[g for pair in grads for g in pair]))


@res_encoder_backward.register_fake
def _(x, tensors, state, dy, n_down, n_blocks, n_up, eps, mask):
    # one empty tensor per gradient that is not wanted, as the operator returns them: no two results share memory
    return [torch.empty_like(t) if m else x.new_empty(0) for t, m in zip(tensors, mask)]


def _res_encoder_setup(ctx, inputs, output):
    x, tensors, n_down, n_blocks, n_up, eps = inputs
    if ctx.needs_input_grad[0]:
        raise RuntimeError("kpnerf::res_encoder: the 7x7 stem has no input gradient (x.requires_grad is set)")
    ctx.save_for_backward(x, output[1], *tensors)                                # never y, never a normalised tensor
    ctx.cfg = (n_down, n_blocks, n_up, eps)
    ctx.set_materialize_grads(False)


def _res_encoder_bwd(ctx, dy, _d_state):
    x, state, *tensors = ctx.saved_tensors
    none = (None, [None] * len(tensors), None, None, None, None)
    if dy is None:
        return none
    mask = [bool(b) for b in ctx.needs_input_grad[1]]
    if not any(mask):
        return none
    out = torch.ops.kpnerf.res_encoder_backward(x, list(tensors), state, dy, *ctx.cfg, mask)
    return None, list(_none_unless(mask, *out)), None, None, None, None


res_encoder_cl.register_autograd(_res_encoder_bwd, setup_context=_res_encoder_setup)


# torch.ops.kpnerf.res_encoder(x, tensors, n_down, n_blocks, n_up, eps): x in any memory format, converted once to the contiguous NCHW
# layout the stem reads as it is; the result is channels_last.
def _res_encoder(x, tensors, n_down, n_blocks, n_up, eps):
    return torch.ops.kpnerf.res_encoder_cl(x.contiguous(), tensors, n_down, n_blocks, n_up, eps)[0]


_fragment.define("res_encoder(Tensor x, Tensor[] tensors, int n_down, int n_blocks, int n_up, float eps) -> Tensor")
_fragment.impl("res_encoder", _res_encoder, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.hg_filter: a whole HGFilterV2, DIFFERENTIABLE w.r.t. every parameter, one autograd node ----
# tensors, in the order of include/kpnerf.h: conv1 w, b; bn1 w, b; per ConvBlock in dataflow order (conv2, conv3, conv4, the HourGlass in its
# module order b1_d, b2_d, ..., b2_plus_1, b3_1, ..., b3_d, top_m_0) the 9 or 12 tensors of conv_block; unpack1.conv w; unpack1.norm w, b;
# conv_out w, b; conv_last0 w, b; bn_end0 w, b; l0 w, b.  The packed copies of all convolution weights are one buffer, packed once per
# parameter version in the cache of kpnerf::res_encoder (the key is _tensor_key of every weight).  The backward reads x, `state` and the
# parameters; it never reads an output.  There is no input gradient: an x that requires one raises.
def _hg_cfg(x, tensors, depth):
    """(in_ch, c_stem, c2, c3, c4, depth, c_hd, out_ch_hd, out_ch) from the tensors' shapes; ops.hg_filter_shapes checks the rest"""
    nblocks = 3 * depth + 5
    if depth < 1 or len(tensors) < 4 + 9 * nblocks + 11:
        raise ValueError(f"hg_filter takes the tensors of an HGFilterV2 with an HourGlass of depth {depth}, got {len(tensors)} tensors")
    widths, t = [tensors[0].shape[0]], 4
    for _ in range(3):                                  # conv2, conv3, conv4: 9 tensors, 12 where the width changes
        cin, cout = tensors[t].shape[0], 2 * tensors[t + 2].shape[0]
        widths.append(cout)
        t += 12 if cin != cout else 9
    cfg = (x.shape[1], widths[0], widths[1], widths[2], widths[3], depth, tensors[-10].shape[0], tensors[-8].shape[0], tensors[-2].shape[0])
    shapes = ops.hg_filter_shapes(cfg)
    if len(shapes) != len(tensors) or any(tuple(a.shape) != b for a, b in zip(tensors, shapes)):
        raise ValueError(f"hg_filter: the tensors do not have the shapes of an HGFilterV2 with the widths {cfg[1:5]} and depth {depth}")
    return cfg


def _hg_packed(tensors, cfg):
    weights = [t for t in tensors if t.dim() == 4]
    return _packed(_ResPackCache, weights, ("hg_filter",) + tuple(cfg), lambda: ops.hg_filter_pack(tensors, cfg))


@_lib.custom_op("kpnerf::hg_filter_cl", mutates_args=(), device_types="cuda")
def hg_filter_cl(x: torch.Tensor, tensors: List[torch.Tensor], depth: int, eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(out, x_hd, state) of an HGFilterV2 for a contiguous NCHW x (kpn_hg_filter_forward): what torch.ops.kpnerf.hg_filter runs after its
    memory-format conversion.  out is (N, out_ch, H / 4, W / 4) and x_hd (N, out_ch_hd, H, W), channels_last; state is the side buffer of
    the backward."""
    cfg = _hg_cfg(x, tensors, depth)
    return ops.hg_filter_forward(x, tensors, _hg_packed(tensors, cfg), cfg, eps)


@hg_filter_cl.register_fake
def _(x, tensors, depth, eps):
    cfg = _hg_cfg(x, tensors, depth)
    N, _, H, W = x.shape
    return (x.new_empty(N, H // 4, W // 4, cfg[8]).permute(0, 3, 1, 2), x.new_empty(N, H, W, cfg[7]).permute(0, 3, 1, 2),
            x.new_empty(ops.hg_filter_state_floats(N, H, W, cfg)))


@_lib.custom_op("kpnerf::hg_filter_backward", mutates_args=(), device_types="cuda")
def hg_filter_backward(x: torch.Tensor, tensors: List[torch.Tensor], state: torch.Tensor, d_out: Optional[torch.Tensor],
                       d_x_hd: Optional[torch.Tensor], depth: int, eps: float, mask: List[bool]) -> List[torch.Tensor]:
    """one gradient per tensor of kpnerf::hg_filter_cl for the output gradients d_out and d_x_hd, either of which may be None
    (kpn_hg_filter_backward); mask has one flag per tensor: what is not wanted is not computed and its result is an empty tensor."""
    cfg = _hg_cfg(x, tensors, depth)
    cl = torch.channels_last
    d_out = None if d_out is None else d_out.contiguous(memory_format=cl)
    d_x_hd = None if d_x_hd is None else d_x_hd.contiguous(memory_format=cl)
    grads = ops.hg_filter_backward(x, d_out, d_x_hd, tensors, _hg_packed(tensors, cfg), state, cfg, eps, want=mask)
    return list(_empty_for_none(x, *grads))


@hg_filter_backward.register_fake
def _(x, tensors, state, d_out, d_x_hd, depth, eps, mask):
    return [torch.empty_like(t) if m else x.new_empty(0) for t, m in zip(tensors, mask)]


def _hg_filter_setup(ctx, inputs, output):
    x, tensors, depth, eps = inputs
    if ctx.needs_input_grad[0]:
        raise RuntimeError("kpnerf::hg_filter: the 7x7 stem has no input gradient (x.requires_grad is set)")
    ctx.save_for_backward(x, output[2], *tensors)                                # never an output, never a normalised tensor
    ctx.cfg = (depth, eps)
    ctx.set_materialize_grads(False)


def _hg_filter_bwd(ctx, d_out, d_x_hd, _d_state):
    x, state, *tensors = ctx.saved_tensors
    none = (None, [None] * len(tensors), None, None)
    mask = [bool(b) for b in ctx.needs_input_grad[1]]
    if (d_out is None and d_x_hd is None) or not any(mask):
        return none
    out = torch.ops.kpnerf.hg_filter_backward(x, list(tensors), state, d_out, d_x_hd, *ctx.cfg, mask)
    return None, list(_none_unless(mask, *out)), None, None


hg_filter_cl.register_autograd(_hg_filter_bwd, setup_context=_hg_filter_setup)


# torch.ops.kpnerf.hg_filter(x, tensors, depth, eps) -> [out, x_hd]: x in any memory format, converted once to the contiguous NCHW layout
# the stem reads as it is; the results are channels_last.
def _hg_filter(x, tensors, depth, eps):
    out, x_hd, _ = torch.ops.kpnerf.hg_filter_cl(x.contiguous(), tensors, depth, eps)
    return [out, x_hd]


_fragment.define("hg_filter(Tensor x, Tensor[] tensors, int depth, float eps) -> Tensor[]")
_fragment.impl("hg_filter", _hg_filter, "CompositeImplicitAutograd")


# ---- torch.ops.kpnerf.avg_pool2 / upsample2x_add: the two resampling steps of an HourGlass, DIFFERENTIABLE ----
# Neither backward reads a forward tensor: the pool's gradient is 0.25 dy under each window, the upsample's is the transposed
# interpolation of dy as a gather in a fixed order (no atomics: bit-identical from run to run) and dy itself for the skip.
@_lib.custom_op("kpnerf::avg_pool2_cl", mutates_args=(), device_types="cuda")
def avg_pool2_cl(x: torch.Tensor) -> torch.Tensor:
    """avg_pool2d(x, 2, stride=2) for a channels_last x (N, C, 2h, 2w), C a multiple of 4 (kpn_avg_pool2_forward): what
    torch.ops.kpnerf.avg_pool2 runs after its memory-format conversion.  Returns (N, C, h, w) channels_last."""
    return ops.avg_pool2_forward(x)


@avg_pool2_cl.register_fake
def _(x):
    N, C, H, W = x.shape
    return x.new_empty(N, H // 2, W // 2, C).permute(0, 3, 1, 2)


@_lib.custom_op("kpnerf::avg_pool2_backward", mutates_args=(), device_types="cuda")
def avg_pool2_backward(dy: torch.Tensor) -> torch.Tensor:
    """dx (N, C, 2h, 2w) channels_last of kpnerf::avg_pool2_cl for the output gradient dy (N, C, h, w) (kpn_avg_pool2_backward)"""
    return ops.avg_pool2_backward(dy.contiguous(memory_format=torch.channels_last))


@avg_pool2_backward.register_fake
def _(dy):
    N, C, h, w = dy.shape
    return dy.new_empty(N, 2 * h, 2 * w, C).permute(0, 3, 1, 2)


def _avg_pool2_bwd(ctx, dy):
    if dy is None or not ctx.needs_input_grad[0]:
        return None
    return torch.ops.kpnerf.avg_pool2_backward(dy)


avg_pool2_cl.register_autograd(_avg_pool2_bwd)


@_lib.custom_op("kpnerf::upsample2x_add_cl", mutates_args=(), device_types="cuda")
def upsample2x_add_cl(low: torch.Tensor, skip: Optional[torch.Tensor]) -> torch.Tensor:
    """skip + interpolate(low, scale_factor=2, mode="bicubic", align_corners=True) for channels_last low (N, C, h, w) and skip
    (N, C, 2h, 2w), or the interpolation alone for skip = None; C a multiple of 4 (kpn_upsample2x_add_forward): what
    torch.ops.kpnerf.upsample2x_add runs after its memory-format conversion.  Returns (N, C, 2h, 2w) channels_last."""
    return ops.upsample2x_add_forward(low, skip)


@upsample2x_add_cl.register_fake
def _(low, skip):
    N, C, h, w = low.shape
    return low.new_empty(N, 2 * h, 2 * w, C).permute(0, 3, 1, 2)


@_lib.custom_op("kpnerf::upsample2x_add_backward", mutates_args=(), device_types="cuda")
def upsample2x_add_backward(dy: torch.Tensor) -> torch.Tensor:
    """d_low (N, C, h, w) channels_last of kpnerf::upsample2x_add_cl for the output gradient dy (N, C, 2h, 2w)
    (kpn_upsample2x_add_backward)"""
    return ops.upsample2x_add_backward(dy.contiguous(memory_format=torch.channels_last))


@upsample2x_add_backward.register_fake
def _(dy):
    N, C, H, W = dy.shape
    return dy.new_empty(N, H // 2, W // 2, C).permute(0, 3, 1, 2)


def _upsample2x_add_bwd(ctx, dy):
    if dy is None:
        return None, None
    need = ctx.needs_input_grad
    d_low = torch.ops.kpnerf.upsample2x_add_backward(dy) if need[0] else None      # computed only if low needs it
    return d_low, (dy if need[1] else None)                                        # the skip's gradient is dy itself


upsample2x_add_cl.register_autograd(_upsample2x_add_bwd)


# torch.ops.kpnerf.avg_pool2(x) / upsample2x_add(low, skip): tensors in any memory format, converted to channels_last once (as
# kpnerf::conv2d does); the results are channels_last.
def _avg_pool2(x):
    return torch.ops.kpnerf.avg_pool2_cl(x.contiguous(memory_format=torch.channels_last))


def _upsample2x_add(low, skip):
    cl = torch.channels_last
    return torch.ops.kpnerf.upsample2x_add_cl(low.contiguous(memory_format=cl), None if skip is None else skip.contiguous(memory_format=cl))


_fragment.define("avg_pool2(Tensor x) -> Tensor")
_fragment.impl("avg_pool2", _avg_pool2, "CompositeImplicitAutograd")
_fragment.define("upsample2x_add(Tensor low, Tensor? skip) -> Tensor")
_fragment.impl("upsample2x_add", _upsample2x_add, "CompositeImplicitAutograd")
