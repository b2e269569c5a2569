"""Hot-path parameters: from the reference's (unchanged) state-dict / module tree to kernel operands.

The checkpoint format is untouched: parameters are read by the reference's own
names — ``mlp_geo.layers1.layers.N.linear.{weight_g,weight_v,bias}``, ``ibr_compress_gfeat.*``,
``mlp_tex.*`` — optionally behind the Lightning prefix ``model.`` (reference src/model.py:42).

Two products:
  * ``effective_weights``: weight-norm folded, plain row-major (out,in) fp32 matrices
    (``w = g * v / ||v||_row``, reference src/utils.py:542-543 via torch.nn.utils.weight_norm dim=0);
  * ``pack_for_mfma``: the same matrices re-ordered into the A-operand stream of
    ``v_mfma_f32_32x32x2_f32`` as consumed by csrc/field_kernels.hip.
"""
import numpy as np
import torch

from .synthetic import HOTPATH_LAYERS, N_KPT, SP_LEVEL, hotpath_layers

CANONICAL_SHAPE = (N_KPT, SP_LEVEL)


def field_shape(net):
    """(n_kpt, sp_level) of a live module's spatial encoder (reference src/spatial.py:10-21): the keypoint count and the octaves
    that size the first linear of mlp_geo (src/spatial.py:49-53, src/model.py:569-572).  A module without an encoder object is
    taken for the shipped 24 / 3 model."""
    enc = getattr(net, "sp_encoder", None)
    if enc is None:
        return CANONICAL_SHAPE
    return int(getattr(enc, "n_kpt", N_KPT)), int(getattr(enc, "sp_level", SP_LEVEL))


def _layers(shape):
    """HOTPATH_LAYERS of a (n_kpt, sp_level) model; None = the shipped one"""
    return HOTPATH_LAYERS if shape is None or tuple(shape) == CANONICAL_SHAPE else hotpath_layers(*shape)


def canonical_columns(shape):
    """Per column of the narrow (128, D + 64) first-layer weight of a (n_kpt, sp_level) model its column in the kernels' 24 / 3
    layout: encoding value (block t, keypoint k) t n_kpt + k -> 24 t + k, geometry channel D + j -> 168 + j (include/kpnerf.h,
    "Keypoint sets")."""
    n, L = int(shape[0]), int(shape[1])
    return np.array([N_KPT * t + k for t in range(1 + 2 * L) for k in range(n)] + [(1 + 2 * SP_LEVEL) * N_KPT + j for j in range(64)],
                    dtype=np.int64)


def widen_plain_host(narrow, shape):
    """The narrow plain vector (flatten_plain of a (n_kpt, sp_level) model) as the kernels' plain vector, on the host: zeros in the
    padded columns of g1_0 (what kpn_widen_plain does on the device)."""
    narrow = np.ascontiguousarray(narrow, dtype=np.float32).reshape(-1)
    cols = canonical_columns(shape)
    rows, wide = HOTPATH_LAYERS[0][2]
    w = np.zeros((rows, wide), np.float32)
    w[:, cols] = narrow[:rows * cols.size].reshape(rows, cols.size)
    return np.ascontiguousarray(np.concatenate([w.reshape(-1), narrow[rows * cols.size:]]), dtype=np.float32)


def _strip_prefix(sd):
    if any(k.startswith("model.") for k in sd):
        return {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    return sd


def effective_weights(state_dict, shape=None):
    """dict name -> (W (out,in) float32 numpy, b (out,) float32 numpy); plus 'ani_al' -> float.  shape = (n_kpt, sp_level) of the
    model (None: the shipped 24 / 3): g1_0 is then the narrow (128, (1 + 2 sp_level) n_kpt + 64) matrix."""
    sd = _strip_prefix(state_dict)
    out = {}
    for name, prefix, shape, wn in _layers(shape):
        if wn and (prefix + ".weight_g") in sd:
            g = sd[prefix + ".weight_g"].detach().float().cpu()
            v = sd[prefix + ".weight_v"].detach().float().cpu()
            w = torch._weight_norm(v, g, 0)
        elif (prefix + ".parametrizations.weight.original0") in sd:  # new-style weight_norm
            g = sd[prefix + ".parametrizations.weight.original0"].detach().float().cpu()
            v = sd[prefix + ".parametrizations.weight.original1"].detach().float().cpu()
            w = torch._weight_norm(v, g, 0)
        else:
            w = sd[prefix + ".weight"].detach().float().cpu()
        b = sd[prefix + ".bias"].detach().float().cpu()
        if tuple(w.shape) != tuple(shape) or b.shape[0] != shape[0]:
            raise ValueError(
                f"unsupported architecture: {prefix} has shape {tuple(w.shape)}, the HIP path is built "
                f"for {shape} (configs/zju.json of the reference; the first layer's width follows n_kpt / sp_level)")
        out[name] = (np.ascontiguousarray(w.numpy(), dtype=np.float32),
                     np.ascontiguousarray(b.numpy(), dtype=np.float32))
    out["ani_al"] = float(sd["mlp_tex.ani_al"].detach().float().cpu())
    return out


def flatten_plain(eff):
    """Flat fp32 vector in HOTPATH_LAYERS order: for each layer W row-major then b; then |ani_al|
    is NOT folded: the raw ani_al is appended last.  This is the layout the C oracle reads
    (oracle/kpnerf_oracle.c: struct kpo_weights offsets are derived from the same table)."""
    parts = []
    for name, _, _, _ in HOTPATH_LAYERS:
        w, b = eff[name]
        parts.append(w.reshape(-1))
        parts.append(b.reshape(-1))
    parts.append(np.array([eff["ani_al"]], dtype=np.float32))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def plain_grads_to_state_dict(state_dict, d_plain, shape=None):
    """Gradient w.r.t. the flat effective parameters (the layout of ``flatten_plain``; what
    ``kpn_geo_rows_backward`` accumulates) -> gradient w.r.t. the reference's own parameters
    (``weight_g`` / ``weight_v`` / ``bias`` / ``weight``), by differentiating the weight-norm fold
    ``torch._weight_norm(v, g, 0)`` (reference src/utils.py:542-543).  Returns {state-dict key: grad tensor}.
    shape = (n_kpt, sp_level) of the model: d_plain is then the gradient of the NARROW plain vector (kpn_narrow_plain_grad)."""
    sd = _strip_prefix(state_dict)
    d_plain = torch.as_tensor(d_plain).detach().float().cpu()
    grads, off = {}, 0
    for name, prefix, shape, wn in _layers(shape):
        n = shape[0] * shape[1]
        dW = d_plain[off:off + n].reshape(shape); off += n
        db = d_plain[off:off + shape[0]]; off += shape[0]
        grads[prefix + ".bias"] = db.clone()
        if wn and (prefix + ".weight_g") in sd:
            g = sd[prefix + ".weight_g"].detach().float().cpu().requires_grad_(True)
            v = sd[prefix + ".weight_v"].detach().float().cpu().requires_grad_(True)
            dg, dv = torch.autograd.grad(torch._weight_norm(v, g, 0), [g, v], dW)
            grads[prefix + ".weight_g"], grads[prefix + ".weight_v"] = dg, dv
        elif (prefix + ".parametrizations.weight.original0") in sd:
            g = sd[prefix + ".parametrizations.weight.original0"].detach().float().cpu().requires_grad_(True)
            v = sd[prefix + ".parametrizations.weight.original1"].detach().float().cpu().requires_grad_(True)
            dg, dv = torch.autograd.grad(torch._weight_norm(v, g, 0), [g, v], dW)
            grads[prefix + ".parametrizations.weight.original0"], grads[prefix + ".parametrizations.weight.original1"] = dg, dv
        else:
            grads[prefix + ".weight"] = dW.clone()
    grads["mlp_tex.ani_al"] = d_plain[off:off + 1].clone()
    return grads


def plain_tensor_from_module(net):
    """The flat effective-parameter vector (``flatten_plain`` layout) as a DIFFERENTIABLE torch tensor built from a
    live module's parameters: weight-norm folded with ``torch._weight_norm`` (reference src/utils.py:542-543), raw
    ``ani_al`` last.  Gradients of a loss w.r.t. this tensor reach ``weight_g`` / ``weight_v`` / ``weight`` / ``bias``
    through autograd — this is how the training drop-in hands the library's ``d_plain`` to the optimizer.
    A model with fewer keypoints or octaves (``field_shape``) is folded on its own narrow first-layer tensor and then widened to
    the kernels' layout by ``torch.ops.kpnerf.widen_plain`` (one launch; its backward gathers the gradient back)."""
    params = dict(net.named_parameters())
    if any(k.startswith("model.") for k in params):
        params = {k[len("model."):]: v for k, v in params.items() if k.startswith("model.")}
    parts = []
    fshape = field_shape(net)
    for name, prefix, shape, wn in _layers(fshape):
        if (prefix + ".weight_g") in params:
            w = torch._weight_norm(params[prefix + ".weight_v"], params[prefix + ".weight_g"], 0)
        elif (prefix + ".parametrizations.weight.original0") in params:
            w = torch._weight_norm(params[prefix + ".parametrizations.weight.original1"],
                                   params[prefix + ".parametrizations.weight.original0"], 0)
        else:
            w = params[prefix + ".weight"]
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"unsupported architecture: {prefix} has shape {tuple(w.shape)}, expected {shape}")
        parts += [w.reshape(-1).float(), params[prefix + ".bias"].reshape(-1).float()]
    parts.append(params["mlp_tex.ani_al"].reshape(1).float())
    if fshape == CANONICAL_SHAPE:
        return torch.cat(parts)
    from . import torch_ops  # noqa: F401  (registers torch.ops.kpnerf.*)
    return torch.ops.kpnerf.widen_plain(torch.cat(parts), fshape[0], fshape[1])


def hot_tensor_names(params, shape=None):
    """The 44 hot-path tensors of ``params`` (a name -> tensor mapping, Lightning's ``model.`` prefix already stripped) in the
    order of the C ABI's ``kpn_param_table``: per layer of HOTPATH_LAYERS ``weight_g, weight_v, bias`` (either weight-norm
    spelling: ``weight_g`` / ``weight_v`` or ``parametrizations.weight.original0`` / ``original1``) or ``weight, bias``; then
    ``mlp_tex.ani_al``.  The weight-normed layers must be the reference's (src/utils.py:542-543).  shape = (n_kpt, sp_level) of
    the model (None: 24 / 3): the first layer's ``weight_v`` is then the narrow tensor ``kpn_fold_params_shape`` takes."""
    names = []
    for name, prefix, shape, wn in _layers(shape):
        if (prefix + ".weight_g") in params:
            gv = [prefix + ".weight_g", prefix + ".weight_v"]
        elif (prefix + ".parametrizations.weight.original0") in params:
            gv = [prefix + ".parametrizations.weight.original0", prefix + ".parametrizations.weight.original1"]
        else:
            gv = [prefix + ".weight"]
        if (len(gv) == 2) != wn:
            raise ValueError(f"unsupported architecture: {prefix} is {'not ' if wn else ''}weight-normed in the reference")
        if tuple(params[gv[-1]].shape) != tuple(shape):
            raise ValueError(f"unsupported architecture: {prefix} has shape {tuple(params[gv[-1]].shape)}, expected {shape}")
        names += gv + [prefix + ".bias"]
    return names + ["mlp_tex.ani_al"]


def live_parameters(net):
    """name -> parameter of a live module, Lightning's ``model.`` prefix stripped (as ``_strip_prefix`` does for a state dict)"""
    return _strip_prefix(dict(net.named_parameters()))


def hot_tensors(net):
    """``hot_tensor_names`` resolved on a live module: the list ``torch.ops.kpnerf.fold_params`` takes."""
    params = live_parameters(net)
    return [params[n] for n in hot_tensor_names(params, field_shape(net))]


def plain_tensor_native(net):
    """``plain_tensor_from_module``'s contract — the flat effective-parameter vector as a differentiable tensor of the live
    parameters — in one launch (``torch.ops.kpnerf.fold_params`` = kpn_fold_params), and one more in ``loss.backward()``
    (kpn_fold_params_backward), instead of the cat's and the five weight-norms' autograd graph."""
    from . import torch_ops  # noqa: F401  (registers torch.ops.kpnerf.*)
    shape = field_shape(net)
    if shape == CANONICAL_SHAPE:
        return torch.ops.kpnerf.fold_params(hot_tensors(net))
    return torch.ops.kpnerf.fold_params_shape(hot_tensors(net), shape[0], shape[1])
