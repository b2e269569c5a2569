"""Training loss of the reference (compute_error / compute_error_nerf / pix_loss, reference src/utils.py:97-196) with every
pixel and mask term on the device — SURVEY.md §8(f) row 3.

``compute_error(out_nerf, vggloss, lambdas)`` has the reference's signature, returns the reference's ``(loss, err_dict)``
with the reference's keys in the reference's order (``e_pix_c``, ``e_pix_l1``, ``e_pix_l2``, ``e_pix_lp``, ``mask_loss_c``,
``mask_loss_f``, ``e_vgg``, ``e_all``, each under the reference's condition) and is differentiable.  For CUDA fp32 tensors of
batch size 1 all pixel and mask terms — the coarse and fine L1 terms (configs/zju.json:109-112), l2, lp and the two mask
losses (``lambda_l2`` / ``lambda_lp`` / ``lambda_mloss``) — are ONE call of ``torch.ops.kpnerf.train_loss``: one kernel computes
the six values and their seed gradients, the backward only scales what the forward saved, so ``loss.backward()`` hands
``kpn_render_rays_train_backward`` its ``d_tex_fg`` / ``d_tex_fg_fine`` / ``d_alpha`` / ``d_alpha_fine`` without eager elementwise
passes.  Anything else (CPU tensors, batch > 1, another dtype) takes the per-term path: ``torch.ops.kpnerf.pix_l1_loss`` for L1
and the reference's eager formulas for the rest.  The perceptual term stays the caller's ``vggloss`` module (a pretrained
torchvision VGG19 — model weights that are not part of this path; its gradient joins ``d_tex_fg_fine`` through autograd).
An ssim weight and `*top*` lambdas have no effect, as in the reference; only the auxiliary texture heads (never produced by
this renderer) are refused.

``install_loss(module)`` rebinds the module-global ``compute_error`` that ``KeypointNeRF.forward`` looks up
(reference src/model.py:894) — the same kind of seam as dropin.install uses for the renderer.
"""
import torch

from . import torch_ops  # noqa: F401  (registers torch.ops.kpnerf.*)


def pix_loss(src, tar, w_losses={"l1": 1.0}):
    """reference src/utils.py:173-196: the L1 term (the one configs/zju.json switches on) is one device kernel; l2 / lp keep the
    reference's eager formulas; an "ssim" weight is ignored exactly as the reference ignores it (its pix_loss has no such
    branch).  The top-k terms cannot occur: compute_error_nerf collects the `*top*` lambdas but never passes them on (:124-127)."""
    losses = {}
    for k, v in w_losses.items():
        if v <= 0.0:
            continue
        if k == "l1":
            losses[k] = torch.ops.kpnerf.pix_l1_loss(src.contiguous(), tar.contiguous(), float(v))[0]
        elif k == "l2":
            losses[k] = v * (src - tar).pow(2.0).mean()
        elif k == "lp":
            losses[k] = v * ((src - tar).abs() + 1e-4).pow(0.4).mean()
    return losses


_on_device = lambda t: t.is_cuda
_FUSED_KEYS = ("tex_cal", "tex_cal_fine", "tar_img", "alpha", "alpha_fine", "tar_alpha")


def _fusable(out_nerf):
    """one kpn_train_loss call serves these outputs: CUDA fp32, batch 1, the shapes batch_render_pifu_nerf produces"""
    tar = out_nerf.get("tar_img")
    if tar is None or tar.dim() < 1 or tar.shape[0] != 1 or tar.numel() == 0 or tar.numel() % 3:
        return False
    n = tar.numel() // 3
    for k in _FUSED_KEYS:
        t = out_nerf.get(k)
        if t is None:
            continue
        if not (isinstance(t, torch.Tensor) and _on_device(t) and t.dtype == torch.float32):
            return False
        if t.numel() != (3 * n if k.startswith("tex") or k == "tar_img" else n):
            return False
    return True


def _fused_terms(out_nerf, lambda_l1_c, pix_weights, lambda_mloss):
    """err_dict of the pixel and mask terms from one torch.ops.kpnerf.train_loss call"""
    c = lambda k: out_nerf[k].contiguous() if k in out_nerf else None
    tex, tex_fine = c("tex_cal"), c("tex_cal_fine")
    ta = c("tar_alpha")
    alpha, alpha_fine = (c("alpha"), c("alpha_fine")) if ta is not None else (None, None)
    w = [float(lambda_l1_c), float(pix_weights["l1"]), float(pix_weights["l2"]), float(pix_weights["lp"]), float(lambda_mloss)]
    on = torch_ops._train_loss_active((tex, tex_fine, None, alpha, alpha_fine, ta, w))
    if not any(on):
        return {}
    terms = torch.ops.kpnerf.train_loss(tex, tex_fine, out_nerf["tar_img"].contiguous(), alpha, alpha_fine, ta, w)[0].unbind(0)
    err_dict = {}
    if on[0] and terms[0] > 0.0:                  # the reference's own test, src/utils.py:136 (one host sync, as there)
        err_dict["e_pix_c"] = terms[0]
    for k, name in enumerate(("e_pix_l1", "e_pix_l2", "e_pix_lp", "mask_loss_c", "mask_loss_f")):
        if on[1 + k]:
            err_dict[name] = terms[1 + k]
    return err_dict


def _per_term(out_nerf, lambda_l1_c, pix_weights, lambda_mloss):
    """the same err_dict term by term: pix_l1_loss for L1, the reference's eager formulas for the rest"""
    err_dict = {}
    if "tex_cal" in out_nerf and lambda_l1_c > 0.0:
        loss_pix_c = pix_loss(out_nerf["tex_cal"], out_nerf["tar_img"], {"l1": lambda_l1_c})["l1"]
        if loss_pix_c > 0.0:
            err_dict["e_pix_c"] = loss_pix_c
    if "tex_cal_fine" in out_nerf:
        for k, v in pix_loss(out_nerf["tex_cal_fine"], out_nerf["tar_img"], pix_weights).items():
            err_dict[f"e_pix_{k}"] = v
    if "tar_alpha" in out_nerf and lambda_mloss > 0.0:
        for key, name in (("alpha", "mask_loss_c"), ("alpha_fine", "mask_loss_f")):
            if key in out_nerf:
                err_dict[name] = lambda_mloss * torch.nn.functional.mse_loss(out_nerf[key].clip(1e-3, 1.0).squeeze(),
                                                                            out_nerf["tar_alpha"].squeeze())
    return err_dict


def compute_error_nerf(out_nerf, lambdas, vggloss):
    """reference src/utils.py:108-171 for the outputs batch_render_pifu_nerf produces (no aux heads): same keys under the same
    conditions — e_pix_c only when it is > 0 (:141, one host sync as there), the mask losses when tar_alpha is present and
    lambda_mloss > 0 (:155-163), `*top*` lambdas without effect (:124-127)."""
    lambda_l1_c = lambdas.get("lambda_l1_c", 10.0)
    pix_weights = {"l1": lambdas.get("lambda_l1", 10.0), "l2": lambdas.get("lambda_l2", 0.0), "lp": lambdas.get("lambda_lp", 0.0),
                   "ssim": lambdas.get("lambda_ssim", 0.0)}
    lambda_vgg = lambdas.get("lambda_vgg", 1.0)
    lambda_mloss = lambdas.get("lambda_mloss", 0.0)
    if "tex_aux_cal" in out_nerf or "tex_aux_cal_fine" in out_nerf:
        raise NotImplementedError("auxiliary texture heads are not produced by batch_render_pifu_nerf")
    if _fusable(out_nerf):
        err_dict = _fused_terms(out_nerf, lambda_l1_c, pix_weights, lambda_mloss)
    else:
        err_dict = _per_term(out_nerf, lambda_l1_c, pix_weights, lambda_mloss)
    if vggloss is not None and "tex_cal_fine" in out_nerf:
        loss_vgg = lambda_vgg * vggloss(out_nerf["tex_cal_fine"], out_nerf["tar_img"])
        if loss_vgg > 0.0:                       # the reference's own test, src/utils.py:168 (one host sync, as there)
            err_dict["e_vgg"] = loss_vgg
    return err_dict


def compute_error(out_nerf=None, vggloss=None, lambdas={}):
    """reference src/utils.py:97-106."""
    err_dict = compute_error_nerf(out_nerf, lambdas, vggloss)
    loss = 0.0
    for v in err_dict.values():
        loss = loss + v
    err_dict["e_all"] = loss
    return loss, err_dict


def install_loss(model_module):
    """Rebinds ``compute_error`` in the namespace KeypointNeRF.forward resolves it in (``src.model``); returns the
    reference's function so that it can be restored."""
    ref = model_module.compute_error
    model_module.compute_error = compute_error
    return ref
