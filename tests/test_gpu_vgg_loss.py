"""The native VGG perceptual term (kpn_vgg_loss; reference VGGLoss, src/utils.py:750-805) on the MI355X: the three parity
rules on every recorded golden case (fp64 oracle on the CPU, tests/vgg_golden.py), the exact properties, the same e_vgg as
the same-weight module through MIOpen, the gradient through compute_error / autograd, and a drop-in training step."""
import os

import numpy as np
import pytest
import torch

from tests import vgg_golden as vg
from tests.golden_io import GOLDEN_DIR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(GOLDEN_DIR, "case_v_vgg_loss.npz")


@pytest.fixture(scope="module")
def packed():
    from keypointnerf_amd import ops
    g = np.load(GOLDEN)
    feats = vg.features(int(g["seed"]))
    vg.check_checksums(feats, g["checksums"])
    return ops.vgg_pack(vg.plain(feats).cuda()), vg.conv_params(feats), g


def run(packed, x, y, lam=1.0, tap_w=vg.TAP_W, grad=True, stages=False):
    from keypointnerf_amd import ops
    loss, dx, st = ops.vgg_loss(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), packed[0], vg.MEAN, vg.STD, tap_w, lam,
                                want_grad=grad, want_stages=stages)
    torch.cuda.synchronize()
    return (loss.cpu().numpy(), None if dx is None else dx.cpu().numpy(), None if st is None else st.cpu().numpy())


@pytest.mark.parametrize("case", ["c32", "c64", "c19x27", "half32"])
def test_parity_rules_on_the_reference_golden(packed, case):
    params, g = packed[1], packed[2]
    x, y = g[f"{case}_x"], g[f"{case}_y"]
    B, _, H, W = x.shape
    loss, dx, st = run(packed, x, y, stages=True)
    S = vg.stages_nchw(st, B, H, W)
    worst, l_own = vg.rule1(x, y, S, params, B)
    assert worst <= 1.0, worst
    assert abs(float(loss) - l_own) <= 1e-6 * abs(l_own)
    dm = vg.decision_matched_backward(S, params, B).numpy()
    assert np.linalg.norm(dx - dm) <= 1e-5 * np.linalg.norm(dm)
    assert np.abs(dx - dm).max() <= 1e-4 * np.abs(dm).max()
    e_loss, cos, e_loss32, cos32 = vg.end_to_end(loss, dx, g, case)
    n_diff, n_out = vg.differing_decisions(S, *vg.reference64(x, y, params), B)
    print(f"{case}: rule 1 worst {worst:.3f} of the bound; loss rel err {e_loss:.2e} (reference fp32: {e_loss32:.2e}), d_x cosine "
          f"{cos:.9f} (reference fp32: {cos32:.9f}), differing decisions {n_diff}, outside the rule-1 margin {n_out}")
    assert e_loss <= 1e-5 and cos >= 0.9999 and n_out == 0


def test_exact_properties(packed):
    rng = np.random.default_rng(6)
    a, b = rng.random((1, 3, 64, 64), dtype=np.float32), rng.random((1, 3, 64, 64), dtype=np.float32)
    loss, dx, _ = run(packed, a, a.copy())
    assert loss == 0.0 and np.all(dx == 0.0)
    x, y = np.concatenate([a, a]), np.concatenate([b, b])
    loss, dx, st = run(packed, x, y, stages=True)
    assert np.array_equal(dx[0], dx[1])
    S = vg.stages_nchw(st, 2, 64, 64)
    assert all(torch.equal(s[0], s[1]) and torch.equal(s[2], s[3]) for s in S)
    loss2, dx2, st2 = run(packed, x, y, stages=True)
    assert loss2.tobytes() == loss.tobytes() and np.array_equal(dx2, dx) and np.array_equal(st2, st)
    loss3, _, _ = run(packed, x, y, grad=False)
    assert loss3.tobytes() == loss.tobytes()
    loss4, dx4, _ = run(packed, x, y, lam=2.0)
    assert loss4 == 2 * loss and np.array_equal(dx4, 2 * dx)


def test_compute_error_matches_the_miopen_module_and_delivers_the_gradient():
    from keypointnerf_amd import ops
    from keypointnerf_amd.losses import compute_error
    from keypointnerf_amd.vgg import NativeVGGLoss
    m = vg.StandInVGGLoss().cuda()
    torch.manual_seed(1)
    tar = torch.rand(1, 3, 64, 64, device="cuda")
    tex = torch.rand(1, 3, 64, 64, device="cuda", requires_grad=True)
    lam = {"lambda_l1_c": 0.0, "lambda_l1": 10.0, "lambda_vgg": 0.5}
    loss, err = compute_error(out_nerf={"tex_cal_fine": tex, "tar_img": tar}, vggloss=NativeVGGLoss(m), lambdas=lam)
    loss.backward()
    ref_tex = tex.detach().clone().requires_grad_(True)
    _, err_ref = compute_error(out_nerf={"tex_cal_fine": ref_tex, "tar_img": tar}, vggloss=m, lambdas=lam)
    e_ref = float(err_ref["e_vgg"])
    assert abs(float(err["e_vgg"]) - e_ref) <= 1e-5 * e_ref
    _, d_l1 = ops.pix_l1_loss(tex.detach(), tar, 10.0)
    _, d_vgg, _ = ops.vgg_loss(tex.detach(), tar, NativeVGGLoss(m).packed_weights(tex.device), vg.MEAN, vg.STD, vg.TAP_W, 1.0)
    want = d_l1 + 0.5 * d_vgg
    assert torch.allclose(tex.grad, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    err_ref["e_vgg"].backward()
    cos = float((d_vgg * ref_tex.grad).sum() / (d_vgg.norm() * ref_tex.grad.norm()))
    assert cos >= 0.9999


def test_dropin_training_step_with_the_native_vgg_term():
    from keypointnerf_amd.dropin import install
    from keypointnerf_amd.losses import compute_error
    from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict, to_device
    from keypointnerf_amd.vgg import install_vgg
    from scripts.bench_dropin_train import Carrier
    dev = torch.device("cuda", 0)
    s = to_device(make_scene(n_views=3, src_hw=(128, 128), tar_hw=(128, 128), mask="ellipsoid", seed=1, tar_focal_at_512=800.0), dev)
    net = install(Carrier(random_hotpath_state_dict(seed=3), s).to(dev))
    net.vgg_loss = vg.StandInVGGLoss().to(dev)
    install_vgg(net)
    net.train()
    net.train_out_h = net.train_out_w = 32
    yy, xx = torch.meshgrid(torch.arange(128), torch.arange(128), indexing="ij")
    msk = (((yy - 64) ** 2 + (xx - 64) ** 2) < 40 ** 2)[None, None].to(dev)
    feat_tex = s["feat_tex"].clone().requires_grad_(True)
    np.random.seed(0)
    torch.manual_seed(0)
    out = net.batch_render_pifu_nerf(net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=5, stride=0,
                                     tar_img=torch.rand(1, 3, 128, 128, device=dev), bg_img=None, feat_geo=s["feat_geo"],
                                     feat_tex=feat_tex, sp_data=dict(s["sp_data"]), camcenter=None, objcenter=None, msk=msk,
                                     src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"], fine=True, uniform=False,
                                     blur=3, sample_per_ray_c=16, sample_per_ray_f=16, rand_noise_std=0.01)
    out["tex_cal"], out["tex_cal_fine"] = out["tex_fg"], out["tex_fg_fine"]
    loss, err = compute_error(out_nerf=out, vggloss=net.vgg_loss, lambdas={"lambda_l1_c": 1.0, "lambda_l1": 10.0, "lambda_vgg": 0.5})
    loss.backward()
    assert "e_vgg" in err and torch.isfinite(loss)
    grads = [p.grad for p in net.parameters() if p.grad is not None] + [feat_tex.grad]
    assert grads and all(bool(torch.isfinite(g_).all()) for g_ in grads)
    assert any(float(g_.abs().sum()) > 0 for g_ in grads)
