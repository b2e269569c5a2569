"""The parameter step on the device: the kernel checks of tests/test_param_step_cpu.py through the product library (cases and
bars: tests/param_step_cases.py), and a 5-step training loop through install(net, native_params=True) + keypointnerf_amd.optim.Adam
against the same loop on the default path + torch.optim.Adam."""
import ctypes

import numpy as np
import pytest
import torch

from tests import param_step_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from keypointnerf_amd import lib as kl

    def to_host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return pc.Driver(kl.get_library(), to_dev=lambda a: torch.from_numpy(np.array(a)).cuda(), ptr=lambda t: ctypes.c_void_p(t.data_ptr()),
                     to_host=to_host, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_fold_against_fp64(drv):
    pc.check_fold(drv)


def test_fold_backward_against_fp64_overwrite_and_accumulate(drv):
    pc.check_backward(drv)


@pytest.mark.parametrize("step,wd", [(1, 0.0), (1, 0.01), (1000, 0.0), (1000, 0.01)])
def test_adam_one_step_against_fp64(drv, step, wd):
    pc.check_adam_one_step(drv, step, wd)


def test_adam_trajectory_no_further_from_fp64_than_twice_torch(drv):
    pc.check_adam_trajectory(drv)


def test_same_bytes_in_same_bytes_out(drv):
    pc.check_determinism(drv)


def test_bad_tables_are_error_codes(drv):
    pc.check_bad_tables(drv)


LR, STEPS = 1e-3, 5
LAMBDAS = {"lambda_l1_c": 1.0, "lambda_l1": 10.0}


def _loop(native):
    """5 training steps at 32 x 32 rays, 16 + 16 samples -> (losses, initial parameters, final parameters, per step the gradients
    the optimizer saw, the drop-in's state)"""
    from keypointnerf_amd import losses, optim
    from keypointnerf_amd.dropin import install
    from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict
    from tests.test_gpu_dropin import StandInNet
    s = make_scene(n_views=3, src_hw=(128, 128), tar_hw=(64, 64), mask="ellipsoid", seed=5, tar_focal_at_512=800.0, device="cuda")
    net = StandInNet(random_hotpath_state_dict(seed=3), s).cuda()
    install(net, native_params=True) if native else install(net)
    net.train()
    net.train_out_h = net.train_out_w = 32
    opt = optim.Adam(net.parameters(), net=net, lr=LR) if native else torch.optim.Adam(net.parameters(), lr=LR)
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    msk = (((yy - 32) ** 2 + (xx - 32) ** 2) < 19 ** 2)[None, None].cuda()
    tar = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
    init = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
    loss_log, grad_log = [], []
    for t in range(STEPS):
        np.random.seed(100 + t)
        torch.manual_seed(100 + t)
        opt.zero_grad(set_to_none=True)
        out = net.batch_render_pifu_nerf(net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=5, stride=0,
                                         tar_img=tar, bg_img=None, feat_geo=s["feat_geo"], feat_tex=s["feat_tex"], sp_data=dict(s["sp_data"]),
                                         camcenter=None, objcenter=None, msk=msk, src_foreground_mask=s["src_foreground_mask"],
                                         bounds=s["bounds"], fine=True, uniform=False, blur=3, sample_per_ray_c=16, sample_per_ray_f=16,
                                         rand_noise_std=0.01)
        out["tex_cal"], out["tex_cal_fine"] = out["tex_fg"], out["tex_fg_fine"]
        loss, _ = losses.compute_error(out_nerf=out, vggloss=None, lambdas=LAMBDAS)
        loss.backward()
        grad_log.append({n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()})
        opt.step()
        loss_log.append(float(loss.detach()))
    final = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
    return loss_log, init, final, grad_log, net._kpnerf_state, net


def test_five_training_steps_native_against_default():
    """Losses: the two loops start from the same parameters with the same draws; `plain` agrees to 2^-23, so every rendered value
    agrees within the parity bar 1e-4 and the loss, a (1 + 10)-weighted mean of absolute differences, within 11e-4 — at the first
    step and, the parameters staying as close as asserted below, at the later ones.
    Parameters, against the default loop: Adam's bias-corrected step is at most 1.01 lr per element in the first five steps
    (Cauchy-Schwarz on m and v), so two runs whose gradients differ in the last bits (the training backward adds with atomics) are
    at most 2 * 5 * 1.01 lr apart, the bound an element with a gradient near zero can reach.
    Parameters, the trajectory bar: torch.optim.Adam (fp32, CPU, foreach=False) and the fp64 formulas replay the gradients the
    native optimizer saw; the native parameters are at most twice as far from the fp64 result as torch's."""
    loss_n, init, final_n, grads_n, st, net = _loop(True)
    loss_d, init_d, final_d, _, _, _ = _loop(False)
    for n in init:
        assert torch.equal(init[n], init_d[n])
    for t, (a, b) in enumerate(zip(loss_n, loss_d)):
        print(f"step {t}: loss native {a:.6f}, default {b:.6f}")
        assert abs(a - b) <= 11e-4, (t, a, b)
    assert loss_n[0] > 0.1
    d_native = d_torch = 0.0
    for n in init:
        assert float((final_n[n] - init[n]).abs().max()) > 0.0, n                  # every tensor was stepped (steps of either sign may cancel)
        assert float((final_n[n] - final_d[n]).abs().max()) <= 2 * STEPS * 1.01 * LR + 2.0 ** -20 * float(final_d[n].abs().max()), n
        p64, m64, v64 = init[n].numpy().astype(np.float64), 0.0, 0.0
        pt = torch.nn.Parameter(init[n].clone())
        opt = torch.optim.Adam([pt], lr=LR, foreach=False)
        for t in range(STEPS):
            g = grads_n[t][n]
            p64, m64, v64, _ = pc.adam64(p64, g.numpy(), m64, v64, t + 1, lr=LR, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)
            pt.grad = g.clone()
            opt.step()
        d_native = max(d_native, float(np.abs(final_n[n].numpy().astype(np.float64) - p64).max()))
        d_torch = max(d_torch, float(np.abs(pt.detach().numpy().astype(np.float64) - p64).max()))
    print(f"5-step loop: max |native - fp64| = {d_native:.3e}, max |torch.optim.Adam - fp64| = {d_torch:.3e}")
    assert d_torch > 0.0 and d_native <= 2.0 * d_torch
    # the native step moved the version counters: the operands of the last render are stale and are built again, once
    stale = st.weights
    rebuilt = st.packed_weights()
    assert rebuilt is not stale and st.packed_weights() is rebuilt
    torch.cuda.synchronize()
