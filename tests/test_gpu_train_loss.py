"""kpn_train_loss on the device, through the C ABI: the checks of tests/test_train_loss_cpu.py (fp64 formulas, exact cases, L1 bit
identity with kpn_pix_l1_loss, re-run on a workspace the kernel has left ready) and the drop-in training step end to end with
every lambda switched on — the fused operator against today's per-term path on the same draws."""
import ctypes

import numpy as np
import pytest
import torch

from tests import train_loss_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drv():
    from keypointnerf_amd import lib as kl

    def to_host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return tc.Driver(kl.get_library(), to_dev=lambda a: torch.from_numpy(np.array(a)).cuda(), ptr=lambda t: ctypes.c_void_p(t.data_ptr()),
                     to_host=to_host, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("n", tc.SHAPES)
def test_values_and_gradients_against_fp64(drv, n):
    tc.check_values_and_gradients(drv, n)


@pytest.mark.parametrize("n", tc.SHAPES)
def test_l1_terms_bit_identical_to_pix_l1_loss_and_rerun_without_reset(drv, n):
    tc.check_l1_bit_identical_and_rerun(drv, n)


def test_exact_cases(drv):
    tc.check_ties(drv)
    tc.check_clamp_band(drv)
    tc.check_skipped_terms_leave_their_buffers(drv)


def test_operator_reuses_its_workspace_and_is_graph_capture_clean():
    """ops.train_loss keeps one workspace per stream and zeroes its ticket once (later calls are a single launch); under graph
    capture it takes a workspace of the capture's own.  Eager, repeated and replayed results are the same bits."""
    from keypointnerf_amd import ops
    inp = tc.inputs(4096)
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in inp.items()}
    call = lambda: ops.train_loss(t["tex"], t["tex_fine"], t["tar"], t["alpha"], t["alpha_fine"], t["tar_alpha"], tc.WEIGHTS)
    first = [v.clone() for v in call()]
    key = (t["tar"].device, torch.cuda.current_stream().cuda_stream)
    ws = ops._TRAIN_LOSS_WS[key]
    again = call()
    assert ops._TRAIN_LOSS_WS[key] is ws
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):                                                 # as tests/test_gpu_parity.py captures a frame
        call()                                                                    # warm-up on the capture's stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = call()
    for _ in range(2):
        for v in captured:
            v.fill_(-1.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert torch.equal(a, b)


def _carrier(scene):
    from tests.test_gpu_dropin import _net
    return _net(scene)


def test_training_step_with_every_lambda_on_fused_against_per_term(monkeypatch):
    """The drop-in training step on the fixture scene of tests/test_gpu_dropin.py (case k) with l1_c, l1, l2, lp and mloss > 0:
    loss.backward() through torch.ops.kpnerf.train_loss against the same step through today's per-term path, same draws.
    Seed gradients (d_tex_fg, d_tex_fg_fine, d_alpha, d_alpha_fine): the bar of tests/train_loss_cases.py against the fp64
    formulas, the eager error being the per-term path's own.  Parameter gradients: the bar test_training_step_through_the_dropin
    applies between the library's and the reference's evaluation order, 1e-4 of the layer's largest gradient + 1e-7."""
    from keypointnerf_amd import losses
    from keypointnerf_amd.synthetic import HOTPATH_LAYERS
    from tests.golden_io import load_case
    scene, cfg, g = load_case("case_k_v3_train_grad")
    net, s = _carrier(scene)
    V, Sc, Sf = cfg["n_views"], cfg["Sc"], cfg["Sf"]
    patch = int(round(g["pix"].shape[0] ** 0.5))
    Ht, Wt = s["cam_tar"]["height"], s["cam_tar"]["width"]
    yy, xx = torch.meshgrid(torch.arange(Ht), torch.arange(Wt), indexing="ij")
    msk = (((yy - Ht / 2) ** 2 + (xx - Wt / 2) ** 2) < (0.3 * min(Ht, Wt)) ** 2)[None, None].cuda()
    tar = torch.rand(1, 3, Ht, Wt, generator=torch.Generator().manual_seed(4)).cuda()
    lambdas = {"lambda_l1_c": 1.0, "lambda_l1": 10.0, "lambda_l2": 3.0, "lambda_lp": 0.5, "lambda_mloss": 4.0}
    net.train()
    net.train_out_h = net.train_out_w = patch
    seeds_of = ("tex_fg", "tex_fg_fine", "alpha", "alpha_fine")

    def step(fused):
        net.zero_grad(set_to_none=True)
        np.random.seed(6)
        torch.manual_seed(6)
        out = net.batch_render_pifu_nerf(net=net, img_in=s["img"], cam_in=s["cam"], n_views=V, cam_tar=s["cam_tar"], level=5, stride=0,
                                         tar_img=tar, bg_img=None, feat_geo=s["feat_geo"], feat_tex=s["feat_tex"], sp_data=dict(s["sp_data"]),
                                         camcenter=None, objcenter=None, msk=msk, src_foreground_mask=s["src_foreground_mask"],
                                         bounds=s["bounds"], fine=True, uniform=False, blur=3, sample_per_ray_c=Sc,
                                         sample_per_ray_f=Sf, rand_noise_std=float(g["noise_std"]))
        for k in seeds_of:
            out[k].retain_grad()
        out["tex_cal"], out["tex_cal_fine"] = out["tex_fg"], out["tex_fg_fine"]
        assert losses._fusable(out)
        with monkeypatch.context() as m:
            if not fused:
                m.setattr(losses, "_fusable", lambda o: False)
            loss, err = losses.compute_error(out_nerf=out, vggloss=None, lambdas=lambdas)
        loss.backward()
        return (float(loss), list(err), {k: out[k].detach().clone() for k in seeds_of + ("tar_img", "tar_alpha")},
                {k: out[k].grad.clone() for k in seeds_of}, {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})

    loss_f, keys_f, outs_f, seeds_f, params_f = step(True)
    loss_e, keys_e, outs_e, seeds_e, params_e = step(False)
    assert keys_f == keys_e == ["e_pix_c", "e_pix_l1", "e_pix_l2", "e_pix_lp", "mask_loss_c", "mask_loss_f", "e_all"]
    for k in outs_f:
        assert torch.equal(outs_f[k], outs_e[k]), k                              # same draws, same forward
    # seed gradients against the fp64 formulas
    flat = lambda k: outs_f[k].reshape(-1).cpu().numpy()
    inp = {"tex": flat("tex_fg"), "tex_fine": flat("tex_fg_fine"), "tar": flat("tar_img"), "alpha": flat("alpha"), "alpha_fine": flat("alpha_fine"),
           "tar_alpha": flat("tar_alpha")}
    ref_t, ref_g = tc.formulas(inp, tuple(lambdas.values()), torch.float64)
    refs = {"tex_fg": ref_g["d_tex"], "tex_fg_fine": sum(ref_g["d_tex_fine"]), "alpha": ref_g["d_alpha"], "alpha_fine": ref_g["d_alpha_fine"]}
    for k in seeds_of:
        b, e = tc.bar(seeds_e[k].reshape(-1).cpu().numpy(), refs[k])
        err = float(np.abs(seeds_f[k].reshape(-1).cpu().numpy().astype(np.float64) - refs[k]).max())
        print(f"seed gradient {k}: |fused - fp64| = {err:.3e}, per-term eager = {e:.3e}, bar = {b:.3e}")
        assert err <= b, (k, err, e, b)
    b, e = tc.bar(loss_e, np.array([ref_t.sum()]))
    print(f"loss: |fused - fp64| = {abs(loss_f - ref_t.sum()):.3e}, per-term eager = {e:.3e}, bar = {b:.3e}")
    assert abs(loss_f - ref_t.sum()) <= b
    # parameter gradients
    checked = 0
    for lname, prefix, shape, wn in HOTPATH_LAYERS:
        names = [n for n in params_e if n.startswith(prefix + ".")]
        scale = max(float(params_e[n].abs().max()) for n in names)
        for n in names:
            err = float((params_f[n] - params_e[n]).abs().max())
            assert err <= 1e-4 * scale + 1e-7, (n, err, scale)
            checked += 1
    assert checked >= 40
