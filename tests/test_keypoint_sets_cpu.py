"""Keypoint sets on the wave64 emulator build (no GPU): models with 1..24 keypoints and 0..3 encoding octaves served as the
kernels' 24 / 3 model (include/kpnerf.h, "Keypoint sets").  The C entries against numpy scatters / gathers and against the existing
entries on widened tensors, bit for bit (tests/keypoint_set_cases.py); the live reference class built with another skeleton,
rendered and trained through install(); the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import keypoint_set_cases as kc
from tests import param_step_cases as pc
from tests import simt_harness as sh

needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference source tree (KPNERF_REFERENCE_ROOT)")
_IDS = [kc.case_id(c) for c in kc.CASES]


@pytest.fixture(scope="module")
def drv():
    return pc.Driver(sh.simt_lib(), to_dev=lambda a: np.array(a), ptr=sh.ptr, to_host=lambda a: a)


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------
def test_narrow_plain_sizes(drv):
    kc.check_sizes(drv)


@pytest.mark.parametrize("case", kc.CASES, ids=_IDS)
def test_widen_is_a_scatter_and_its_adjoint_a_gather(drv, case):
    kc.check_widen_and_narrow(drv, *case)


@pytest.mark.parametrize("case", kc.CASES, ids=_IDS)
def test_fold_with_a_load_map_equals_fold_of_the_widened_tensor(drv, case):
    kc.check_fold_shape(drv, *case)


def test_bad_shapes_are_refused_before_any_launch(drv):
    kc.check_bad_shapes(drv)


def _host_prepare():
    from keypointnerf_amd.synthetic import make_scene
    L = sh.simt_lib()
    scene = make_scene(n_views=3, src_hw=(64, 64), tar_hw=(16, 16), mask="ellipsoid", seed=5)
    hs = sh.HostScene(L, scene)
    kpt24 = hs.bufs["kpt3d"].copy()
    off = (ctypes.c_size_t * 6)()
    L.check(L.kpn_scene_layout(ctypes.byref(hs.desc), off))

    def prepare(kpt, n):
        kpt = np.ascontiguousarray(kpt, np.float32)
        hs.desc.kpt3d = kpt.ctypes.data
        ws = np.full(hs.ws.size, np.nan, np.float32)
        if n is None:
            assert kpt.shape == (24, 3)
            L.check(L.kpn_scene_prepare(ctypes.byref(hs.desc), sh.ptr(ws), None))
        else:
            assert kpt.shape == (n, 3)
            L.check(L.kpn_scene_prepare_kpt(ctypes.byref(hs.desc), n, sh.ptr(ws), None))
        hs.desc.kpt3d = hs.bufs["kpt3d"].ctypes.data
        return ws, list(off), hs.V
    return L, hs, prepare, kpt24


def test_scene_tables_repeat_keypoint_0_in_the_padded_rows():
    L, hs, prepare, kpt24 = _host_prepare()
    kc.check_scene_tables(prepare, kpt24)
    ws = np.full(hs.ws.size, np.nan, np.float32)
    for n in (0, 25, -3):
        assert L.kpn_scene_prepare_kpt(ctypes.byref(hs.desc), n, sh.ptr(ws), None) == -1 and b"n_kpt" in L.kpn_last_error()
    assert np.isnan(ws).all()                                          # nothing was launched


# ---- the Python layers over the emulator build ---------------------------------------------------------------------------------
_CPU_KERNELS = ("rgba2out", "rgba2out_backward", "importance_sample", "ray_bbox_intersection", "field_query", "render_rays",
                "render_rays_train", "render_rays_train_backward", "pix_l1_loss", "fold_params_norms", "fold_params_backward",
                "widen_plain", "narrow_plain_grad", "fold_params_norms_shape", "fold_params_backward_shape")


@pytest.fixture
def emulated(monkeypatch):
    """as tests/test_dropin_real_class_emulated.py: the unchanged ops / torch_ops / dropin / optim code over the emulator library"""
    from keypointnerf_amd import lib as kl, ops, torch_ops
    L = sh.simt_lib()
    monkeypatch.setattr(kl, "get_library", lambda: L)
    monkeypatch.setattr(ops, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    with torch.library._scoped_library("kpnerf", "FRAGMENT") as frag:
        for name in _CPU_KERNELS:
            frag.impl(name, getattr(torch_ops, name)._init_fn, "CPU")
        yield L


def _reference_net(n, lv, seed=0):
    """KeypointNeRF(cfg) of the reference with sp_args.n_kpt / sp_level edited (oracle.ref_shim.build_reference_net otherwise)"""
    from keypointnerf_amd.synthetic import perturb_reference_net
    rmodel = ref_shim.load_reference()
    cfg = ref_shim.load_config()
    cfg["models"]["KeypointNeRF"]["sp_args"]["n_kpt"] = n
    cfg["models"]["KeypointNeRF"]["sp_args"]["sp_level"] = lv
    torch.manual_seed(seed)
    net = rmodel.KeypointNeRF(cfg)
    net.eval()
    assert tuple(net.mlp_geo.layers1.layers[0].linear.weight_v.shape) == (128, kc.dim(n, lv) + 64)
    return perturb_reference_net(net, seed=7)


def _scene(n, tar=16, src=128):
    """the tiny scene of tests/test_dropin_real_class_emulated.py, its keypoints sliced to n rows"""
    from keypointnerf_amd.synthetic import make_scene
    s = make_scene(n_views=3, src_hw=(src, src), tar_hw=(tar, tar), mask="ellipsoid", seed=5, tar_focal_at_512=800.0, n_kpt=n)
    full = make_scene(n_views=3, src_hw=(src, src), tar_hw=(tar, tar), mask="ellipsoid", seed=5, tar_focal_at_512=800.0)
    assert torch.equal(s["sp_data"]["kpt3d"], full["sp_data"]["kpt3d"][:, :n]) and torch.equal(s["img"], full["img"])
    return s


def _close(got, ref, name, tol=1e-4, flips=0):
    """tests/test_dropin_real_class_emulated.py::_close"""
    d = (got - ref).abs().reshape(-1) if got.dim() < 3 else (got - ref).abs().reshape(-1, got.shape[-2] * got.shape[-1]).max(0)[0]
    assert int((d > tol).sum()) <= flips, (name, float(d.max()))


# ---- 2. the live reference class, rendered -------------------------------------------------------------------------------------
@needs_reference
@torch.no_grad()
@pytest.mark.parametrize("case", [(13, 3), (17, 2)], ids=kc.case_id)
def test_render_pifu_nerf_of_the_live_class_with_another_skeleton(emulated, case):
    from keypointnerf_amd.dropin import install, uninstall
    n, lv = case
    net, s = _reference_net(n, lv), _scene(n)
    kw = dict(net=net, img_in=s["img"], cam_in=s["cam"], cam_tar=s["cam_tar"], tar_img=None, sp_data=dict(s["sp_data"]),
              objcenter=torch.zeros(1, 3), fine=True, uniform=True, objrad=250., blur=3, level=1, sample_per_ray_c=12,
              sample_per_ray_f=8, src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"], mask_at_box=torch.ones(1, 16, 16))
    ref = net.render_pifu_nerf(**kw)
    install(net)                                                       # accepted
    got = net.render_pifu_nerf(**kw)
    uninstall(net)
    assert float(ref["alpha_fine"].max()) > 0.5 and float(ref["alpha_fine"].min()) < 0.05    # a subject and a background
    for k in ("tex_fg", "alpha", "depth", "tex_fg_fine", "alpha_fine", "depth_fine"):
        assert got[k].shape == ref[k].shape and got[k].device.type == "cpu", k
        print(f"{kc.case_id(case)} {k}: max |got - ref| = {float((got[k] - ref[k]).abs().max()):.3e} (bar 1e-4)")
        _close(got[k], ref[k], k)


# ---- 3. the live reference class, trained --------------------------------------------------------------------------------------
def _train_step(net, s):
    net.train()
    net.train_out_h = net.train_out_w = 6
    tar = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    msk = torch.zeros(1, 1, 16, 16)
    msk[..., 4:12, 4:12] = 1
    torch.manual_seed(21)
    np.random.seed(5)
    net.zero_grad(set_to_none=True)
    feat_geo = net.attach_geo_feat(s["img"], return_val=True)
    feat_tex = net.attach_tex_feat(s["img"], return_val=True)
    out = net.batch_render_pifu_nerf(
        net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=1, stride=0, tar_img=tar, bg_img=None,
        feat_geo=feat_geo, feat_tex=feat_tex, sp_data=dict(s["sp_data"]), camcenter=None, objcenter=None, msk=msk,
        src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"], fine=True, uniform=False, blur=3, rand_noise_std=0.01,
        sample_per_ray_c=8, sample_per_ray_f=8)
    loss = (out["tex_fg"] - out["tar_img"]).abs().mean() + 10.0 * (out["tex_fg_fine"] - out["tar_img"]).abs().mean() \
        + 0.1 * out["alpha_fine"].mean() + 0.01 * out["depth"].mean()
    loss.backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items() if v is not None}, float(loss), grads


def _check_step(got, ref):
    """the bars of tests/test_dropin_real_class_emulated.py::test_training_step_of_the_live_class_forward_and_gradients"""
    (got_out, got_loss, got_g), (ref_out, ref_loss, ref_g) = got, ref
    assert set(got_out) == set(ref_out)
    for k in ref_out:
        _close(got_out[k], ref_out[k], k)
    assert torch.equal(got_out["tar_img"], ref_out["tar_img"])        # same patch centre
    assert float(ref_out["alpha_fine"].max()) > 0.9 and float(ref_out["alpha_fine"].min()) < 0.1 and max(
        float(g.abs().max()) for g in ref_g.values()) > 1e-3          # the patch sees the subject; the gradients are not noise
    assert abs(got_loss - ref_loss) < 1e-5
    assert set(got_g) == set(ref_g)
    hot = [k for k in ref_g if k.startswith(("mlp_geo.", "mlp_tex.", "ibr_compress_gfeat."))]
    enc = [k for k in ref_g if k.startswith(("geo_encoder.", "tex_encoder."))]
    assert len(hot) >= 40 and len(enc) >= 20
    gmax = max(float(g.abs().max()) for g in ref_g.values())
    worst = 0.0
    for k in ref_g:
        assert got_g[k].shape == ref_g[k].shape, k
        scale = float(ref_g[k].abs().max())
        err = float((got_g[k] - ref_g[k]).abs().max())
        worst = max(worst, err / (2e-4 * scale + max(2e-7, 1e-6 * gmax)))
        assert err <= 2e-4 * scale + max(2e-7, 1e-6 * gmax), (k, scale, err)
    print(f"worst gradient error / bar = {worst:.3f}")


@needs_reference
def test_training_step_of_the_live_class_with_13_keypoints(emulated):
    """forward outputs and every gradient — the narrow weight_v / weight_g of layers1.0 among them — against the reference's own
    loss.backward()"""
    from keypointnerf_amd.dropin import install, uninstall
    net, s = _reference_net(13, 3), _scene(13)
    ref = _train_step(net, s)
    install(net)
    got = _train_step(net, s)
    uninstall(net)
    v = "mlp_geo.layers1.layers.0.linear.weight_v"
    assert tuple(got[2][v].shape) == (128, kc.dim(13, 3) + 64) and float(ref[2][v].abs().max()) > 0
    assert "mlp_geo.layers1.layers.0.linear.weight_g" in got[2]
    _check_step(got, ref)


@needs_reference
def test_native_parameter_step_of_the_live_class_with_13_keypoints(emulated):
    """install(net, native_params=True): the same step through kpn_fold_params_shape / _backward_shape, then one
    keypointnerf_amd.optim.Adam step against torch.optim.Adam on the reference.

    The bar of the parameters after the step.  Step 1 of Adam moves p by lr u(g), u(g) = g / (|g| + eps) (m-hat = g, v-hat = g^2).
    The two runs step from gradients that differ within the gradient bar above, so the updates differ by lr |u(g_got) - u(g_ref)|,
    evaluated here in fp64 from the two gradient sets; what remains is arithmetic: the rounding of p (2^-20 |p| as
    tests/test_param_step_cpu.py::_close_to_torch) and torch's fp32 evaluation of the update (3e-5 of the step, as there)."""
    from keypointnerf_amd import optim
    from keypointnerf_amd.dropin import install, uninstall
    lr, eps = 1e-3, 1e-8
    net, s = _reference_net(13, 3), _scene(13)
    twin = _reference_net(13, 3)                                       # (weight_norm modules do not deepcopy)
    twin.load_state_dict(net.state_dict())
    ref = _train_step(twin, s)
    torch.optim.Adam(twin.parameters(), lr=lr, eps=eps).step()
    install(net, native_params=True)
    got = _train_step(net, s)
    st = net._kpnerf_state
    assert st.native_params and st.shape == (13, 3) and tuple(st.native_tensors()[1].shape) == (128, kc.dim(13, 3) + 64)
    init = {k: p.detach().clone() for k, p in net.named_parameters()}
    optim.Adam(net.parameters(), net=net, lr=lr, eps=eps).step()
    uninstall(net)
    _check_step(got, ref)
    u = lambda g: g.double() / (g.double().abs() + eps)
    moved = 0
    for (k, p), q in zip(net.named_parameters(), twin.parameters()):
        if k not in ref[2]:
            continue
        bar = 2.0 ** -20 * q.detach().abs() + 3e-5 * lr + lr * (u(got[2][k]) - u(ref[2][k])).abs()
        assert ((p.detach() - q.detach()).abs().double() <= bar).all(), k
        moved += int(not torch.equal(p.detach(), init[k]))
    assert moved == len(ref[2])                                        # every parameter with a gradient was stepped


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
@needs_reference
def test_refusals_name_the_capacity_and_uninstall_restores_the_reference(emulated):
    from keypointnerf_amd.dropin import check_supported, install, uninstall
    net = _reference_net(13, 3)
    for attr, value, word in (("n_kpt", 25, "n_kpt in 1..24"), ("n_kpt", 0, "n_kpt in 1..24"), ("sp_level", 4, "sp_level in 0..3"),
                              ("sp_type", "rel_z", "rel_z_decay")):
        old = getattr(net.sp_encoder, attr)
        setattr(net.sp_encoder, attr, value)
        with pytest.raises(NotImplementedError, match=word) as e:
            install(net)
        if attr != "sp_type":
            assert "24 keypoints and 3 octaves" in str(e.value)           # the capacity
        assert "_kpnerf_state" not in net.__dict__
        setattr(net.sp_encoder, attr, old)
    net.sp_encoder.scale = 2.0
    with pytest.raises(NotImplementedError, match="scale"):
        check_supported(net)
    net.sp_encoder.scale = 1.0
    # a kpt3d whose row count is not the model's n_kpt: the reference asserts (src/spatial.py:80), the drop-in raises
    s = _scene(13)
    s24 = _scene(24)
    kw = dict(net=net, img_in=s["img"], cam_in=s["cam"], cam_tar=s["cam_tar"], tar_img=None, objcenter=torch.zeros(1, 3), fine=True,
              uniform=True, objrad=250., blur=3, level=1, sample_per_ray_c=4, sample_per_ray_f=4,
              src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"], mask_at_box=torch.ones(1, 16, 16))
    install(net)
    with torch.no_grad():
        for bad in (s24["sp_data"], {"kpt3d": s["sp_data"]["kpt3d"][:, :12].contiguous(), "extrin": s["sp_data"]["extrin"]}):
            with pytest.raises(ValueError, match="n_kpt is 13"):
                net.render_pifu_nerf(sp_data=dict(bad), **kw)
    uninstall(net)
    cls = type(net)
    for k in ("batch_render_pifu_nerf", "render_pifu_nerf", "query", "rgba2out", "importance_sample", "ray_bbox_intersection",
              "attach_geo_feat", "attach_tex_feat"):
        assert k not in net.__dict__, k
        f = getattr(net, k)
        assert getattr(f, "__func__", f) is getattr(cls.__dict__[k], "__func__", cls.__dict__[k]), k
    with torch.no_grad(), pytest.raises(AssertionError):               # the reference's own assert is back
        net.render_pifu_nerf(sp_data=dict(s24["sp_data"]), **kw)


def test_prepared_scene_and_weights_refuse_what_does_not_fit(emulated):
    """without the reference: ops.PreparedScene takes (1, n, 3) up to 24 rows and refuses more; weights of a narrow model are refused
    as the shipped shape and accepted with theirs"""
    from keypointnerf_amd import ops, weights
    from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict
    s = make_scene(n_views=2, src_hw=(64, 64), tar_hw=(8, 8), seed=2, n_kpt=13)
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    assert ps.n_kpt == 13
    for rows in (25, 0):
        bad = dict(s["sp_data"], kpt3d=torch.zeros(1, rows, 3))
        with pytest.raises(ValueError, match="1..24"):
            ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], bad, s["src_foreground_mask"])
    with pytest.raises(ValueError):
        make_scene(n_kpt=25)
    sd = random_hotpath_state_dict(seed=1, n_kpt=13, sp_level=2)
    assert tuple(sd["mlp_geo.layers1.layers.0.linear.weight_v"].shape) == (128, 13 * 5 + 64)
    with pytest.raises(ValueError, match="unsupported architecture"):
        weights.effective_weights(sd)
    narrow = weights.flatten_plain(weights.effective_weights(sd, (13, 2)))
    assert narrow.size == kc.narrow_floats(13, 2)
    assert weights.widen_plain_host(narrow, (13, 2)).tobytes() == kc.widen_np(narrow, 13, 2).tobytes()
    assert np.array_equal(weights.canonical_columns((13, 2)), kc.canonical_cols(13, 2))
    # the defaults are today's values, bit for bit
    a, b = random_hotpath_state_dict(seed=1), random_hotpath_state_dict(seed=1, n_kpt=24, sp_level=3)
    assert all(torch.equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


# ---- the reference fixtures of the GPU suite, on the emulator: the same checks, so that they also run where the fixtures are made
# (one tile and one training step; the GPU suite runs every combination)
def test_fixture_tile_through_the_c_abi(emulated):
    kc.check_golden_render_abi((13, 3), "cpu", "f16x2")


def test_fixture_training_step_through_the_dropin(emulated):
    kc.check_golden_train((17, 2), "cpu", native_params=True)
