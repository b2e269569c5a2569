"""The parameter step (csrc/param_kernels.hip: kpn_fold_params, kpn_fold_params_backward, kpn_adam_step) on the wave64 emulator
build: the kernels against their fp64 restatements (cases and bars: tests/param_step_cases.py), torch.ops.kpnerf.fold_params and
its autograd against weights.plain_tensor_from_module, keypointnerf_amd.optim.Adam's interface, and the drop-in's training step
with native_params=True against the default path.  tests/test_gpu_param_step.py repeats the kernel checks on the device."""
import copy

import numpy as np
import pytest
import torch

from tests import param_step_cases as pc
from tests import simt_harness as sh


@pytest.fixture(scope="module")
def drv():
    return pc.Driver(sh.simt_lib(), to_dev=lambda a: np.array(a), ptr=sh.ptr, to_host=lambda a: a)


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


# ---- the Python layers, served by the emulator build on CPU tensors ------------------------------------------------------------
_CPU_KERNELS = ("rgba2out", "rgba2out_backward", "importance_sample", "ray_bbox_intersection", "field_query", "render_rays",
                "render_rays_train", "render_rays_train_backward", "pix_l1_loss", "fold_params_norms", "fold_params_backward")


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


class _Carrier(torch.nn.Module):
    """the hot-path parameters under the reference's names, plus an encoder that is not on the hot path"""

    def __init__(self, sd, new_style=False):
        super().__init__()
        for k, v in sd.items():
            if new_style:
                k = k.replace(".weight_g", ".parametrizations.weight.original0").replace(".weight_v", ".parametrizations.weight.original1")
            mod, parts = self, k.split(".")
            for p in parts[:-1]:
                if not hasattr(mod, p):
                    setattr(mod, p, torch.nn.Module())
                mod = getattr(mod, p)
            mod.register_parameter(parts[-1], torch.nn.Parameter(v.clone()))
        self.geo_encoder = torch.nn.Linear(5, 3)


def _spread_state_dict():
    """a state dict holding tests/param_step_cases.inputs(): rows spread over 2^-12 .. 2^12, g of both signs"""
    from keypointnerf_amd.weights import hot_tensor_names
    from keypointnerf_amd.synthetic import random_hotpath_state_dict
    sd = random_hotpath_state_dict(seed=1)
    tensors, _ = pc.inputs()
    for name, x in zip(hot_tensor_names(sd), tensors):
        sd[name] = torch.from_numpy(np.array(x)).reshape(sd[name].shape)
    return sd


@pytest.mark.parametrize("new_style", [False, True])
@pytest.mark.parametrize("through", ["operator", "plain_tensor_native"])
def test_operator_and_its_autograd_against_plain_tensor_from_module(emulated, new_style, through, monkeypatch):
    """torch.ops.kpnerf.fold_params (the registered operator and its autograd formula) called directly and through
    weights.plain_tensor_native on a live module, either weight-norm spelling: the value within 2^-23 of the fp64 fold plus torch's own
    distance from it, and loss.backward() through it against loss.backward() through plain_tensor_from_module — each within the
    kernel's bar of the fp64 gradient plus the eager path's own distance from it."""
    from keypointnerf_amd import weights
    if through == "operator":
        monkeypatch.setattr(weights, "plain_tensor_native", lambda net: torch.ops.kpnerf.fold_params(weights.hot_tensors(net)))
    net = _Carrier(_spread_state_dict(), new_style)
    tensors, d_plain = pc.inputs()
    upstream = torch.from_numpy(np.array(d_plain))
    eager = weights.plain_tensor_from_module(net)
    native = weights.plain_tensor_native(net)
    assert native.requires_grad and native.shape == eager.shape
    ref, is_copy = pc.fold64(tensors)
    err = np.abs(native.detach().numpy().astype(np.float64) - eager.detach().numpy().astype(np.float64))
    assert (err <= np.where(is_copy, 0.0, 2.0 ** -23 * np.abs(ref)) + np.abs(eager.detach().numpy().astype(np.float64) - ref)).all()
    (eager * upstream).sum().backward()
    g_eager = [p.grad.clone() for p in weights.hot_tensors(net)]
    net.zero_grad(set_to_none=True)
    (native * upstream).sum().backward()
    g_native = [p.grad for p in weights.hot_tensors(net)]
    assert net.geo_encoder.weight.grad is None
    for (field, l, shape), a, b, (r, scale) in zip(pc.slots(), g_native, g_eager, pc.backward64(tensors, d_plain)):
        a, b, r = (np.asarray(x, np.float64).reshape(shape) for x in (a.numpy(), b.numpy(), r))
        if scale is None:
            assert np.array_equal(a, b), (field, l)
            continue
        bar = (2.0 ** -23 if field == "g" else 2.0 ** -22) * scale.reshape(shape)
        assert (np.abs(a - b) <= bar + np.abs(b - r)).all(), (field, l)


def test_native_gradients_accumulate_like_any_other(emulated):
    """two backward passes without zero_grad: .grad holds the sum (autograd's accumulation over the operator's outputs), and
    ops.fold_params_backward(accumulate=True) adds into given destinations"""
    from keypointnerf_amd import ops, weights
    from keypointnerf_amd.synthetic import random_hotpath_state_dict
    net = _Carrier(random_hotpath_state_dict(seed=2))
    w = torch.randn(pc.N_PLAIN, generator=torch.Generator().manual_seed(0))
    (weights.plain_tensor_native(net) * w).sum().backward()
    once = [p.grad.clone() for p in weights.hot_tensors(net)]
    (weights.plain_tensor_native(net) * w).sum().backward()
    for p, g in zip(weights.hot_tensors(net), once):
        assert torch.equal(p.grad, g + g)
    tensors = weights.hot_tensors(net)
    plain, norms = ops.fold_params(tensors)
    dst = [g.clone() for g in once]
    ops.fold_params_backward(tensors, norms, w, out=dst, accumulate=True)
    for d, g in zip(dst, once):
        assert torch.equal(d, g + g)


def _adam_pair(emulated, **kw):
    """the same module twice: one under keypointnerf_amd.optim.Adam, one under torch.optim.Adam"""
    from keypointnerf_amd import optim
    from keypointnerf_amd.synthetic import random_hotpath_state_dict
    a = _Carrier(random_hotpath_state_dict(seed=4))
    b = copy.deepcopy(a)
    return a, optim.Adam(a.parameters(), net=a, **kw), b, torch.optim.Adam(b.parameters(), **kw)


def _set_grads(net, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for n, p in net.named_parameters():
        p.grad = None if n in skip else torch.randn(p.shape, generator=g) * 0.1


def _close_to_torch(p, q, path):
    """A hot parameter under the native step against the same parameter under torch.optim.Adam; `path` = the distance torch's
    parameter travelled, summed over the steps taken.  Both evaluate the same formulas: they differ by the roundings of p (2^-24
    |p| per step and implementation: 2^-20 |p| covers the steps of this test) and by torch's fp32 evaluation of the update — a
    dozen roundings, below 1e-6 of a step — so 3e-5 of the path is wide for arithmetic and narrow for a mis-plumbed lr, beta,
    eps or weight_decay (wd = 0.01 moves these updates by parts in a thousand)."""
    return bool(((p - q).abs() <= 2.0 ** -20 * q.abs() + 3e-5 * path).all())


def test_optimizer_steps_like_torch_and_round_trips_its_state_dict(emulated):
    a, opt_a, b, opt_b = _adam_pair(emulated, lr=1e-3, weight_decay=0.01)
    init = {n: p.detach().clone() for n, p in a.named_parameters()}
    path = {n: torch.zeros_like(p) for n, p in init.items()}

    def step_both(na, oa, nb, ob):
        before = {n: p.detach().clone() for n, p in nb.named_parameters()}
        oa.step()
        ob.step()
        for n, p in nb.named_parameters():
            path[n] += (p.detach() - before[n]).abs()

    skip = ("mlp_tex.ani_al", "geo_encoder.bias")
    assert opt_a.state_dict()["state"] == {}                          # as torch: no state before the first step
    for t in range(3):
        _set_grads(a, t, skip)
        _set_grads(b, t, skip)
        versions = {n: p._version for n, p in a.named_parameters()}
        step_both(a, opt_a, b, opt_b)
        assert all((p._version > versions[n]) == (n not in skip) for n, p in a.named_parameters())   # packed operands key on this
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    for n in pa:
        if n in skip:                                                  # grad None: untouched, no state, step not advanced
            assert pa[n] not in opt_a.state and torch.equal(pa[n], init[n]), n
        elif n.startswith("geo_encoder."):
            assert torch.equal(pa[n], pb[n]) and not torch.equal(pa[n], init[n]), n      # not on the hot path: exactly torch's result
        else:
            assert float(path[n].min()) > 0 and _close_to_torch(pa[n].detach(), pb[n].detach(), path[n]), n
    # the moments of the hot parameters are views of two flat buffers; the step count is a host tensor
    hot = [p for n, p in pa.items() if not n.startswith("geo_encoder.") and n not in skip]
    assert len(hot) == 43
    assert len({opt_a.state[p]["exp_avg"].untyped_storage().data_ptr() for p in hot}) == 1
    assert len({opt_a.state[p]["exp_avg_sq"].untyped_storage().data_ptr() for p in hot}) == 1
    assert all(float(opt_a.state[p]["step"]) == 3.0 and opt_a.state[p]["step"].device.type == "cpu" for p in hot)
    # state_dict: torch.optim.Adam's layout, loadable both ways; one more step from the loaded state agrees as before
    sa, sb = opt_a.state_dict(), opt_b.state_dict()
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys() and sa["state"].keys() == sb["state"].keys()
    for k in sb["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"])
        assert sa["state"][k]["exp_avg"].shape == sb["state"][k]["exp_avg"].shape
    a2, opt_a2, b2, opt_b2 = _adam_pair(emulated, lr=1e-3, weight_decay=0.01)
    a2.load_state_dict(b.state_dict())
    b2.load_state_dict(a.state_dict())
    opt_a2.load_state_dict(copy.deepcopy(sb))                          # torch's state into ours
    opt_b2.load_state_dict(copy.deepcopy(sa))                          # ours into torch's
    hot2 = [p for n, p in a2.named_parameters() if not n.startswith("geo_encoder.") and n not in skip]
    assert len({opt_a2.state[p]["exp_avg"].untyped_storage().data_ptr() for p in hot2}) == 1
    for (n, p), q in zip(a2.named_parameters(), b.parameters()):
        if n not in skip:
            assert torch.equal(opt_a2.state[p]["exp_avg_sq"], opt_b.state[q]["exp_avg_sq"]), n
    _set_grads(a2, 9, skip)
    _set_grads(b2, 9, skip)
    step_both(a2, opt_a2, b2, opt_b2)
    for (n, p), q in zip(a2.named_parameters(), b2.parameters()):
        if n in skip:
            continue
        # the two started this step from each other's end of the first three: twice the bar
        assert _close_to_torch(p.detach(), q.detach(), 2 * path[n]) or n.startswith("geo_encoder."), n
        assert float(opt_a2.state[p]["step"]) == float(opt_b2.state[q]["step"]) == 4.0


def test_refused_options_raise(emulated):
    from keypointnerf_amd import optim
    net = _Carrier({"mlp_tex.ani_al": torch.tensor(0.2)})
    for kw in ({"amsgrad": True}, {"maximize": True}):
        with pytest.raises(NotImplementedError):
            optim.Adam(net.parameters(), net=net, **kw)
    with pytest.raises(ValueError):
        optim.Adam(net.parameters(), lr=1e-3)                          # no net


def test_hot_parameters_have_no_cpu_path():
    """without the emulation above the optimizer refuses hot-path parameters that are not on the GPU: no eager fall-back"""
    from keypointnerf_amd import optim
    net = _Carrier({"mlp_tex.ani_al": torch.tensor(0.2)})
    opt = optim.Adam(net.parameters(), net=net)
    _set_grads(net, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()


def _training_step(native):
    """one drop-in training step on a small scene (the stand-in carrier of tests/test_gpu_dropin.py on CPU tensors)"""
    from keypointnerf_amd.dropin import install, uninstall
    from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict
    from tests.test_gpu_dropin import StandInNet
    s = make_scene(n_views=3, src_hw=(128, 128), tar_hw=(16, 16), mask="ellipsoid", seed=5, tar_focal_at_512=800.0)
    net = StandInNet(random_hotpath_state_dict(seed=3), s)
    install(net, native_params=True) if native else install(net)
    net.train()
    net.train_out_h = net.train_out_w = 6
    msk = torch.zeros(1, 1, 16, 16)
    msk[..., 4:12, 4:12] = 1
    torch.manual_seed(21)
    np.random.seed(5)
    out = net.batch_render_pifu_nerf(
        net=net, img_in=s["img"], cam_in=s["cam"], n_views=3, cam_tar=s["cam_tar"], level=1, stride=0, tar_img=torch.rand(1, 3, 16, 16),
        bg_img=None, feat_geo=s["feat_geo"], feat_tex=s["feat_tex"], sp_data=dict(s["sp_data"]), camcenter=None, objcenter=None, msk=msk,
        src_foreground_mask=s["src_foreground_mask"], bounds=s["bounds"], fine=True, uniform=False, blur=3, rand_noise_std=0.01,
        sample_per_ray_c=8, sample_per_ray_f=8)
    loss = (out["tex_fg"] - out["tar_img"]).abs().mean() + 10.0 * (out["tex_fg_fine"] - out["tar_img"]).abs().mean() + 0.1 * out["alpha_fine"].mean()
    loss.backward()
    grads = {n: p.grad.clone() for n, p in net.named_parameters()}
    st = net._kpnerf_state
    uninstall(net)
    return {k: v.detach() for k, v in out.items() if v is not None}, grads, st


def test_dropin_training_step_native_against_default(emulated):
    """install(net, native_params=True): out_nerf of one training step equals the default path's — `plain` agrees to the fold
    bar 2^-23, the rendered patch within the parity bar 1e-4 — the parameter gradients agree, and the operands are packed once:
    by the drop-in for this parameter version, not again inside render_rays_train.  install(net) without the keyword is the
    parent's path: no native fold, one pack inside render_rays_train, outputs byte-identical from run to run (the gradients of
    either path come from the training backward's atomic adds and are not compared bit for bit)."""
    from keypointnerf_amd import ops, torch_ops
    packs, folds = [], []
    real_pack, real_fold = ops.PackedWeights.from_plain.__func__, ops.fold_params
    with pytest.MonkeyPatch.context() as m:
        m.setattr(ops.PackedWeights, "from_plain", classmethod(lambda cls, *a, **k: (packs.append(1), real_pack(cls, *a, **k))[1]))
        m.setattr(ops, "fold_params", lambda *a, **k: (folds.append(1), real_fold(*a, **k))[1])
        out_d, g_d, _ = _training_step(False)
        assert len(folds) == 0 and len(packs) == 1
        out_d2, _, st_d = _training_step(False)
        out_n, g_n, st = _training_step(True)
        assert len(folds) == 1 and len(packs) == 3                     # one fold, ONE pack for the native step
    assert st.native_params and st.weights is not None and torch_ops._IterCache.seed is None
    assert not st_d.native_params and st_d.weights is None
    for k in out_d:
        assert torch.equal(out_d[k], out_d2[k]), k
        assert out_n[k].shape == out_d[k].shape and float((out_n[k] - out_d[k]).abs().max()) <= 1e-4, k
    assert float(out_d["alpha_fine"].max()) > 0.5                      # the patch sees the subject
    gmax = max(float(g.abs().max()) for g in g_d.values())
    assert gmax > 1e-3
    for n in g_d:
        scale = float(g_d[n].abs().max())
        assert float((g_n[n] - g_d[n]).abs().max()) <= 2e-4 * scale + max(2e-7, 1e-6 * gmax), n


def test_native_plain_of_the_dropin_agrees_to_the_fold_bar(emulated):
    from keypointnerf_amd import weights
    from keypointnerf_amd.synthetic import random_hotpath_state_dict
    net = _Carrier(random_hotpath_state_dict(seed=3))
    with torch.no_grad():
        a, b = weights.plain_tensor_native(net).double(), weights.plain_tensor_from_module(net).double()
    ref, is_copy = pc.fold64([p.detach().numpy() for p in weights.hot_tensors(net)])
    assert (np.abs(a.numpy() - ref) <= 2.0 ** -23 * np.abs(ref)).all() and np.array_equal(a.numpy()[is_copy], b.numpy()[is_copy])


def test_packed_weights_folds_only_for_a_new_parameter_version(emulated, monkeypatch):
    """_State.packed_weights() with native_params=True: a second call for the same parameter version launches nothing (no fold,
    no pack); an in-place change of one tensor makes it fold and pack once more"""
    from keypointnerf_amd import dropin, ops
    from keypointnerf_amd.synthetic import random_hotpath_state_dict
    net = _Carrier(random_hotpath_state_dict(seed=3))
    calls = {"fold": 0, "pack": 0}
    real_fold, real_pack = ops.fold_params, ops.PackedWeights.from_plain.__func__
    monkeypatch.setattr(ops, "fold_params", lambda *a, **k: (calls.__setitem__("fold", calls["fold"] + 1), real_fold(*a, **k))[1])
    monkeypatch.setattr(ops.PackedWeights, "from_plain",
                        classmethod(lambda cls, *a, **k: (calls.__setitem__("pack", calls["pack"] + 1), real_pack(cls, *a, **k))[1]))
    st = dropin._State(net, native_params=True)
    w = st.packed_weights()
    assert st.packed_weights() is w and calls == {"fold": 1, "pack": 1}
    with torch.no_grad():
        net.mlp_tex.ani_al.mul_(2.0)
    assert st.packed_weights() is not w and calls == {"fold": 2, "pack": 2}
