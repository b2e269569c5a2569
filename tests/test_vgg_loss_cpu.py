"""The native VGG perceptual term (kpn_vgg_loss, csrc/vgg_kernels.hip; reference VGGLoss, src/utils.py:750-805) on the host
emulator build of the kernel sources (tests/simt): the three parity rules on the recorded reference golden, the exact
properties (equal inputs give exact zeros, position independence, loss-only = same bits, reproducibility, linearity), and
the Python layer (keypointnerf_amd.vgg: refusals, fall-back to the module's own forward, install on the live class)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import simt_harness as sh
from tests import vgg_golden as vg
from tests.golden_io import GOLDEN_DIR

GOLDEN = os.path.join(GOLDEN_DIR, "case_v_vgg_loss.npz")


@pytest.fixture(scope="module")
def emu():
    L = sh.simt_lib()
    g = np.load(GOLDEN)
    feats = vg.features(int(g["seed"]))
    vg.check_checksums(feats, g["checksums"])
    plain = vg.plain(feats).numpy()
    assert plain.size == L.kpn_vgg_plain_floats()
    packed = np.zeros(L.kpn_vgg_packed_floats(), np.float32)
    L.check(L.kpn_vgg_pack_device(sh.ptr(plain), sh.ptr(packed), None))
    return L, packed, vg.conv_params(feats), g


def run(emu, x, y, lam=1.0, tap_w=vg.TAP_W, grad=True, stages=False):
    L, packed = emu[0], emu[1]
    x, y = sh.f32(x), sh.f32(y)
    B, _, H, W = x.shape
    nb = L.kpn_vgg_workspace_bytes(B, H, W)
    ws = np.zeros(nb // 4, np.float32)
    loss = np.full(1, np.nan, np.float32)
    dx = np.full_like(x, np.nan) if grad else None
    st = np.full(L.kpn_vgg_stage_floats(B, H, W), np.nan, np.float32) if stages else None
    consts = [np.array(v, np.float32) for v in (vg.MEAN, vg.STD, tap_w)]
    L.check(L.kpn_vgg_loss(sh.ptr(x), sh.ptr(y), B, H, W, sh.ptr(packed), *[sh.ptr(c) for c in consts], lam, sh.ptr(loss),
                           sh.ptr(dx), sh.ptr(st), sh.ptr(ws), nb, None))
    return loss[0], dx, st


@pytest.mark.parametrize("case", ["c32", "c19x27", "half32"])
def test_parity_rules_on_the_reference_golden(emu, case):
    g, params = emu[3], emu[2]
    x, y = g[f"{case}_x"], g[f"{case}_y"]
    B, _, H, W = x.shape
    loss, dx, st = run(emu, x, y, stages=True)
    S = vg.stages_nchw(st, B, H, W)
    # rule 1: stage-wise forward, and the loss from the library's own stages
    worst, l_own = vg.rule1(x, y, S, params, B)
    assert worst <= 1.0, worst
    assert abs(float(loss) - l_own) <= 1e-6 * abs(l_own)
    # rule 2: decision-matched backward
    dm = vg.decision_matched_backward(S, params, B).numpy()
    assert np.linalg.norm(dx - dm) <= 1e-5 * np.linalg.norm(dm)
    assert np.abs(dx - dm).max() <= 1e-4 * np.abs(dm).max()
    # rule 3: end to end against the reference's fp64 result
    e_loss, cos, e_loss32, cos32 = vg.end_to_end(loss, dx, g, case)
    n_diff, n_out = vg.differing_decisions(S, *vg.reference64(x, y, params), B)
    print(f"{case}: loss rel err {e_loss:.2e} (reference fp32: {e_loss32:.2e}), d_x cosine {cos:.9f} (reference fp32: "
          f"{cos32:.9f}), differing decisions {n_diff}, outside the rule-1 margin {n_out}")
    assert e_loss <= 1e-5 and cos >= 0.9999 and n_out == 0


def test_equal_inputs_give_exact_zeros(emu):
    x = np.random.default_rng(3).random((1, 3, 9, 12), dtype=np.float32)
    loss, dx, _ = run(emu, x, x.copy())
    assert loss == 0.0 and np.all(dx == 0.0)


def test_position_independence_and_reproducibility(emu):
    rng = np.random.default_rng(4)
    a, b = rng.random((1, 3, 10, 8), dtype=np.float32), rng.random((1, 3, 10, 8), dtype=np.float32)
    x, y = np.concatenate([a, a]), np.concatenate([b, b])
    loss, dx, st = run(emu, x, y, stages=True)
    assert np.array_equal(dx[0], dx[1])
    S = vg.stages_nchw(st, 2, 10, 8)
    assert all(torch.equal(s[0], s[1]) and torch.equal(s[2], s[3]) for s in S)
    loss2, dx2, st2 = run(emu, x, y, stages=True)
    assert loss2.tobytes() == loss.tobytes() and np.array_equal(dx2, dx) and np.array_equal(st2, st)
    loss_only, none, _ = run(emu, x, y, grad=False)
    assert none is None and loss_only.tobytes() == loss.tobytes()


def test_lambda_and_tap_weights_act_linearly(emu):
    rng = np.random.default_rng(5)
    x, y = rng.random((1, 3, 8, 8), dtype=np.float32), rng.random((1, 3, 8, 8), dtype=np.float32)
    loss, dx, st = run(emu, x, y, stages=True)
    loss2, dx2, _ = run(emu, x, y, lam=2.0)
    assert loss2 == 2 * loss and np.array_equal(dx2, 2 * dx)
    S = vg.stages_nchw(st, 1, 8, 8)
    l4, dx4, _ = run(emu, x, y, tap_w=(0.0, 0.0, 0.0, 1.0))
    ref4 = float((S[8][:1] - S[8][1:]).abs().mean())
    assert abs(float(l4) - ref4) <= 1e-6 * ref4
    parts = [run(emu, x, y, tap_w=tuple(float(i == t) * vg.TAP_W[t] for i in range(4))) for t in range(4)]
    assert abs(sum(float(p[0]) for p in parts) - float(loss)) <= 1e-6 * float(loss)
    assert np.allclose(sum(p[1] for p in parts), dx, rtol=0, atol=1e-6 * np.abs(dx).max())


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_install_refuses_what_the_kernels_do_not_implement():
    from keypointnerf_amd.vgg import NativeVGGLoss
    m = vg.StandInVGGLoss()
    NativeVGGLoss(m)
    bad = vg.StandInVGGLoss()
    bad.vgg_net.slice2[3] = torch.nn.Conv2d(64, 128, 5, padding=2).requires_grad_(False)
    with pytest.raises(NotImplementedError):
        NativeVGGLoss(bad)
    bad = vg.StandInVGGLoss()
    bad.vgg_net.slice3[2] = torch.nn.MaxPool2d(2, 2, ceil_mode=True)
    with pytest.raises(NotImplementedError):
        NativeVGGLoss(bad)
    bad = vg.StandInVGGLoss()
    bad.vgg_net.slice4[0].weight.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        NativeVGGLoss(bad)


def test_cpu_tensors_go_to_the_modules_own_forward():
    from keypointnerf_amd.vgg import NativeVGGLoss
    m = vg.StandInVGGLoss()
    x, y = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    assert torch.equal(NativeVGGLoss(m)(x, y), m(x, y))


@pytest.fixture
def emulated_op(monkeypatch):
    """torch.ops.kpnerf.vgg_loss on the emulator for the duration of a test (a scoped CPU kernel, as in
    test_dropin_real_class_emulated.py) and CPU tensors inside the served envelope"""
    from keypointnerf_amd import lib as kl, ops, torch_ops, vgg
    L = sh.simt_lib()
    monkeypatch.setattr(kl, "get_library", lambda: L)
    monkeypatch.setattr(ops, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(vgg.NativeVGGLoss, "served", lambda self, x, y: x.dim() == 4 and x.shape[-1] >= 8 and x.shape[-2] >= 8)
    with torch.library._scoped_library("kpnerf", "FRAGMENT") as frag:
        frag.impl("vgg_loss", torch_ops.vgg_loss._init_fn, "CPU")
        yield L


def test_native_term_through_compute_error_and_autograd(emulated_op):
    from keypointnerf_amd.losses import compute_error
    from keypointnerf_amd.vgg import NativeVGGLoss
    m = vg.StandInVGGLoss()
    tex = torch.rand(1, 3, 8, 8, requires_grad=True)
    tar = torch.rand(1, 3, 8, 8)
    nat = NativeVGGLoss(m)
    loss = 0.5 * nat(tex, tar)
    loss.backward()
    ref = tex.detach().clone().requires_grad_(True)
    (0.5 * m(ref, tar)).backward()
    assert abs(float(loss) - float(0.5 * m(ref, tar))) <= 1e-5 * float(loss)
    cos = float((tex.grad * ref.grad).sum() / (tex.grad.norm() * ref.grad.norm()))
    assert cos >= 0.9999
    # repacked after an in-place parameter change, not before
    packed = nat.packed
    nat(tex, tar)
    assert nat.packed is packed
    with torch.no_grad():
        m.vgg_net.slice1[0].bias.add_(0.01)
    nat(tex, tar)
    assert nat.packed is not packed


needs_reference = pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference source tree (KPNERF_REFERENCE_ROOT)")


@needs_reference
def test_install_vgg_on_the_live_reference_class(emulated_op):
    """the reference's own VGGLoss (src/utils.py:750-805, seeded stand-in weights): install_vgg keeps the module tree and the
    state_dict, serves net.vgg_loss natively (also through the reference's own compute_error, src/utils.py:97-171, as
    KeypointNeRF.forward calls it at src/model.py:894), and uninstall_vgg restores the method."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("make_vgg_golden", os.path.join(os.path.dirname(os.path.dirname(__file__)),
                                                                                  "scripts", "make_vgg_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    VGGLoss = gen.load_reference_vggloss()
    from keypointnerf_amd.vgg import NativeVGGLoss, install_vgg, uninstall_vgg
    net = torch.nn.Module()
    net.vgg_loss = VGGLoss()
    keys, mods = list(net.state_dict()), [n for n, _ in net.named_modules()]
    x, y = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    ref = float(net.vgg_loss(x, y))
    install_vgg(net)
    assert isinstance(net.vgg_loss.forward, NativeVGGLoss)
    assert list(net.state_dict()) == keys and [n for n, _ in net.named_modules()] == mods
    got = float(net.vgg_loss(x, y))
    assert abs(got - ref) <= 1e-5 * ref
    ref_shim.load_reference()
    loss, err = sys.modules["src.utils"].compute_error(out_nerf={"tex_cal_fine": x, "tar_img": y}, vggloss=net.vgg_loss,
                                       lambdas={"lambda_l1": 0.0, "lambda_l1_c": 0.0, "lambda_vgg": 0.5})
    assert abs(float(err["e_vgg"]) - 0.5 * got) <= 1e-6 * got
    uninstall_vgg(net)
    assert "forward" not in net.vgg_loss.__dict__ and float(net.vgg_loss(x, y)) == ref
