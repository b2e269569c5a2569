"""Keypoint sets on the MI355X: models with 1..24 keypoints and 0..3 encoding octaves served as the kernels' 24 / 3 model
(include/kpnerf.h, "Keypoint sets").  The oracle is the reference's own record of two such models (tests/golden/case_kp13_l3.npz,
case_kp17_l2.npz, made by scripts/make_keypoint_set_golden.py) and, for the degenerate 1 / 0 model, the eager restatement; the new
C entries are checked on the device bit for bit as on the emulator (tests/keypoint_set_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import keypoint_set_cases as kc
from tests import param_step_cases as pc

pytestmark = pytest.mark.gpu
_IDS = [kc.case_id(c) for c in kc.CASES]
_GOLDEN = list(kc.GOLDEN_CASES)


@pytest.fixture(scope="module")
def drv():
    from keypointnerf_amd import lib as kl

    def to_host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return pc.Driver(kl.get_library(), to_dev=lambda a: torch.from_numpy(np.array(a)).cuda(), ptr=lambda t: ctypes.c_void_p(t.data_ptr()),
                     to_host=to_host, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_kernel", ["f16x2", "bf16x3", "f32"])
@pytest.mark.parametrize("case", _GOLDEN, ids=kc.case_id)
def test_tile_through_the_c_abi(case, rows_kernel):
    kc.check_golden_render_abi(case, "cuda", rows_kernel)


@pytest.mark.parametrize("rows_mode", [3, 2, 0])
@pytest.mark.parametrize("case", _GOLDEN, ids=kc.case_id)
def test_tile_through_install(case, rows_mode):
    kc.check_golden_render_install(case, "cuda", rows_mode)


@pytest.mark.parametrize("native", [False, True], ids=["default", "native_params"])
@pytest.mark.parametrize("case", _GOLDEN, ids=kc.case_id)
def test_training_step_through_the_dropin(case, native):
    kc.check_golden_train(case, "cuda", native_params=native)


# ---- the C entries on the device, bit for bit ---------------------------------------------------------------------------------
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


def test_scene_tables_repeat_keypoint_0_in_the_padded_rows():
    from keypointnerf_amd import lib as kl, ops
    from keypointnerf_amd.synthetic import make_scene
    L = kl.get_library()
    s = make_scene(n_views=3, src_hw=(64, 64), tar_hw=(16, 16), mask="ellipsoid", seed=5, device="cuda")
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    kpt24 = s["sp_data"]["kpt3d"].reshape(24, 3).cpu().numpy()
    off = (ctypes.c_size_t * 6)()
    L.check(L.kpn_scene_layout(ctypes.byref(ps.desc), off))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = ps.desc.kpt3d

    def prepare(kpt, n):
        k = torch.from_numpy(np.ascontiguousarray(kpt, np.float32)).cuda()
        ws = torch.full_like(ps.ws, float("nan"))
        ps.desc.kpt3d = k.data_ptr()
        if n is None:
            assert tuple(k.shape) == (24, 3)
            L.check(L.kpn_scene_prepare(ctypes.byref(ps.desc), ctypes.c_void_p(ws.data_ptr()), stream))
        else:
            assert tuple(k.shape) == (n, 3)
            L.check(L.kpn_scene_prepare_kpt(ctypes.byref(ps.desc), n, ctypes.c_void_p(ws.data_ptr()), stream))
        torch.cuda.synchronize()
        ps.desc.kpt3d = keep
        return ws.cpu().numpy(), list(off), 3

    kc.check_scene_tables(prepare, kpt24)
    ref, _, _ = prepare(kpt24, None)
    tbl = slice(int(off[0]), int(off[0]) + 3 * 112)                    # (the gaps between the regions are never written)
    assert ref[tbl].tobytes() == ps.ws.cpu().numpy()[tbl].tobytes()    # ops.PreparedScene on 24 keypoints: today's tables
    ws = torch.full_like(ps.ws, float("nan"))
    for n in (0, 25):
        assert L.kpn_scene_prepare_kpt(ctypes.byref(ps.desc), n, ctypes.c_void_p(ws.data_ptr()), stream) == -1
        assert b"n_kpt" in L.kpn_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all())                                 # nothing was launched


# ---- the degenerate shape -----------------------------------------------------------------------------------------------------
def test_one_keypoint_no_octaves_against_the_eager_restatement():
    """(1, 0): one keypoint, dz w alone — a first layer of 1 + 64 inputs.  Rendered through the C ABI and compared with
    oracle/torch_eager.py on what the kernels are told to compute: the widened parameters and the keypoint repeated 24 times (the
    eager restatement has no notion of a narrow model, so it also checks that the padded values change nothing).  Bar: the
    project's 1e-4 on colour and alpha."""
    from keypointnerf_amd import ops, weights
    from keypointnerf_amd.synthetic import make_scene, random_hotpath_state_dict
    from oracle import torch_eager as te
    n, lv, tile = 1, 0, 8
    sd = random_hotpath_state_dict(seed=30, n_kpt=n, sp_level=lv)
    assert tuple(sd["mlp_geo.layers1.layers.0.linear.weight_v"].shape) == (128, 65)
    s = make_scene(n_views=3, src_hw=(64, 64), tar_hw=(tile, tile), mask="ellipsoid", seed=53, tar_focal_at_512=800.0, n_kpt=n, device="cuda")
    assert tuple(s["sp_data"]["kpt3d"].shape) == (1, 1, 3)
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    narrow = torch.from_numpy(weights.flatten_plain(weights.effective_weights(sd, (n, lv)))).cuda()
    plain = ops.widen_plain(narrow, n, lv)
    out = ops.render_rays(ps, ops.PackedWeights.from_plain(plain, device="cuda"), s["cam_tar"], s["bounds"], grid=(0, 0, 1, tile, tile),
                          n_coarse=16, n_fine=16)
    padded = dict(s, sp_data={"kpt3d": s["sp_data"]["kpt3d"].expand(1, 24, 3).contiguous(), "extrin": s["sp_data"]["extrin"]})
    yy, xx = torch.meshgrid(torch.arange(tile), torch.arange(tile), indexing="ij")
    pix = torch.stack([xx.reshape(-1), yy.reshape(-1)], -1).cuda()
    with torch.no_grad():
        ref = te.render_rays(te.unpack_plain(plain), padded, pix, 16, 16, fine=True, sigma=0.1)
    a = ref["alpha_fine"]
    assert float(a.max()) > 0.5 and float(a.min()) < 0.05, (float(a.min()), float(a.max()))   # a subject and a background
    for k in ("tex_fg", "alpha", "tex_fg_fine", "alpha_fine"):
        got = out[k][0].permute(1, 2, 0).reshape(-1, 3) if out[k].dim() == 4 else out[k].reshape(-1)
        err = float((got - ref[k]).abs().max())
        print(f"kp1_l0 {k}: max |got - eager| = {err:.3e} (bar 1e-4)")
        assert err <= 1e-4, (k, err)
