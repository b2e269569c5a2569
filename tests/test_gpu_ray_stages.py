"""The ray-stage kernels (keypointnerf_amd/csrc/ray_kernels.hip) on the MI355X: the C ABI on device memory, the same checks as
tests/test_ray_stages_cpu.py runs on the emulator (real cross-lane scans, v_readlane, LDS), and the grid-stride loops of the compositor
and of the render's sampler.  Cases, references and bars: tests/ray_stage_cases.py."""
import numpy as np
import pytest
import torch

from tests import ray_stage_cases as rc
from tests.golden_io import load_case, load_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from keypointnerf_amd import lib as kl
    return kl.get_library()


@pytest.fixture(scope="module")
def B():
    return rc.DeviceArrays()


@pytest.fixture(scope="module")
def world():
    """case_c on the device: (ops, scene tensors, PreparedScene, PackedWeights)"""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from keypointnerf_amd import ops
    from keypointnerf_amd.synthetic import to_device
    s = to_device(load_case(rc.CASE_C)[0], "cuda")
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    return ops, s, ps, ops.PackedWeights(load_weights())


def _eval_stages(world, grid, Sc, Sf, chunk_rays=0):
    ops, s, ps, w = world
    out, st = ops.render_rays(ps, w, s["cam_tar"], s["bounds"], grid=grid, n_coarse=Sc, n_fine=Sf, chunk_rays=chunk_rays, stages=True)
    return {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in st.items()}


def _host_camera(s):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s["cam_tar"].items()}, s["bounds"].cpu()


# ---- 1. compositor backward ----
@pytest.mark.parametrize("S", sorted(rc.BWD_CASES))
def test_backward_against_fp64(L, B, S):
    rc.check_backward_case(L, B, S)


@pytest.mark.parametrize("S", sorted(rc.BWD_CASES))
def test_backward_null_gradients_give_zeros_and_two_calls_equal_bits(L, B, S):
    rc.check_backward_null_and_repeat(L, B, S)


# ---- 2. the render's sampler against the stand-alone one ----
@pytest.mark.parametrize("Sc,Sf,step", rc.EVAL_CASES)
def test_render_sampler_is_the_stand_alone_sampler_eval(L, B, world, Sc, Sf, step):
    n = 24 // step
    _, st = _eval_stages(world, (0, 0, step, n, n), Sc, Sf)
    znew = rc.check_sampler_agrees(L, B, st, Sf)
    rc.check_coarse_records_kept(st, znew)


@pytest.mark.parametrize("Sc,Sf", rc.TRAIN_CASES)
def test_render_sampler_is_the_stand_alone_sampler_train(L, B, world, Sc, Sf):
    _, s, ps, w = world
    cam_tar, bounds = _host_camera(s)
    pix, u_c, u_f = rc.train_draws(Sc, Sf)
    st = rc.render_train_device(L, B, ps, w, cam_tar, bounds, pix, Sc, Sf, u_c, u_f)
    rc.check_sampler_agrees(L, B, st, Sf, u_f)
    assert (np.diff(st["z_fine"], axis=-1) >= 0).all()


# ---- 3. the stage entry points at their edges ----
@pytest.mark.parametrize("Dm2", rc.IS_BINS)
def test_importance_sample_edges_against_the_oracle(L, B, Dm2):
    rc.check_sampler_grid(L, B, Dm2, exact=False)


def test_importance_sample_refuses_129_bins(L, B):
    rc.check_sampler_refuses_129_bins(L, B)


@pytest.mark.parametrize("where", sorted(rc.BOX_ORIGINS))
def test_ray_bbox_edges_against_the_oracle(L, B, where):
    rc.check_ray_bbox(L, B, where, exact=False)


def test_make_rays_entry_point(L, B, world):
    cam_tar, bounds = _host_camera(world[1])
    rc.check_make_rays(L, B, cam_tar, bounds, _eval_stages(world, rc.MAKE_RAYS_GRID, 3, 1)[1])


# ---- 4. grid-stride paths ----
@pytest.mark.parametrize("S", [3, 65])
def test_rgba2out_stride_loop_and_prefetch(L, B, S):
    rc.check_rgba2out_stride(L, B, S)


def test_render_stride_loops_of_sampler_and_merged_compositor(L, B, world):
    """182 x 181 rays of case_c in one pass (rays beyond the 24 x 24 image are still rays) at 8 + 4 samples: 8,236 workgroups of four
    rays on grids capped at 8,192, so the sampler and the merged compositor run their stride loops with a ragged tail"""
    nx, ny = 182, 181
    assert nx * ny > 4 * 8192 and (nx * ny) % 4 != 0
    out, st = _eval_stages(world, (0, 0, 1, nx, ny), 8, 4, chunk_rays=nx * ny)
    znew = rc.check_sampler_agrees(L, B, st, 4)
    rc.check_coarse_records_kept(st, znew)
    # the merged compositor reads the same records in place: its images are, bit for bit, kpn_rgba2out of the merged stage arrays
    color, depth, alpha, _, sdf = rc.rgba2out(L, B, st["rgba_fine"], st["z_fine"])
    assert np.array_equal(rc.bits(out["tex_fg_fine"].reshape(3, -1).T), rc.bits(color))
    for k, v in (("depth_fine", depth), ("alpha_fine", alpha), ("sdf", sdf)):
        assert np.array_equal(rc.bits(out[k].reshape(-1)), rc.bits(v)), k
