"""The ray-stage kernels (keypointnerf_amd/csrc/ray_kernels.hip) on the host SIMT emulator: the very kernel sources, with numpy buffers
through the C ABI.  Cases, references and bars: tests/ray_stage_cases.py."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import ray_stage_cases as rc
from tests import simt_harness as sh
from tests.golden_io import GOLDEN_DIR, load_case, load_weights
from tests.test_oracle_vs_golden import assert_grad_close

B = rc.HostArrays()


@pytest.fixture(scope="module")
def L():
    return sh.simt_lib()


@pytest.fixture(scope="module")
def world(L):
    scene, _, _ = load_case(rc.CASE_C)
    return scene, sh.HostScene(L, scene), sh.pack_weights(L, load_weights())


# ---- 1. compositor backward ----
def test_restatement_is_the_oracles_and_the_references_backward():
    """the fp64 reference of the cases below, pinned: against the reference's own autograd (golden case_h) with the oracle's bar, and
    against the oracle's fp64 backward, which hands out fp32 (2^-24 relative per element), per ray within 1e-6 of the ray's largest
    gradient"""
    g = np.load(os.path.join(GOLDEN_DIR, "case_h_rgba2out_grad.npz"))
    rgba, z = sh.f32(g["rgba"][0]), sh.f32(g["z"][0])
    up = {k: sh.f32(g["d_" + k]).reshape(-1, 3) if k == "color" else sh.f32(g["d_" + k]).reshape(-1) for k in ("color", "depth", "alpha", "sdf")}
    assert_grad_close(rc.composite_backward(rgba, z, up), g["g_all"][0])
    assert_grad_close(rc.composite_backward(rgba, z, {"color": up["color"]}), g["g_color_only"][0])
    for S in (2, 65, 700):
        for call in rc.BWD_CALLS:
            rgba, z, up, r64, _ = rc.bwd_reference(S, call)
            o = oracle.rgba2out_backward(rgba, z, *[up.get(k) for k in ("color", "depth", "alpha", "sdf")])
            assert_grad_close(r64, o, rtol=1e-6)


@pytest.mark.parametrize("S", sorted(rc.BWD_CASES))
def test_backward_against_fp64(L, S):
    rc.check_backward_case(L, B, S)


@pytest.mark.parametrize("S", sorted(rc.BWD_CASES))
def test_backward_null_gradients_give_zeros_and_two_calls_equal_bits(L, S):
    rc.check_backward_null_and_repeat(L, B, S)


# ---- 2. the render's sampler against the stand-alone one ----
@pytest.mark.parametrize("Sc,Sf,step", rc.EVAL_CASES)
def test_render_sampler_is_the_stand_alone_sampler_eval(L, world, Sc, Sf, step):
    scene, hs, packed = world
    n = 24 // step
    _, st = sh.render(L, hs, packed, scene["cam_tar"], scene["bounds"], (0, 0, step, n, n), Sc, Sf, stages=True)
    znew = rc.check_sampler_agrees(L, B, st, Sf)
    rc.check_coarse_records_kept(st, znew)


@pytest.mark.parametrize("Sc,Sf", rc.TRAIN_CASES)
def test_render_sampler_is_the_stand_alone_sampler_train(L, world, Sc, Sf):
    scene, hs, packed = world
    pix, u_c, u_f = rc.train_draws(Sc, Sf)
    _, st = sh.render_train(L, hs, packed, scene["cam_tar"], scene["bounds"], pix, Sc, Sf, u_c, None, None, u_f, 7, 7, 0.0, stages=True)
    rc.check_sampler_agrees(L, B, st, Sf, u_f)
    assert (np.diff(st["z_fine"], axis=-1) >= 0).all()


# ---- 3. the stage entry points at their edges ----
@pytest.mark.parametrize("Dm2", rc.IS_BINS)
def test_importance_sample_edges_bit_equal_to_the_oracle(L, Dm2):
    differ, _ = rc.check_sampler_grid(L, B, Dm2, exact=True)
    assert differ == 0


def test_importance_sample_refuses_129_bins(L):
    rc.check_sampler_refuses_129_bins(L, B)


@pytest.mark.parametrize("where", sorted(rc.BOX_ORIGINS))
def test_ray_bbox_edges_bit_equal_to_the_oracle(L, where):
    rc.check_ray_bbox(L, B, where, exact=True)


def test_make_rays_entry_point(L, world):
    scene, hs, packed = world
    _, st = sh.render(L, hs, packed, scene["cam_tar"], scene["bounds"], rc.MAKE_RAYS_GRID, 3, 1, stages=True)
    rc.check_make_rays(L, B, scene["cam_tar"], scene["bounds"], st)


# ---- 4. the compositor's grid-stride loop (the sampler's needs a render of 32,773 rays: device only) ----
def test_rgba2out_stride_loop_and_prefetch(L):
    rc.check_rgba2out_stride(L, B, 3)
