"""The fp16 range guard on every path that runs behind it, on the MI355X (-m gpu): density first forced on and off, passes of several
batches (a 1 MiB row scratch cap: batches of 262,144 points, concurrent workgroups in k_mask_compact), kpn_query, the per-call kernel
selection and the train branch with and without a kept state.  Inputs and checks: tests/range_guard_cases.py; the same cases on the
emulator: tests/test_range_guard_cpu.py.  Every process-wide setting a check changes is restored behind it (rows mode 3, fuse mode 1,
density first auto, range guard on, the row scratch cap): tests/test_gpu_range.py asserts the defaults."""
import ctypes

import numpy as np
import pytest
import torch

from tests import range_guard_cases as rg

pytestmark = pytest.mark.gpu

CAP = 1 << 20    # kpn_set_row_scratch_cap_bytes: the floor of 262,144 points per batch applies


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class DeviceDriver:
    emulated, batch_points = False, 262144

    def __init__(self):
        assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
        from keypointnerf_amd import lib as kl
        from keypointnerf_amd import ops
        self.ops, self.lib = ops, kl.get_library()

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scene(self, scene):
        from keypointnerf_amd.synthetic import to_device
        s = to_device(scene, "cuda")
        return s, self.ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])

    def weights(self, sd):
        return self.ops.PackedWeights(sd)

    def render(self, hs, w, scene, grid, Sc, Sf, fine=True, rows_kernel=None, fuse_kernel=None):
        s, ps = hs
        plan = self.ops.RenderPlan(ps, grid, Sc, Sf, fine=fine, rows_kernel=rows_kernel, fuse_kernel=fuse_kernel)
        out = self.ops.render_rays(ps, w, s["cam_tar"], s["bounds"], plan=plan)
        return {k: v[0].cpu().numpy() for k, v in out.items()}

    def query(self, hs, w, pts, view, mode):
        out, valid = self.ops.query(hs[1], w, _cu(pts), _cu(view), mode=mode)
        return out[0].cpu().numpy(), valid.reshape(-1).cpu().numpy()

    @staticmethod
    def _train_args(hs, w, d):
        s, ps = hs
        return ((ps, w, s["cam_tar"], s["bounds"], _cu(d.pix), _cu(d.u_c), _cu(d.u_f), d.keep_c, d.keep_f),
                dict(noise_coarse=_cu(d.n_c), noise_fine=_cu(d.n_f), rand_noise_std=d.std, n_coarse=d.Sc, n_fine=d.Sf))

    def train_forward(self, hs, w, scene, d, keep_state=False):
        args, kw = self._train_args(hs, w, d)
        res = self.ops.render_rays_train(*args, keep_state=keep_state, **kw)
        out, state = res if keep_state else (res, None)
        return {k: v[0].cpu().numpy() for k, v in out.items()}, state

    def train_backward(self, hs, w, scene, d, state=None):
        args, kw = self._train_args(hs, w, d)
        grads = {k: _cu(v).reshape(1, *v.shape) for k, v in d.grads.items()}
        return [g.cpu().numpy() for g in self.ops.render_rays_train_backward(*args, grads, state=state, **kw)]


@pytest.fixture(scope="module")
def drv():
    return DeviceDriver()


@pytest.fixture(scope="module")
def world(drv):
    """the 10 x 10 base scene, a density head biased so that the hull holds dead and live points"""
    return rg.World(drv, density_bias=rg.DENSITY_BIAS)


@pytest.fixture(scope="module")
def plain(drv):
    """the 10 x 10 base scene with the unbiased density head"""
    return rg.World(drv)


# ---- 1. density first and the guard ----
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["map", "activation", "colour"])
def test_density_first_and_the_guard(world, name, mode):
    rg.check_density_first(world, name, mode)


def test_colour_input_overflows_in_pass_b_only(world):
    rg.check_colour_overflows_in_pass_b_only(world)


def test_in_range_frame_leaves_the_counter_alone_in_both_forms(world):
    rg.check_base_frame(world)


# ---- 2. several batches, one of them flagged ----
def test_only_the_flagged_batch_is_evaluated_again(plain):
    """about 600 k valid points in batches of 262,144: at least three batches, the valid list's order across workgroups from an atomic"""
    rg.check_one_flagged_batch(plain, n_candidates=1_300_000, n_valid=600_000, cap=CAP)


# ---- 3. several batches in a render pass ----
def test_batched_render_pass_fused_and_density_first(drv):
    """256 x 256 rays at 12 samples through a dense mask: one pass of 786 k points, between 43 and 64 % of them valid, so two batches of
    at most 262,144 at any fraction in that range; the oracle renders every 17th ray."""
    rg.check_batched_render(rg.World(drv, tar_hw=(256, 256), mask="dense", density_bias=rg.DENSITY_BIAS), cap=CAP, oracle_stride=17)


# ---- 4. kpn_query ----
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", rg.OVERFLOWS)
def test_query_entry_point(plain, name, mode):
    rg.check_query(plain, name, mode)


# ---- 5. per-call kernel selection ----
@pytest.mark.parametrize("name,plan", rg.PLAN_CASES)
def test_per_call_kernel_selection(plain, name, plan):
    rg.check_per_call_kernels(plain, name, plan)


# ---- 6. train branch ----
@pytest.mark.parametrize("name", ["activation", "weight"])
def test_train_branch_forward_and_backward(plain, name):
    rg.check_train(plain, name, keep_state=True)
