"""The fp16 range guard on every path that runs behind it, on the host SIMT emulator: the very kernel sources and run_field, with numpy
buffers through the C ABI.  Inputs and checks: tests/range_guard_cases.py; the same cases on the device: tests/test_gpu_range_guard.py.
(The emulator build batches a pass at 2048 points and runs workgroups serially.)"""
import pytest

from tests import range_guard_cases as rg
from tests import simt_harness as sh


class HostDriver:
    emulated, batch_points = True, 2048

    def __init__(self):
        self.lib = sh.simt_lib()

    def stream(self):
        return None

    def scene(self, scene):
        return sh.HostScene(self.lib, scene)

    def weights(self, sd):
        return sh.pack_weights(self.lib, sd)

    def render(self, hs, w, scene, grid, Sc, Sf, fine=True, rows_kernel=None, fuse_kernel=None):
        return sh.render(self.lib, hs, w, scene["cam_tar"], scene["bounds"], grid, Sc, Sf, fine=fine, rows_kernel=rows_kernel,
                         fuse_kernel=fuse_kernel)

    def query(self, hs, w, pts, view, mode):
        return sh.query(self.lib, hs, w, pts, view, mode=mode)

    def _train_args(self, hs, w, scene, d):
        return (self.lib, hs, w, scene["cam_tar"], scene["bounds"], d.pix, d.Sc, d.Sf, d.u_c, d.n_c, d.n_f, d.u_f, d.keep_c, d.keep_f, d.std)

    def train_forward(self, hs, w, scene, d, keep_state=False):
        assert not keep_state
        return sh.render_train(*self._train_args(hs, w, scene, d)), None

    def train_backward(self, hs, w, scene, d, state=None):
        assert state is None
        return sh.render_train_backward(*self._train_args(hs, w, scene, d), d.grads)


@pytest.fixture(scope="module")
def drv():
    return HostDriver()


@pytest.fixture(scope="module")
def world(drv):
    """the 10 x 10 base scene, a density head biased so that the hull holds dead and live points"""
    return rg.World(drv, density_bias=rg.DENSITY_BIAS)


@pytest.fixture(scope="module")
def plain(drv):
    """the 10 x 10 base scene with the unbiased density head"""
    return rg.World(drv)


# ---- 1. density first and the guard (the fused form: one case, the emulator guard test of tests/test_kernels_simt.py runs the rest in
# auto mode, which stays on the fused kernel) ----
@pytest.mark.parametrize("name,mode", [("map", 1), ("activation", 1), ("colour", 1), ("activation", 0)])
def test_density_first_and_the_guard(world, name, mode):
    rg.check_density_first(world, name, mode)


def test_colour_input_overflows_in_pass_b_only(world):
    rg.check_colour_overflows_in_pass_b_only(world)


def test_in_range_frame_leaves_the_counter_alone_in_both_forms(world):
    rg.check_base_frame(world)


# ---- 2. several batches, one of them flagged ----
def test_only_the_flagged_batch_is_evaluated_again(plain):
    rg.check_one_flagged_batch(plain, n_candidates=7500, n_valid=3800)


# ---- 3. several batches in a render pass ----
def test_batched_render_pass_fused_and_density_first(drv):
    """22 x 22 rays at 12 samples through a dense mask: more than 2048 valid points, two batches"""
    rg.check_batched_render(rg.World(drv, tar_hw=(22, 22), mask="dense", density_bias=rg.DENSITY_BIAS))


# ---- 4. kpn_query ----
# (each input once and each mode twice here, 19 s a case; the device file runs all eight)
@pytest.mark.parametrize("name,mode", [("map", 0), ("weight", 1), ("activation", 0), ("colour", 1)])
def test_query_entry_point(plain, name, mode):
    rg.check_query(plain, name, mode)


# ---- 5. per-call kernel selection ----
# (one plan per input here: both f16 kernels standing aside, and the two mixed pairs with a flagged batch; the device file runs all five)
@pytest.mark.parametrize("name,plan", [rg.PLAN_CASES[0], rg.PLAN_CASES[3], rg.PLAN_CASES[4]])
def test_per_call_kernel_selection(plain, name, plan):
    rg.check_per_call_kernels(plain, name, plan)


# ---- 6. train branch ----
# (the flagged-batch input here, 44 s; the device file also runs the input whose kernels stand aside, and both with a kept state)
def test_train_branch_forward_and_backward(plain):
    rg.check_train(plain, "activation")
