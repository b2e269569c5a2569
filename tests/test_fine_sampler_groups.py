"""k_fine_samples_w takes its rays in groups (16 per wavefront for Sc, Sf <= 64, otherwise 8): one lane per ray walks the cdf, then
the group's rays are drawn and merged one at a time.  Ray counts around a group, a wavefront's group and a workgroup (1, 63, 64, 65,
257; on the device one above the 4 x 8192 x 16 rays of a full grid, so the grid-stride loop runs with a ragged tail) at sample counts
on both specialisations, with uniform u (the eval branch) and unsorted random u (the train branch).

The check is the existing one (tests/ray_stage_cases.py): z_fine of the render's stages is bit-equal to kpn_importance_sample on the
render's own coarse stage plus a NumPy sort(cat).  The new samples and the source index behind z_fine are checked through what the
render does with them: z_fine is sorted, and rgba_fine holds the coarse records exactly at the coarse depths' merged positions.
The rows come from case_c's field: rays that miss the body give all-zero contribution rows, rays that graze it rows with one spike,
the others general rows; each test prints what it met and the 64-ray lattice asserts all three kinds."""
import numpy as np
import pytest
import torch

from tests import ray_stage_cases as rc
from tests.golden_io import load_case, load_weights

# ray count -> the lattice (x0, y0, step, nx, ny) on case_c's 24 x 24 target (rays beyond the image are still rays)
GRIDS = {1: (12, 12, 1, 1, 1), 17: (2, 12, 1, 17, 1), 63: (0, 0, 3, 9, 7), 64: (0, 0, 3, 8, 8), 65: (0, 2, 2, 13, 5), 257: (0, 12, 1, 257, 1)}
SIZES = [(3, 1), (8, 12), (64, 64), (65, 64), (128, 128)]
RAYS = [1, 63, 64, 65, 257]
# the emulator evaluates the field at 2 ms a point: every ray count at (3, 1), three at (8, 12), one ray at the large sizes and
# 17 rays (two or three groups, the last one ragged) on each specialisation
EMU_EVAL = [(3, 1, r) for r in RAYS] + [(8, 12, 1), (8, 12, 63), (8, 12, 65), (64, 64, 1), (64, 64, 17), (65, 64, 1), (65, 64, 17), (128, 128, 1)]
EMU_TRAIN = [(3, 1, 65), (8, 12, 65), (65, 64, 17)]
# one above a full grid of the smaller specialisation's groups: 4 wavefronts x 8192 workgroups x 16 rays; the lattice ends on the
# image's row 11, so the rays that only the stride loop reaches cross the body
BIG_NX, BIG_NY = 724, 725
assert BIG_NX * BIG_NY > 4 * 8192 * 16 and (BIG_NX * BIG_NY) % 16 != 0


def pixels(grid):
    x0, y0, step, nx, ny = grid
    ys, xs = np.meshgrid(y0 + step * np.arange(ny), x0 + step * np.arange(nx), indexing="ij")
    return np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32)


def row_kinds(L, B, st):
    """(all-zero, one-spike, general) rows of contrib[..., 1:-1], the sampler's input, from the render's coarse stage"""
    contrib = rc.rgba2out(L, B, st["rgba_coarse"], st["z_coarse"])[3][:, 1:-1]
    nz = (contrib != 0).sum(-1)
    kinds = int((nz == 0).sum()), int((nz == 1).sum()), int((nz > 1).sum())
    print(f"[fine sampler] {len(nz)} rays x {contrib.shape[1]} bins: {kinds[0]} zero rows, {kinds[1]} one-spike rows, {kinds[2]} general rows")
    return kinds


def check(L, B, st, Sc, Sf, R, u=None):
    assert st["z_fine"].shape == (R, Sc + Sf)
    znew = rc.check_sampler_agrees(L, B, st, Sf, u, min_hit_rays=0)
    rc.check_coarse_records_kept(st, znew)
    kinds = row_kinds(L, B, st)
    if R == 64 and Sc == 8 and u is None:
        assert min(kinds) > 0, kinds
    elif R >= 63:
        assert kinds[0] > 0 and kinds[1] + kinds[2] > 0, kinds


def train_u(Sc, Sf, R):
    rng = np.random.default_rng(8800 + 1000 * Sc + 10 * Sf + R)
    return rng.random((R, Sc), dtype=np.float32), rng.random((R, Sf), dtype=np.float32)      # iid: unsorted


# ---- the emulator build ----
@pytest.fixture(scope="module")
def emu():
    from tests import simt_harness as sh
    L = sh.simt_lib()
    scene, _, _ = load_case(rc.CASE_C)
    return sh, L, rc.HostArrays(), scene, sh.HostScene(L, scene), sh.pack_weights(L, load_weights())


@pytest.mark.parametrize("Sc,Sf,R", EMU_EVAL)
def test_groups_eval_emulated(emu, Sc, Sf, R):
    sh, L, B, scene, hs, packed = emu
    _, st = sh.render(L, hs, packed, scene["cam_tar"], scene["bounds"], GRIDS[R], Sc, Sf, stages=True)
    check(L, B, st, Sc, Sf, R)


@pytest.mark.parametrize("Sc,Sf,R", EMU_TRAIN)
def test_groups_train_emulated(emu, Sc, Sf, R):
    sh, L, B, scene, hs, packed = emu
    u_c, u_f = train_u(Sc, Sf, R)
    _, st = sh.render_train(L, hs, packed, scene["cam_tar"], scene["bounds"], pixels(GRIDS[R]), Sc, Sf, u_c, None, None, u_f, 7, 7, 0.0, stages=True)
    check(L, B, st, Sc, Sf, R, u_f)


# ---- the device ----
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from keypointnerf_amd import lib as kl
    from keypointnerf_amd import ops
    from keypointnerf_amd.synthetic import to_device
    s = to_device(load_case(rc.CASE_C)[0], "cuda")
    ps = ops.PreparedScene(s["img"], s["cam"], s["feat_geo"], s["feat_tex"], s["sp_data"], s["src_foreground_mask"])
    return kl.get_library(), rc.DeviceArrays(), ops, s, ps, ops.PackedWeights(load_weights())


def _eval_stages(dev, grid, Sc, Sf, chunk_rays=0):
    _, _, ops, s, ps, w = dev
    _, st = ops.render_rays(ps, w, s["cam_tar"], s["bounds"], grid=grid, n_coarse=Sc, n_fine=Sf, chunk_rays=chunk_rays, stages=True)
    return {k: v.cpu().numpy() for k, v in st.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("R", RAYS)
@pytest.mark.parametrize("Sc,Sf", SIZES)
def test_groups_eval(dev, Sc, Sf, R):
    check(dev[0], dev[1], _eval_stages(dev, GRIDS[R], Sc, Sf), Sc, Sf, R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", RAYS)
@pytest.mark.parametrize("Sc,Sf", SIZES)
def test_groups_train(dev, Sc, Sf, R):
    L, B, _, s, ps, w = dev
    cam_tar = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in s["cam_tar"].items()}
    u_c, u_f = train_u(Sc, Sf, R)
    st = rc.render_train_device(L, B, ps, w, cam_tar, s["bounds"].cpu(), pixels(GRIDS[R]), Sc, Sf, u_c, u_f)
    check(L, B, st, Sc, Sf, R, u_f)


@pytest.mark.gpu
def test_groups_stride_loop_with_a_ragged_tail(dev):
    R = BIG_NX * BIG_NY
    st = _eval_stages(dev, (24 - BIG_NX, 12 - BIG_NY, 1, BIG_NX, BIG_NY), 3, 1, chunk_rays=R)
    check(dev[0], dev[1], st, 3, 1, R)
    tail = rc.rgba2out(dev[0], dev[1], st["rgba_coarse"][4 * 8192 * 16:], st["z_coarse"][4 * 8192 * 16:])[2]
    assert (tail > 1e-3).any()                   # the rays behind the full grid are not all misses
