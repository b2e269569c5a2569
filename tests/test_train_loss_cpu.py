"""k_train_loss (csrc/loss_kernels.hip, kpn_train_loss) on the wave64 emulator build: every pixel and mask term of the reference's
compute_error_nerf (src/utils.py:108-183) and the gradients autograd derives, against the formulas in fp64 (bar and cases:
tests/train_loss_cases.py), the exact cases, and the reference's recorded compute_error (golden case U) through
torch.ops.kpnerf.train_loss / losses.compute_error.  tests/test_gpu_train_loss.py repeats the kernel checks on the device."""
import json
import os

import numpy as np
import pytest
import torch

from tests import simt_harness as sh
from tests import train_loss_cases as tc


@pytest.fixture(scope="module")
def drv():
    return tc.Driver(sh.simt_lib(), to_dev=lambda a: np.array(a), ptr=sh.ptr, to_host=lambda a: a)


@pytest.mark.parametrize("n", tc.SHAPES)
def test_values_and_gradients_against_fp64(drv, n):
    tc.check_values_and_gradients(drv, n)


@pytest.mark.parametrize("n", tc.SHAPES)
def test_l1_terms_bit_identical_to_pix_l1_loss_and_rerun_without_reset(drv, n):
    tc.check_l1_bit_identical_and_rerun(drv, n)


def test_ties_have_zero_gradient(drv):
    tc.check_ties(drv)


def test_clamp_band_ends_and_nan(drv):
    tc.check_clamp_band(drv)


def test_skipped_terms_leave_their_gradient_buffers(drv):
    tc.check_skipped_terms_leave_their_buffers(drv)


def test_bad_arguments_are_error_codes(drv):
    L = drv.L
    assert L.kpn_train_loss_workspace_bytes(0) == 0 and L.kpn_train_loss_workspace_bytes(4096) >= 48 * 6 * 8 + 4
    import ctypes
    from keypointnerf_amd import lib as kl
    tex, terms, ws = np.zeros(3, np.float32), np.zeros(6, np.float32), np.zeros(L.kpn_train_loss_workspace_bytes(1), np.uint8)
    args = kl.TrainLossArgs(tex=sh.ptr(tex), n=1, l1_c=1.0, reset_ticket=1, terms=sh.ptr(terms))
    assert L.kpn_train_loss(ctypes.byref(args), sh.ptr(ws), None) == -1 and b"need tar" in L.kpn_last_error()
    args.n = 0
    assert L.kpn_train_loss(ctypes.byref(args), sh.ptr(ws), None) == -1 and b"pixel count" in L.kpn_last_error()


@pytest.fixture
def emulated_op(monkeypatch):
    """torch.ops.kpnerf.train_loss served by the emulator build on CPU tensors, and losses.compute_error taking its one-call
    path for them (as tests/test_dropin_real_class_emulated.py does for the other operators)"""
    from keypointnerf_amd import lib as kl, losses, ops, torch_ops
    L = sh.simt_lib()
    monkeypatch.setattr(kl, "get_library", lambda: L)
    monkeypatch.setattr(ops, "_on_gpu", lambda t: True)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(losses, "_on_device", lambda t: True)
    calls = []
    real = ops.train_loss
    monkeypatch.setattr(ops, "train_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.library._scoped_library("kpnerf", "FRAGMENT") as frag:
        frag.impl("train_loss", torch_ops.train_loss._init_fn, "CPU")
        yield calls


_REFERENCE_ORDER = ("e_pix_c", "e_pix_l1", "e_pix_l2", "e_pix_lp", "mask_loss_c", "mask_loss_f", "e_vgg", "e_all")   # src/utils.py:136-169, :104


def test_compute_error_through_the_operator_matches_the_reference_golden(emulated_op):
    """Golden case U (the reference's compute_error on 8 x 8 inputs, two lambda sets; the second switches l2, lp and the mask
    losses on): one operator call per compute_error, the reference's keys in the reference's order, and every value within the
    bar of tests/train_loss_cases.py — 4 x the recorded reference value's own distance from the fp64 formulas, plus an ulp."""
    from keypointnerf_amd import losses
    from tests.golden_io import GOLDEN_DIR
    z = np.load(os.path.join(GOLDEN_DIR, "case_u_loss_lambdas.npz"))
    out = {k[len("in."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
    inp = {"tex": z["in.tex_cal"].reshape(-1), "tex_fine": z["in.tex_cal_fine"].reshape(-1), "tar": z["in.tar_img"].reshape(-1),
           "alpha": z["in.alpha"].reshape(-1), "alpha_fine": z["in.alpha_fine"].reshape(-1), "tar_alpha": z["in.tar_alpha"].reshape(-1)}
    assert int(z["n_sets"]) == 2
    for i in range(2):
        lambdas = json.loads(str(z[f"set{i}.lambdas_json"]))
        want = dict(zip(z[f"set{i}.keys"].tolist(), z[f"set{i}.values"].tolist()))
        before = len(emulated_op)
        got_loss, got = losses.compute_error(out, None, lambdas)
        assert len(emulated_op) == before + 1                                       # ONE call serves every term
        assert list(got) == [k for k in _REFERENCE_ORDER if k in want], list(got)
        w = (lambdas.get("lambda_l1_c", 10.0), lambdas.get("lambda_l1", 10.0), lambdas.get("lambda_l2", 0.0), lambdas.get("lambda_lp", 0.0),
             lambdas.get("lambda_mloss", 0.0))
        ref64, _ = tc.formulas(inp, w, torch.float64)
        ref = dict(zip(tc.TERMS, ref64))
        ref["e_all"] = sum(ref[k] for k in want if k != "e_all")
        for k in want:
            b, e = tc.bar(want[k], np.array([ref[k]]))
            err = abs(float(got[k]) - ref[k])
            print(f"set{i} {k}: |native - fp64| = {err:.3e}, reference fp32 = {e:.3e}, bar = {b:.3e}")
            assert err <= b, (i, k, err, b)
        assert float(got_loss) == float(got["e_all"])


def test_operator_autograd_scales_each_term_by_its_upstream_gradient(emulated_op):
    """backward of torch.ops.kpnerf.train_loss: the saved seed gradients times the six upstream gradients, the three fine pixel
    terms summed into one d_tex_fine — against autograd on the fp64 formulas with the same per-term weights"""
    n = 65
    inp = tc.inputs(n)
    t = {k: torch.from_numpy(np.array(v)) for k, v in inp.items()}
    for k in ("tex", "tex_fine", "alpha", "alpha_fine"):
        t[k].requires_grad_(True)
    up = [0.5, 2.0, -1.5, 3.0, 0.25, 4.0]
    terms = torch.ops.kpnerf.train_loss(t["tex"].view(1, 3, 5, 13), t["tex_fine"].view(1, 3, 5, 13), t["tar"].view(1, 3, 5, 13),
                                        t["alpha"].view(1, 5, 13), t["alpha_fine"].view(1, 5, 13), t["tar_alpha"].view(1, 1, 5, 13), list(tc.WEIGHTS))[0]
    (terms * torch.tensor(up)).sum().backward()
    ref_t, ref_g = tc.formulas(inp, tc.WEIGHTS, torch.float64)
    eag_t, eag_g = tc.formulas(inp, tc.WEIGHTS, torch.float32)
    comb = lambda g: sum(up[1 + k] * g["d_tex_fine"][k] for k in range(3))
    for name, got, ref, eag in (("tex", t["tex"].grad, up[0] * ref_g["d_tex"], up[0] * eag_g["d_tex"]),
                                ("tex_fine", t["tex_fine"].grad, comb(ref_g), comb(eag_g)),
                                ("alpha", t["alpha"].grad, up[4] * ref_g["d_alpha"], up[4] * eag_g["d_alpha"]),
                                ("alpha_fine", t["alpha_fine"].grad, up[5] * ref_g["d_alpha_fine"], up[5] * eag_g["d_alpha_fine"])):
        b, e = tc.bar(eag, ref)
        b += 2 * float(np.spacing(np.float32(np.abs(ref).max())))        # the fp32 scaling and the two additions of the backward itself
        assert float(np.abs(got.numpy().astype(np.float64) - ref).max()) <= b, name
    # a switched-off term: its uninitialised seed gradient never reaches the result
    t["tex_fine"].grad = None
    terms = torch.ops.kpnerf.train_loss(None, t["tex_fine"], t["tar"], None, None, None, [0.0, 10.0, 0.0, 0.0, 4.0])[0]
    terms.sum().backward()
    assert np.array_equal(t["tex_fine"].grad.numpy(), np.asarray(tc.formulas(inp, (0.0, 10.0, 0.0, 0.0, 0.0), torch.float32)[1]["d_tex_fine"][0], np.float32))


def test_cpu_tensors_keep_the_per_term_path():
    """without a device (and without the emulation above) compute_error does not reach for the operator"""
    from keypointnerf_amd import losses
    out = {"tex_cal_fine": torch.rand(1, 3, 4, 4), "tar_img": torch.rand(1, 3, 4, 4)}
    assert not losses._fusable(out)
    loss, err = losses.compute_error(out, None, {"lambda_l1": 0.0, "lambda_l2": 2.0})
    assert list(err) == ["e_pix_l2", "e_all"] and abs(float(loss) - 2.0 * float((out["tex_cal_fine"] - out["tar_img"]).pow(2).mean())) < 1e-6
