"""The keypoint gradient (d loss / d sp_data["kpt3d"]; include/kpnerf.h, the *_kpt backward entries) on the MI355X: the checks of
tests/keypoint_grad_cases.py against the fp64 autograd restatement, the reference's own record of a training step
(tests/golden/case_kpgrad.npz) and one finite-difference check of the whole field."""
import pytest

from tests import keypoint_grad_cases as kg

pytestmark = pytest.mark.gpu


def test_rows_level_gradient():
    kg.check_rows("cuda")


def test_rows_level_one_point_one_view():
    kg.check_rows_one_point_one_view("cuda")


def test_rows_level_every_point_masked_out():
    kg.check_rows_all_masked("cuda")


def test_accumulation():
    kg.check_accumulation("cuda")


@pytest.mark.parametrize("shape", kg.NARROW, ids=kg.case_id)
def test_narrow_models(shape):
    kg.check_narrow("cuda", shape)


def test_finite_difference_of_the_field():
    kg.check_finite_difference("cuda")


@pytest.mark.parametrize("kept", [False, True], ids=["classic", "kept"])
@pytest.mark.parametrize("shape", kg.GOLDEN_SHAPES, ids=kg.case_id)
def test_training_step_against_the_reference_record(shape, kept):
    kg.check_golden_train("cuda", shape, kept)
