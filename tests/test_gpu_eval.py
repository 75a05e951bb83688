"""GPU suite (-m gpu) for the evaluation of finished samples on the MI355X: the cases of tests/test_eval.py on k_cluster_hist, k_mmd_prep,
k_mmd_pairs and k_mmd_final themselves."""
import pytest

from tests import eval_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("bins", ec.BINS)
@pytest.mark.parametrize("name", ec.GRAPH_SETS)
def test_cluster_hist(lib, name, bins):
    ec.case_cluster(lib, DEV, name, bins)


def test_cluster_landmarks(lib):
    ec.case_cluster_landmarks(lib, DEV)


def test_cluster_raw_samples_and_null_outputs(lib):
    ec.case_cluster_raw_and_null(lib, DEV)


def test_bad_dims(lib):
    ec.case_bad_dims(lib, DEV)


@pytest.mark.parametrize("name", list(ec.MMD_SHAPES))
def test_mmd_against_restatement(lib, name):
    ec.case_mmd_restatement(lib, DEV, name)


@pytest.mark.parametrize("name", ["n3_l2", "n64_l33", "n130_l33"])
def test_mmd_of_identical_sets_is_zero(lib, name):
    ec.case_mmd_identical(lib, DEV, name)


@pytest.mark.parametrize("name", ec.mmd_fixture_sets())
def test_mmd_against_reference_scores(lib, name):
    ec.case_mmd_reference(lib, DEV, name)


def test_eval_torch_batch(lib):
    ec.case_eval_torch_batch(lib, DEV)


def test_eval_cc_batch(lib):
    ec.case_eval_cc_batch(lib, DEV)


def test_unsupported_methods_raise(lib):
    ec.case_unsupported(lib, DEV)
