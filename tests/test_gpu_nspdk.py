"""GPU suite (-m gpu) for the NSPDK score on the MI355X: the cases of tests/test_nspdk.py on k_nspdk_features and the MMD kernels
themselves, and Sampler.evaluate(..., nspdk=True) on a finished molecule run."""
import pytest

from tests import nspdk_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("name", nc.SET_NAMES)
def test_nspdk_rows_against_the_reference_vectoriser(lib, name):
    nc.case_reference_rows(lib, DEV, name)


def test_nspdk_random_graphs_against_the_restatement(lib):
    nc.case_random_against_restatement(lib, DEV)


def test_nspdk_two_calls_give_identical_bits(lib):
    nc.case_two_calls_same_bits(lib, DEV)


def test_nspdk_labels_and_modes(lib):
    nc.case_labels_and_modes(lib, DEV)


def test_nspdk_bad_arguments(lib):
    nc.case_bad_arguments(lib, DEV)


@pytest.mark.parametrize("name", nc.SET_NAMES)
def test_nspdk_mmd_against_the_reference(lib, name):
    nc.case_mmd(lib, DEV, name)


def test_nspdk_mmd_of_a_set_against_itself_and_empty_rows(lib):
    nc.case_mmd_self_and_empty_rows(lib, DEV)


def test_nspdk_scores(lib):
    nc.case_scores(lib, DEV)


def test_nspdk_is_opt_in(lib):
    nc.case_opt_in(lib, DEV)


def test_sampler_evaluate_with_nspdk(lib, tmp_path):
    nc.case_sampler_evaluate(lib, tmp_path)


def test_generic_sampler_evaluate_with_nspdk(lib, tmp_path):
    nc.case_sampler_evaluate_generic(lib, tmp_path)
