"""CPU suite for the NSPDK score (ccsd_nspdk_features, ccsd_nspdk_mmd, SampleOps.nspdk_features / nspdk_mmd, nspdk_stats, the nspdk=True
paths of ccsd_amd/evaluation.py and Sampler.evaluate) over the host emulation of k_nspdk_features and the MMD kernels: feature rows
against the reference's own vectoriser (tests/golden/e4_nspdk.npz) and a pure-Python restatement (tests/nspdk_ref.py), scores against
the reference's compute_nspdk_mmd."""
import pytest

from tests import nspdk_cases as nc
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_fixture_holds_the_generated_graph_sets():
    nc.case_fixture_matches_generator()


@pytest.mark.parametrize("name", nc.SET_NAMES)
def test_restatement_against_the_reference_vectoriser(name):
    nc.case_restatement_against_reference(name)


def test_graph_sets_exercise_blocks_depth_cap_and_merge_rule():
    nc.case_structure_of_the_sets()


@pytest.mark.parametrize("name", nc.SET_NAMES)
def test_emu_nspdk_rows_against_the_reference_vectoriser(lib, name):
    nc.case_reference_rows(lib, DEV, name)


def test_emu_nspdk_random_graphs_against_the_restatement(lib):
    nc.case_random_against_restatement(lib, DEV)


def test_emu_nspdk_two_calls_give_identical_bits(lib):
    nc.case_two_calls_same_bits(lib, DEV)


def test_emu_nspdk_labels_and_modes(lib):
    nc.case_labels_and_modes(lib, DEV)


def test_emu_nspdk_bad_arguments(lib):
    nc.case_bad_arguments(lib, DEV)


@pytest.mark.parametrize("name", nc.SET_NAMES)
def test_emu_nspdk_mmd_against_the_reference(lib, name):
    nc.case_mmd(lib, DEV, name)


def test_emu_nspdk_mmd_of_a_set_against_itself_and_empty_rows(lib):
    nc.case_mmd_self_and_empty_rows(lib, DEV)


def test_emu_nspdk_scores(lib):
    nc.case_scores(lib, DEV)


def test_emu_nspdk_is_opt_in(lib):
    nc.case_opt_in(lib, DEV)


def test_emu_sampler_evaluate_with_nspdk(lib, tmp_path):
    nc.case_sampler_evaluate(lib, tmp_path)


def test_emu_generic_sampler_evaluate_with_nspdk(lib, tmp_path):
    nc.case_sampler_evaluate_generic(lib, tmp_path)
