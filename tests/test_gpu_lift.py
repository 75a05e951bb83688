"""GPU suite (-m gpu) for the lifting of graphs to combinatorial complexes on the MI355X: the cases of tests/test_lift.py on k_lift_paths,
k_lift_cycles and k_lift_dense themselves, and Sampler.evaluate(..., lift=True) on finished runs."""
import pytest

from tests import lift_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("case", lc.PATH_CASES, ids=str)
def test_paths_against_the_restatement(lib, case):
    lc.case_paths(lib, DEV, case)


@pytest.mark.parametrize("name", ["n12", "n20"])
def test_paths_against_the_reference(lib, name):
    lc.case_golden_paths(lib, DEV, name)


@pytest.mark.parametrize("name", ["n12", "n20"])
def test_lifted_scores_against_the_reference(lib, name):
    lc.case_golden_scores(lib, DEV, name)


@pytest.mark.parametrize("key", list(lc.special_graphs()) + lc.CYCLE_RANDOM, ids=str)
def test_cycles_against_the_restatement(lib, key):
    lc.case_cycles(lib, DEV, key)


@pytest.mark.parametrize("case", lc.DENSE_CASES, ids=str)
def test_dense_output_and_finish_round_trip(lib, case):
    lc.case_dense(lib, DEV, case)


def test_lift_overwrites_its_outputs(lib):
    lc.case_overwrite(lib, DEV)


def test_lift_quantiser_and_upper_triangle(lib):
    lc.case_quantiser(lib, DEV)


def test_lift_bad_arguments(lib):
    lc.case_bad_args(lib, DEV)


def test_lift_is_opt_in(lib):
    lc.case_opt_in(lib, DEV)


def test_sampler_evaluate_lifts_the_held_out_graphs(lib, tmp_path):
    lc.case_sampler_evaluate_cc(lib, tmp_path)


def test_graph_sampler_evaluate_with_lift(lib, tmp_path):
    lc.case_sampler_evaluate_graph(lib, tmp_path)
