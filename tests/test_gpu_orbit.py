"""GPU suite (-m gpu) for the orbit score on the MI355X: the cases of tests/test_orbit.py on k_orbit_counts itself, and
Sampler.evaluate(..., orbits=True) on a finished run."""
import pytest

from tests import orbit_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("key", oc.BRUTE_SHAPES + ["special"], ids=str)
def test_orbits_against_brute_force(lib, key):
    oc.case_brute(lib, DEV, key)


def test_orbit_landmarks(lib):
    oc.case_landmarks(lib, DEV)


@pytest.mark.parametrize("name", oc.GRAPH_SETS + ("six4",))
def test_orbits_against_the_reference_counter(lib, name):
    oc.case_reference_rows(lib, DEV, name)


def test_orbits_of_k512_need_64_bits(lib):
    oc.case_k512(lib, DEV)


def test_orbit_raw_samples_and_null_outputs(lib):
    oc.case_raw_and_null(lib, DEV)


def test_orbit_bad_dims(lib):
    oc.case_bad_dims(lib, DEV)


def test_orbit_scores(lib):
    oc.case_scores(lib, DEV)


def test_orbits_are_opt_in(lib):
    oc.case_opt_in(lib, DEV)


def test_sampler_evaluate_with_orbits(lib, tmp_path):
    oc.case_sampler_evaluate(lib, tmp_path)
