"""CPU suite for the orbit score (ccsd_orbit_counts, SampleOps.orbit_counts, orbit_stats_all, the orbits=True paths of
ccsd_amd/evaluation.py and Sampler.evaluate) over the host emulation of k_orbit_counts: counts exact against a brute-force enumeration,
hand-written landmarks and the reference's own orbit counter (tests/golden/e3_orbit.npz), scores against the reference's."""
import pytest

from tests import orbit_cases as oc
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_fixture_covers_the_graph_sets():
    z3, meta = oc.e3()
    assert set(meta["graph_sets"]) == set(oc.GRAPH_SETS) | {"six4"}
    for name in meta["graph_sets"]:
        adj, _ = oc.graph_set(name)
        assert z3[f"graphs/{name}/orca"].shape == adj.shape[:2] + (15,) and z3[f"graphs/{name}/nodes"].shape == adj.shape[:1]


@pytest.mark.parametrize("key", oc.BRUTE_SHAPES + ["special"], ids=str)
def test_emu_orbits_against_brute_force(lib, key):
    oc.case_brute(lib, DEV, key)


def test_emu_orbit_landmarks(lib):
    oc.case_landmarks(lib, DEV)


@pytest.mark.parametrize("name", oc.GRAPH_SETS + ("six4",))
def test_emu_orbits_against_the_reference_counter(lib, name):
    oc.case_reference_rows(lib, DEV, name)


def test_emu_orbits_of_k512_need_64_bits(lib):
    oc.case_k512(lib, DEV)


def test_emu_orbit_raw_samples_and_null_outputs(lib):
    oc.case_raw_and_null(lib, DEV)


def test_emu_orbit_bad_dims(lib):
    oc.case_bad_dims(lib, DEV)


def test_emu_orbit_scores(lib):
    oc.case_scores(lib, DEV)


def test_emu_orbits_are_opt_in(lib):
    oc.case_opt_in(lib, DEV)


def test_emu_sampler_evaluate_with_orbits(lib, tmp_path):
    oc.case_sampler_evaluate(lib, tmp_path)
