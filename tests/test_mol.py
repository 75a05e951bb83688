"""CPU suite for molecule post-processing (ccsd_mol_correct, SampleOps.mol_correct, evaluation.MOL_TABLES, Sampler.molecules,
Sampler.evaluate(correct=True)) over the host emulation of k_mol_correct: every output exact against the plain Python restatement of
tests/mol_ref.py on the handcrafted, random and boundary cases of tests/mol_cases.py, the properties every output has, the call as a pure
function of its arguments, the invalid arguments, and the two Sampler methods through fake finished results."""
import pytest

from ccsd_amd import evaluation as ev
from tests import mol_cases as mc


@pytest.fixture(scope="module")
def lib():
    from tests.emu_util import emu_library

    return emu_library()


def test_generator_produces_what_it_promises():
    mc.check_generator()


def test_tables():
    q, z = ev.MOL_TABLES["QM9"], ev.MOL_TABLES["ZINC250k"]
    assert q["atomic_num_list"] == [6, 7, 8, 9] and z["atomic_num_list"] == [6, 7, 8, 9, 15, 16, 17, 35, 53]
    assert [m[0] for m in z["max_valence"]] == [4, 3, 2, 1, 7, 6, 1, 1, 5] and z["max_valence"][1][1] == 4 and z["max_valence"][2][1] == 3
    assert z["charge_base"] == [0, 3, 2, 0, 0, 2, 0, 0, 0] and q["charge_base"] == z["charge_base"][:4] and q["max_valence"] == z["max_valence"][:4]
    assert "NOBODY HAS CHECKED THESE MAXIMA AGAINST RDKIT" in open(ev.__file__).read()


@pytest.mark.parametrize("largest_fragment", [True, False])
@pytest.mark.parametrize("name", ["hand"] + [n for n in mc.CASES if n != "N64_B257"])
def test_emu_exact(lib, name, largest_fragment):
    mc.case_exact(lib, "cpu", name, largest_fragment)


def test_emu_exact_largest_batch(lib):
    mc.case_exact(lib, "cpu", "N64_B257", True)


def test_emu_pure(lib):
    mc.case_pure(lib, "cpu")
    mc.case_pure(lib, "cpu", "N63")


def test_emu_invalid(lib):
    mc.case_invalid(lib, "cpu")


def test_emu_sampler_molecules_and_evaluate(lib):
    mc.case_sampler(lib, "cpu")
