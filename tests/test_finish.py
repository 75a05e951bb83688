"""CPU suite for the one-pass finish of a sampling run (ccsd_finish, PCEngine.finish) over the host emulation of k_finish_rank2 /
k_finish_graph: bitwise against ccsd_quantize / ccsd_rank2_cells, the descriptors against a numpy restatement and against the
reference's own functions on the reference's samples (tests/golden/f1_finish.npz), null outputs and host-side validation."""
import pytest

from tests import finish_cases as fc
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


@pytest.mark.parametrize("name", list(fc.GEOMETRIES))
def test_emu_bitwise_against_existing_entry_points(lib, name):
    fc.case_bitwise(lib, DEV, name)


@pytest.mark.parametrize("name", list(fc.GEOMETRIES))
def test_emu_descriptors_against_numpy(lib, name):
    fc.case_descriptors(lib, DEV, name)


@pytest.mark.parametrize("name,case", fc.f1_cases())
def test_emu_descriptors_against_reference_fixture(lib, name, case):
    fc.case_reference_fixture(lib, DEV, name, case)


def test_emu_null_outputs(lib):
    fc.case_null_outputs(lib, DEV)


def test_emu_bad_dims(lib):
    fc.case_bad_dims(lib, DEV)


def test_emu_sample_ops_need_no_plan(lib, monkeypatch):
    fc.case_no_plan(lib, DEV, monkeypatch)


def test_emu_sample_builds_no_plan_for_the_finish(lib, tmp_path):
    fc.case_sample_builds_no_plan_for_the_finish(lib, tmp_path)


def test_special_values_straddle_every_threshold():
    sp = fc.special_values()
    assert len(sp) == 11 and (sp[:2] == 0).all() and bool(fc.np.signbit(sp[0]))
    for i, t in enumerate((0.5, 1.5, 2.5)):
        lo, at, hi = sp[2 + 3 * i: 5 + 3 * i]
        assert lo < at == fc.np.float32(t) < hi
