"""Host-emulation suite of the folded batch norm sums (tests/sum_fold_cases.py).  The emulation runs the workgroups of a launch one
after the other, so a merged k_r2 launch that wrote the next step's partials into the buffer it reduces would be caught here at any
batch above one: workgroup b would reduce the new partials of workgroups 0 .. b - 1."""
import pytest

from tests import sum_fold_cases as sf
from tests.emu_util import emu_library

DEV = "cpu"
# both parities of the two partial buffers, and a call that starts mid-schedule
RANGES = [(0, 5), (0, 6), (3, 8)]


@pytest.fixture(scope="module")
def lib():
    return emu_library()


@pytest.mark.parametrize("B", [3, 5])
def test_fold_equals_normsum_launches(lib, B):
    sf.case_on_off(sf.QM9, lib, DEV, B, RANGES)


def test_fold_equals_normsum_launches_with_trajectory(lib):
    sf.case_on_off(sf.QM9, lib, DEV, 3, [(0, 5), (3, 8)], traj=True)


def test_reduce_hook_keeps_normsum(lib):
    sf.case_reduce_hook_keeps_normsum(sf.QM9, lib, DEV, 3, 0, 5)


def test_route(lib):
    sf.case_route(lib, DEV)
