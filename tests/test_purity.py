"""Host-emulation suite of the purity cases (tests/purity_cases.py): every call a pure function of its arguments -- whatever the
workspace or scratch holds on entry, nothing touched outside it or outside the outputs, rows independent of their batch, live plans
independent of each other.  The emulation runs the same kernel source and the same launch layer (carve_ws, every memset), so the
carves, the loaders' selects and the per-row indexing are the device's; its MFMA and wave-level loaders, k_gemm_h_full / k_hp_full,
the baked instances and streams are tests/test_gpu_purity.py's."""
import pytest

from tests import purity_cases as pu
from tests.emu_util import emu_library

DEV = "cpu"
# too slow here (an emulated forward at E = 190 or N = 70 is seconds, and a case runs dozens): device only, as DESIGN.md section 3 lists
DEVICE_ONLY = {"community_small_Base_CC"}
DEVICE_ONLY_BATCH = DEVICE_ONLY | {"community_small_CC", "enzymes_small_CC", "base@70"}
DEVICE_ONLY_LOOPS = {"tiled_fuse", "s4"}
EMU_ROUTES = [r for r in pu.ROUTES if r not in DEVICE_ONLY]


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_pad_geometry():
    pu.case_pad_geometry()


@pytest.mark.parametrize("route", EMU_ROUTES)
def test_workspace(lib, route):
    pu.case_workspace(pu.ROUTES[route], lib, DEV)


@pytest.mark.parametrize("form", [f for f in pu.LOOP_ROUTES if f not in DEVICE_ONLY_LOOPS])
def test_workspace_loops(lib, form):
    pu.case_workspace(pu.LOOP_ROUTES[form], lib, DEV)


@pytest.mark.parametrize("name", pu.OP_NAMES)
def test_scratch_of_operations(lib, name):
    pu.case_op(name, lib, DEV)


@pytest.mark.parametrize("route", [r for r in pu.ROUTES if r not in DEVICE_ONLY_BATCH])
def test_batch_independence(lib, route):
    pu.case_batch(pu.ROUTES[route], lib, DEV)


def test_plans_interleaved(lib):
    pu.case_interleaved(lib, DEV)


def test_plan_buffer_growth(lib):
    pu.case_growth(lib, DEV)
