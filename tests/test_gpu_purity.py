"""GPU suite of the purity cases (tests/purity_cases.py) on what the emulation does not have: the MFMA and wave-level loaders, the
baked instances, k_gemm_h_full / k_hp_full (selected from B = 256), and streams -- two plans on two streams at once, and every call
on a side stream behind a sleep, which a launch, memset or copy issued on another stream would overtake."""
import pytest
import torch

from ccsd_amd import _lib
from tests import purity_cases as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.get_library()


def test_pad_geometry():
    pu.case_pad_geometry()


@pytest.mark.parametrize("route", list(pu.ROUTES))
def test_workspace(lib, route):
    pu.case_workspace(pu.ROUTES[route], lib, DEV)


def test_workspace_full_kernels_b256(lib):
    pu.case_workspace(pu.ROUTE_B256, lib, DEV)


@pytest.mark.parametrize("form", list(pu.LOOP_ROUTES))
def test_workspace_loops(lib, form):
    pu.case_workspace(pu.LOOP_ROUTES[form], lib, DEV)


@pytest.mark.parametrize("name", pu.OP_NAMES)
def test_scratch_of_operations(lib, name):
    pu.case_op(name, lib, DEV)


@pytest.mark.parametrize("route", list(pu.ROUTES))
def test_batch_independence(lib, route):
    pu.case_batch(pu.ROUTES[route], lib, DEV)


def test_plans_interleaved(lib):
    pu.case_interleaved(lib, DEV)


def test_plan_buffer_growth(lib):
    pu.case_growth(lib, DEV)


def test_two_plans_on_two_streams(lib):
    pu.case_two_streams(lib, DEV)


def test_stream_harness_tells_a_null_stream_launch():
    pu.case_stream_harness(DEV)


@pytest.mark.parametrize("route", pu.STREAM_ROUTES)
def test_stream_of_units(lib, route):
    pu.case_stream_unit(pu.ROUTES[route], lib, DEV)


@pytest.mark.parametrize("form", list(pu.LOOP_ROUTES))
def test_stream_of_loops(lib, form):
    pu.case_stream_unit(pu.LOOP_ROUTES[form], lib, DEV)


@pytest.mark.parametrize("name", pu.OP_NAMES)
def test_stream_of_operations(lib, name):
    pu.case_stream_op(name, lib, DEV)


def test_stream_of_init_state(lib):
    pu.case_stream_init_state(lib, DEV)
