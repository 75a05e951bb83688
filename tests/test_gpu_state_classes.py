"""GPU suite of the input classes (tests/state_class_cases.py): flags with holes, unmasked states and a non-zero adjacency diagonal on
the device forms the emulation does not have -- the MFMA and wave-level forms of the mask products, the baked instances, and
k_gemm_h_full / k_hp_full (selected from B = 256)."""
import pytest
import torch

from ccsd_amd import _lib
from tests import noise_cases as nc
from tests import state_class_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.get_library()


def test_forward_qm9_instances(lib):
    sc.case_forward_qm9_instances(lib, DEV)


@pytest.mark.parametrize("name", list(sc.CHECKPOINTS))
def test_forward_checkpoint(lib, name):
    sc.case_forward_checkpoint(name, lib, DEV)


def test_forward_ew1(lib):
    sc.case_forward_ew1(lib, DEV)


def test_forward_hodge_general(lib):
    sc.case_forward_hodge_general(lib, DEV)


def test_forward_hodge_wide(lib):
    sc.case_forward_hodge_wide(lib, DEV)


@pytest.mark.parametrize("name", list(sc.FORCED))
def test_forward_forced_tiled_route(lib, name):
    sc.case_forward_forced_tiled(name, lib, DEV)


def test_forward_tiled_route_n70(lib):
    sc.case_forward_n70(lib, DEV)


@pytest.mark.parametrize("N", [33, 64])
def test_forward_word_edge_graph(lib, N):
    sc.case_forward_word_edge_graph(N, lib, DEV)


def test_forward_word_edge_complex(lib):
    sc.case_forward_word_edge_complex(33, lib, DEV)


@pytest.mark.parametrize("cls", ["H", "HU"])
@pytest.mark.parametrize("name", list(sc.STEP_PLANS))
def test_step_calls(lib, name, cls):
    sc.case_step_calls(name, cls, lib, DEV)


@pytest.mark.parametrize("form", list(sc.LOOPS))
def test_production_loop_holes(lib, form):
    sc.case_production_loop(form, lib, DEV)


def test_one_step_holes(lib):
    sc.case_one_step_holes("ccsd_qm9_CC", lib, DEV, "Reverse", "Langevin", 0.2, 0.7)
    sc.case_one_step_holes("gdss_community_small", lib, DEV, "Euler", "Langevin", 0.05, 0.7)


def test_full_kernels_b256_holes(lib):
    sc.case_full_kernels_b256(lib, DEV)


@pytest.mark.parametrize("plan", list(sc.NOISE_SLOTS))
def test_noise_holes(lib, plan):
    sc.case_noise(plan, lib, DEV, nc.BOUND_GPU)


def test_complex_masks_n64(lib):
    """The complex plan at N = 64, node 63 off and on: device only (E = 2016, K = 41664)."""
    sc.case_complex_masks(64, (3, 3), lib, DEV)


def test_complex_masks_small_twin(lib):
    sc.case_complex_masks(12, (3, 4), lib, DEV)
