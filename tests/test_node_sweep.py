"""CPU suite of the node-count sweep (tests/node_sweep_cases.py) on the host emulation, at a bounded list of node counts: the
planner and the LDS carve-up of k_xa are host code and run here as they do on the device; the tile fragment indexing and the
ragged last tile exist only in the device branch (GPU suite, the full sweep: tests/test_gpu_node_sweep.py)."""
import pytest
import torch

from tests import node_sweep_cases as ns
from tests.emu_util import emu_library

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def _bounded(arch, band):
    return [N for N in ns.bounded_nodes(arch) if N in ns.BANDS[band]]


# ---- A
@pytest.mark.parametrize("arch,band,hint", ns.BAND_PARAMS)
def test_emu_graph_band(lib, arch, band, hint):
    ns.case_band(arch, _bounded(arch, band), hint, lib, DEV)


@pytest.mark.parametrize("arch", ns.ARCHS)
def test_planner_coverage(lib, arch):
    ns.case_coverage(arch, lib, DEV, bands=[ns.NODES])         # (the planner's table holds every N; the GPU suite runs them all)
    assert {ns.LAST_XA[arch], ns.LAST_XA[arch] + 1} <= set(ns.bounded_nodes(arch))


def test_emu_variant4_other_architectures(lib):
    ns.case_variant4_other_architectures(lib, DEV)


# ---- B
@pytest.mark.parametrize("N", range(3, 18))
def test_emu_cc_forwards(lib, N):
    ns.case_cc_forwards(N, lib, DEV)


@pytest.mark.parametrize("loop", sorted(ns.CC_LOOPS))
@pytest.mark.parametrize("N", ns.CC_LOOP_NODES)
def test_emu_cc_production_loop(lib, N, loop):
    ns.case_cc_loop(N, loop, lib, DEV)


# ---- C
@pytest.mark.parametrize("N", sorted(ns.ZINC5B_ROUTE))
def test_emu_zinc5b_production_loop(lib, N):
    ns.case_zinc5b_loop(N, lib, DEV)


# ---- D
@pytest.mark.parametrize("loop", sorted(ns.XA_LOOPS))
@pytest.mark.parametrize("arch,N", ns.XA_LOOP_SHAPES_BOUNDED)
def test_emu_xa_production_loop(lib, arch, N, loop):
    ns.case_xa_loop(arch, N, loop, lib, DEV)
