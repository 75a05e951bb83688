"""CPU suite of the node-count sweep of the tiled graph-network route above 64 nodes (tests/lg_node_sweep_cases.py) on the host
emulation, at the node counts whose tests take no longer than the slowest emulated test of the route before it (DESIGN.md section 3
states the times); the planner and the workspace carve are host code and run here at the ceiling as they do on the device.  The full
list, the ceiling's forwards and loops: tests/test_gpu_lg_node_sweep.py."""
import pytest
import torch

from tests import lg_node_sweep_cases as lg
from tests.emu_util import emu_library

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_lists():
    assert set(lg.EMU_NODES) <= set(lg.NODES) and set(lg.LOOP_EMU_NODES) <= set(lg.LOOP_NODES) and max(lg.NODES) == lg.MAXN
    for N in lg.NODES:
        f = lg.sweep_flags(N)
        assert f.sum(1).tolist() == [N, N - 1, N // 2 + 1, 1, 0, N - 8]


def test_planner_ceiling(lib):
    lg.case_planner_ceiling(lib, DEV)


@pytest.mark.parametrize("N", lg.EMU_NODES)
@pytest.mark.parametrize("family", list(lg.FAMILIES))
def test_emu_forward(lib, family, N):
    lg.case_group(family, (N,), lib, DEV)


@pytest.mark.parametrize("loop", sorted(lg.LOOPS))
@pytest.mark.parametrize("N", lg.LOOP_EMU_NODES)
def test_emu_production_loop(lib, N, loop):
    lg.case_loop(N, loop, lib, DEV)
