"""GPU suite (-m gpu) of the node-count sweep of the tiled graph-network route above 64 nodes (tests/lg_node_sweep_cases.py) on the
MI355X: the forwards of three families at 23 node counts from 65 to the ceiling 512 against the float64 oracle, the library loop at
N = 128, 256 and 512, the planner's ceiling and one N = 512 forward with the workspace between guards."""
import pytest

from tests import lg_node_sweep_cases as lg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


def test_guarded_forward_at_the_ceiling(lib):
    """(first: the plan's very first launches run between the guards)"""
    lg.case_guarded_ceiling(lib, DEV)


def test_planner_ceiling(lib):
    lg.case_planner_ceiling(lib, DEV)


@pytest.mark.parametrize("group", list(lg.GROUPS))
@pytest.mark.parametrize("family", list(lg.FAMILIES))
def test_forward_group(lib, family, group):
    lg.case_group(family, lg.GROUPS[group], lib, DEV)


@pytest.mark.parametrize("loop", sorted(lg.LOOPS))
@pytest.mark.parametrize("N", lg.LOOP_NODES)
def test_production_loop(lib, N, loop):
    lg.case_loop(N, loop, lib, DEV)
