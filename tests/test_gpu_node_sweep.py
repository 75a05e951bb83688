"""GPU suite (-m gpu) of the node-count sweep (tests/node_sweep_cases.py) on the MI355X: every node count 2..64 for four graph-only
architectures at two batch hints, the grid_small_CC architecture on k_xa and the small rank-2 geometries, the element-wise rank-2
family at d = 3..4, and the production loop at the last node counts k_xa serves."""
import pytest

from tests import node_sweep_cases as ns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


# ---- A
@pytest.mark.parametrize("arch,band,hint", ns.BAND_PARAMS)
def test_graph_band(lib, arch, band, hint):
    ns.case_band(arch, ns.BANDS[band], hint, lib, DEV)


@pytest.mark.parametrize("arch", ns.ARCHS)
def test_coverage(lib, arch, capsys):
    """Runs after the bands of the file: the routes they recorded, against the planner's table and the coverage the sweep is for."""
    text = ns.case_coverage(arch, lib, DEV)
    with capsys.disabled():
        print("\n" + text)


def test_variant4_other_architectures(lib):
    ns.case_variant4_other_architectures(lib, DEV)


# ---- B
@pytest.mark.parametrize("N", ns.CC_FORWARD_NODES)
def test_cc_forwards(lib, N):
    ns.case_cc_forwards(N, lib, DEV)


@pytest.mark.parametrize("N", ns.CC_XA_NODES)
def test_cc_forwards_x_adj(lib, N):
    ns.case_cc_forwards(N, lib, DEV, targets=("x", "adj"))


@pytest.mark.parametrize("loop", sorted(ns.CC_LOOPS))
@pytest.mark.parametrize("N", ns.CC_LOOP_NODES)
def test_cc_production_loop(lib, N, loop):
    ns.case_cc_loop(N, loop, lib, DEV)


# ---- C
@pytest.mark.parametrize("N", sorted(ns.ZINC5B_ROUTE))
def test_zinc5b_production_loop(lib, N):
    ns.case_zinc5b_loop(N, lib, DEV)


# ---- D
@pytest.mark.parametrize("loop", sorted(ns.XA_LOOPS))
@pytest.mark.parametrize("arch,N", ns.XA_LOOP_SHAPES)
def test_xa_production_loop(lib, arch, N, loop):
    ns.case_xa_loop(arch, N, loop, lib, DEV)
