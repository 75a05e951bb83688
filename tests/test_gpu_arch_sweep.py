"""GPU suite (-m gpu) of the architecture sweep (tests/arch_sweep_cases.py) on the MI355X: the graph-only architectures at N = 9,
at k_xa's 152 KB layouts (N = 40) and on the tiled route (N = 70) in bands of plans, the ScoreNetworkX_GMH and conv = "MLP"
variants, ScoreNetworkF 9 to 32 wide on the fused k_r2 and on the tiled family, one step of the production loop behind four of
these MLP forms, the planner's envelope, and six architectures against the reference constructors' outputs."""
import pytest

from tests import arch_sweep_cases as asw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWEPT = asw.GRAPH + asw.GRAPH_40 + asw.GRAPH_70 + asw.SINGLE + asw.FNET + asw.FNET_GPU         # (test_envelope runs asw.FNET_EDGE)


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


# ---- A
@pytest.mark.parametrize("band", asw.GRAPH_BANDS)
def test_graph_band(lib, band):
    for case in asw.GRAPH_BANDS[band]:
        asw.case_graph(case, lib, DEV)


def test_route_refuses(lib):
    asw.case_route_refuses(lib, DEV)


# ---- B
def test_gmh_mlpconv(lib):
    for case in asw.SINGLE:
        asw.case_single(case, lib, DEV)


# ---- C
@pytest.mark.parametrize("band", asw.FNET_BANDS)
def test_fnet_band(lib, band, monkeypatch):
    for case in asw.FNET_BANDS[band]:
        asw.case_fnet(case, lib, DEV, monkeypatch)


# ---- D
@pytest.mark.parametrize("key", asw.LOOPS)
def test_production_loop(lib, key):
    asw.case_loop(key, lib, DEV)


# ---- E (runs after the sweep of this file: the plans it recorded)
def test_route_final_mlp(lib, monkeypatch):
    assert asw.forms(asw.case_route_final_mlp(lib, DEV, monkeypatch))[1] == 7


def test_coverage():
    asw.case_coverage([c.name for c in SWEPT])


# ---- F
@pytest.mark.parametrize("limit", asw.ENVELOPE)
def test_envelope(lib, limit, monkeypatch):
    asw.case_envelope(limit, lib, DEV, monkeypatch)


# ---- G
@pytest.mark.parametrize("tag", asw.KAT)
def test_kat(lib, tag):
    asw.case_kat_engine(tag, lib, DEV)
