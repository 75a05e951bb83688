"""CPU suite of the architecture sweep (tests/arch_sweep_cases.py): the conditions on every case's inputs, on the oracle alone, and
the sweep on the host emulation (the tiled route at a bounded list of architectures) -- the planner, the packing and the LDS
carve-up are host code and run here as they do on the device; the MFMA fragment indexing, the ragged last tile of a padded width
and the packed-weight reads exist only in the device branch (GPU suite: tests/test_gpu_arch_sweep.py, which also runs the
ScoreNetworkF cases too slow for the emulation)."""
import pytest
import torch

from tests import arch_sweep_cases as asw
from tests.emu_util import emu_library

torch.set_num_threads(8)
DEV = "cpu"
EVERY = asw.GRAPH + asw.GRAPH_40 + asw.GRAPH_70 + asw.SINGLE + asw.FNET + asw.FNET_GPU + asw.FNET_EDGE
SWEPT = asw.GRAPH + asw.GRAPH_40 + asw.GRAPH_70_BOUNDED + asw.SINGLE + asw.FNET + asw.FNET_EDGE


@pytest.fixture(scope="module")
def lib():
    return emu_library()


# ---- the inputs: (a) the oracle's outputs lie in [1e-2, 1e2]; (b) the last unit of the layer a case is about moves them; (c) the
# float32 oracle lies well within the tolerance of its float64 evaluation
@pytest.mark.parametrize("case", EVERY, ids=lambda c: c.name)
def test_input_conditions(case):
    asw.case_conditions(case)


# ---- A
@pytest.mark.parametrize("band", asw.GRAPH_BANDS_BOUNDED)
def test_emu_graph_band(lib, band):
    for case in asw.GRAPH_BANDS_BOUNDED[band]:
        asw.case_graph(case, lib, DEV)


def test_emu_route_refuses(lib):
    asw.case_route_refuses(lib, DEV)


# ---- B
@pytest.mark.parametrize("case", asw.SINGLE, ids=lambda c: c.name)
def test_emu_gmh_mlpconv(lib, case):
    asw.case_single(case, lib, DEV)


# ---- C
@pytest.mark.parametrize("case", asw.FNET + asw.FNET_EDGE, ids=lambda c: c.name)
def test_emu_fnet(lib, case, monkeypatch):
    asw.case_fnet(case, lib, DEV, monkeypatch)


# ---- D
@pytest.mark.parametrize("key", asw.LOOPS)
def test_emu_production_loop(lib, key):
    asw.case_loop(key, lib, DEV)


# ---- E (runs after the sweep of this file: the plans it recorded)
def test_emu_route_final_mlp(lib, monkeypatch):
    assert asw.forms(asw.case_route_final_mlp(lib, DEV, monkeypatch))[1] == 7


def test_coverage():
    asw.case_coverage([c.name for c in SWEPT])


# ---- F
@pytest.mark.parametrize("limit", asw.ENVELOPE)
def test_emu_envelope(lib, limit, monkeypatch):
    asw.case_envelope(limit, lib, DEV, monkeypatch, run=False)


# ---- G
def test_kat_params():
    asw.case_kat_params()


@pytest.mark.parametrize("tag", asw.KAT)
def test_emu_kat(lib, tag):
    asw.case_kat_engine(tag, lib, DEV)
