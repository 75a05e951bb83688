"""GPU suite (-m gpu) for ScoreNetworkA_Base_CC on the tiled graph-network route (k_lg_hb_*; ccsd_amd/csrc/ccsd_k_lg.h) on the
MI355X: the cases of the CPU suite, the three-layer architecture at ego_small_Base_CC.yaml's own geometry (N = 18, E = 153) and at
E = 496 = 31 x 16 (no ragged tile), and the grid_small_Base_CC architecture at N = 49 (E = 1176, K = 18424)."""
import pytest

from tests import base_cc_route_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


def test_planner(lib, monkeypatch):
    bc.case_planner(lib, DEV, monkeypatch)


@pytest.mark.parametrize("name,counts", [("ccsd_community_small_Base_CC", [20, 11, 2]), ("ccsd_qm9_Base_CC", [9, 5, 2])])
def test_forced_route_vs_xa(lib, monkeypatch, name, counts):
    bc.case_forced_vs_xa(name, lib, DEV, counts, monkeypatch)


def test_forced_route_enzymes_small_base_cc_ineligible(lib, monkeypatch):
    bc.case_forced_ineligible(lib, DEV, monkeypatch)


@pytest.mark.parametrize("ckpt,gname", [(bc.EGO7, bc.EGO7_GOLDEN), (bc.EGO12, bc.EGO12_GOLDEN)])
def test_three_layers_forwards_vs_reference_golden(lib, ckpt, gname):
    bc.case_forwards_vs_golden(ckpt, gname, lib, DEV)


def test_three_layers_sampler_vs_reference_golden(lib):
    bc.case_sampler_vs_golden(lib, DEV)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_three_layers_production_loop(lib, predictor, corrector, snr, seps):
    bc.case_production_loop(lib, DEV, predictor, corrector, snr, seps)


def test_three_layers_nsteps2_library_vs_stepwise(lib):
    bc.case_nsteps2(lib, DEV)


def test_three_layers_n18_adj_vs_oracle(lib):
    bc.case_adj_vs_oracle(18, 5, (18, 11, 2), lib, DEV)


def test_three_layers_n32_e496_adj_vs_oracle(lib):
    bc.case_adj_vs_oracle(32, 3, (32, 19), lib, DEV)


def test_grid_small_base_cc_forwards_vs_reference_golden(lib):
    bc.case_forwards_vs_golden(bc.GRID, bc.GRID_GOLDEN, lib, DEV, score=True)


def test_grid_small_base_cc_library_vs_stepwise(lib):
    bc.case_grid_library_vs_stepwise(lib, DEV)


def test_grid_small_base_cc_yaml_run(lib, tmp_path):
    bc.case_grid_yaml_run(lib, tmp_path)
