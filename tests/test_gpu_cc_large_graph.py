"""GPU suite (-m gpu) for the tiled graph-network route of one-hodge-layer combinatorial complexes (k_lg_hodge1;
ccsd_amd/csrc/ccsd_k_lg.h) on the MI355X: the cases of the CPU suite, the rank-2 kernels beyond E = 703, and ccsd_grid_small_CC at
its own geometry (N = 49, E = 1176, K = 18424)."""
import pytest

from tests import cc_large_graph_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


def test_forced_route_community_small_cc(lib, monkeypatch):
    cc.case_forced_vs_xa("ccsd_community_small_CC", lib, DEV, [20, 11, 2], ["x", "adj", "rank2"], monkeypatch)


def test_forced_route_zinc5b(lib, monkeypatch):
    cc.case_forced_vs_xa("zinc250k_CC_5b", lib, DEV, [38, 9], ["adj", "x"], monkeypatch)


def test_planner_crossover(lib, monkeypatch):
    cc.case_crossover_selection(lib, DEV, monkeypatch)


def test_crossover_forwards(lib):
    cc.case_crossover_forwards(lib, DEV)


def test_crossover_rank2_e903(lib):
    cc.case_crossover_rank2(lib, DEV)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_forced_production_loop(lib, monkeypatch, predictor, corrector, snr, seps):
    cc.case_forced_production_loop(lib, DEV, predictor, corrector, snr, seps, monkeypatch)


def test_forced_nsteps2_library_vs_stepwise(lib, monkeypatch):
    cc.case_forced_nsteps2(lib, DEV, monkeypatch)


def test_grid_small_cc_forwards_vs_reference_golden(lib):
    cc.case_grid_forwards(lib, DEV)


def test_grid_small_cc_sampler_vs_reference_golden(lib):
    cc.case_grid_sampler_vs_golden(lib, DEV)


def test_grid_small_cc_production_loop(lib):
    cc.case_grid_production_loop(lib, DEV)


def test_ccsd_grid_small_cc_yaml_run(lib, tmp_path):
    cc.case_grid_yaml_run(lib, tmp_path)
