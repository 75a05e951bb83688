"""GPU suite (-m gpu) for ScoreNetworkA_CC hodge branches up to 8 channels / hodge MLPs up to 16 wide on the MI355X: the cases of the CPU
suite on the kernels themselves (k_lg_hodge1_w, k_lg_hd_diag_w, k_gemm_p_w, k_hodge_value_w), and the yaml surface."""
import pytest

from tests import hodge_wide_cases as hw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("tag", hw.WIDE)
def test_kat_hodge_wide(lib, monkeypatch, tag):
    hw.case_kat(tag, lib, DEV, monkeypatch)


def test_kat_single_linear_k_xa_and_route(lib, monkeypatch):
    hw.case_kat_single(lib, DEV, monkeypatch)


def test_edge_flags(lib, monkeypatch):
    hw.case_edge_flags(lib, DEV, monkeypatch)


def test_enzymes_wide_forwards(lib, monkeypatch):
    hw.case_enz_forwards(lib, DEV, monkeypatch)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_production_loop(lib, monkeypatch, predictor, corrector, snr, seps):
    hw.case_production_loop(lib, DEV, predictor, corrector, snr, seps, monkeypatch)


def test_nsteps2_library_vs_stepwise(lib, monkeypatch):
    hw.case_nsteps2(lib, DEV, monkeypatch)


def test_planner_envelope(lib, monkeypatch):
    hw.case_planner(lib, DEV, monkeypatch)


def test_qm9_wide_yaml_run(lib, tmp_path):
    hw.case_yaml_run(lib, tmp_path)
