"""CPU suite for the tiled graph-network route of ScoreNetworkA_CC stacks of two or more hodge layers (k_lg_hd_*;
ccsd_amd/csrc/ccsd_k_lg.h): the planner, and the host emulation of the route against the oracle, k_xa and the reference goldens."""
import pytest
import torch

from tests import hodge_stack_route_cases as hs
from tests.emu_util import emu_library

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_emu_forced_route_qm9_cc(lib, monkeypatch):
    """Fused rank-2 family, raw P_1, single-Linear mlp_value: E = 36, two full tiles + 4; a full, a partial, a two-node complex."""
    hs.case_forced_vs_xa(hs.QM9, lib, DEV, [9, 5, 2], monkeypatch)


def test_emu_forced_route_enzymes_small_cc(lib, monkeypatch):
    """Tiled rank-2 family, num_linears_h = 2: E = 66, four tiles + 2."""
    hs.case_forced_vs_xa(hs.ENZ, lib, DEV, [12, 7, 2], monkeypatch)


@pytest.mark.parametrize("name", [hs.QM9, hs.ENZ])
def test_emu_forced_route_vs_reference_golden(lib, monkeypatch, name):
    hs.case_forced_vs_golden(name, lib, DEV, monkeypatch)


def test_planner_selection(lib, monkeypatch):
    hs.case_selection(lib, DEV, monkeypatch)


@pytest.mark.parametrize("ckpt,N", [(hs.GRID, 17), (hs.GRID, 24), (hs.ENZ, 14)])
def test_emu_natural_forwards(lib, monkeypatch, ckpt, N):
    hs.case_natural_forwards(ckpt, N, [N, 9], lib, DEV, monkeypatch)


@pytest.mark.parametrize("tag", hs.KAT_LAYERS)
def test_emu_kat_hodge_layers_on_the_route(lib, monkeypatch, tag):
    hs.case_kat("kat_hodge_layers.npz", tag, lib, DEV, monkeypatch)


@pytest.mark.parametrize("tag", hs.KAT_GENERAL)
def test_emu_kat_hodge_general_on_the_route(lib, monkeypatch, tag):
    hs.case_kat("kat_hodge_general.npz", tag, lib, DEV, monkeypatch)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_emu_forced_production_loop_enzymes(lib, monkeypatch, predictor, corrector, snr, seps):
    hs.case_production_loop(hs.ENZ, (12, 7), lib, DEV, predictor, corrector, snr, seps, monkeypatch)


def test_emu_forced_production_loop_qm9(lib, monkeypatch):
    hs.case_production_loop(hs.QM9, (9, 5), lib, DEV, "Reverse", "Langevin", 0.1, 0.7, monkeypatch)


def test_emu_forced_nsteps2_library_vs_stepwise(lib, monkeypatch):
    hs.case_nsteps2(lib, DEV, monkeypatch)


def test_planner_envelope(lib, monkeypatch):
    hs.case_planner(lib, DEV, monkeypatch)
