"""CPU suite for ScoreNetworkA_CC hodge branches up to 8 channels / hodge MLPs up to 16 wide: the fixture against the oracle, the planner,
and the host emulation of the wide kernels (tiled graph-network route, tiled rank-2 family) against the reference and the oracle."""
import pytest
import torch

from tests import hodge_wide_cases as hw
from tests.emu_util import emu_library

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


@pytest.mark.parametrize("tag", hw.TAGS)
def test_oracle_vs_reference(tag):
    hw.case_oracle_vs_reference(tag)


@pytest.mark.parametrize("tag", hw.WIDE)
def test_emu_kat_hodge_wide(lib, monkeypatch, tag):
    hw.case_kat(tag, lib, DEV, monkeypatch)


def test_emu_kat_single_linear_k_xa_and_route(lib, monkeypatch):
    hw.case_kat_single(lib, DEV, monkeypatch)


def test_emu_edge_flags(lib, monkeypatch):
    hw.case_edge_flags(lib, DEV, monkeypatch)


def test_emu_enzymes_wide_forwards(lib, monkeypatch):
    hw.case_enz_forwards(lib, DEV, monkeypatch)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_emu_production_loop(lib, monkeypatch, predictor, corrector, snr, seps):
    hw.case_production_loop(lib, DEV, predictor, corrector, snr, seps, monkeypatch)


def test_emu_nsteps2_library_vs_stepwise(lib, monkeypatch):
    hw.case_nsteps2(lib, DEV, monkeypatch)


def test_planner_envelope(lib, monkeypatch):
    hw.case_planner(lib, DEV, monkeypatch)
