"""GPU suite (-m gpu) for the tiled graph-network route (graph-only plans above 64 nodes; ccsd_amd/csrc/ccsd_k_lg.h) on the MI355X."""
import pytest
import torch

from tests import large_graph_cases as lc
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


def test_forward_enzymes_vs_reference_golden(lib):
    pc.case_forward_vs_reference_golden("gdss_enzymes", lib, DEV)


def test_forward_enzymes_vs_oracle_b8(lib):
    meta, parts = load_ckpt_np("gdss_enzymes")
    lc.case_forward_vs_oracle_src(meta, parts, lib, DEV, [125, 1, 0, 64, 125, 17, 100, 33], "gdss_enzymes B=8")


def test_forward_grid_vs_oracle(lib):
    meta, parts = load_ckpt_np("gdss_grid")
    lc.case_forward_vs_oracle_src(meta, parts, lib, DEV, [361, 144], "gdss_grid B=2")


@pytest.mark.parametrize("N,counts", [(67, [67, 1, 0]), (97, [97, 50, 1])])
def test_forward_random_weights(lib, N, counts):
    meta, parts = lc.resized("gdss_community_small", N, seed=N)
    lc.case_forward_vs_oracle_src(meta, parts, lib, DEV, counts, f"N={N}")


@pytest.mark.parametrize("gname", ["gdss_enzymes", "gdss_grid"])
def test_sampler_vs_reference_golden(lib, gname):
    lc.case_sampler_vs_golden(gname, "n1000_first3", lib, DEV)


def test_production_loop_enzymes_b64(lib):
    counts = [125, 100, 64, 37, 12, 1, 90, 77]
    pc.case_production_loop_vs_oracle("gdss_enzymes", lib, DEV, 64, counts, 3, "S4", "None", 0.15, 0.7,
                                      expect_route={"large_graph": 1})


def test_production_loop_grid_b8(lib):
    pc.case_production_loop_vs_oracle("gdss_grid", lib, DEV, 8, [361, 144, 256, 100, 324, 64, 361, 196], 2, "Reverse", "Langevin", 0.1,
                                      0.7, expect_route={"large_graph": 1})


@pytest.mark.parametrize("name,counts", [("gdss_community_small", [20, 11, 1, 0]), ("gdss_zinc250k", [38, 23, 1, 0])])
def test_forced_route_vs_k_xa(lib, monkeypatch, name, counts):
    lc.case_forced_vs_xa(name, lib, DEV, 4, counts, monkeypatch=monkeypatch)


def test_ccsd_enzymes_yaml_run(lib, tmp_path):
    lc.case_enzymes_yaml_run(lib, tmp_path)
