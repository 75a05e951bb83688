"""CPU suite for ScoreNetworkA_Base_CC on the tiled graph-network route (k_lg_hb_*; ccsd_amd/csrc/ccsd_k_lg.h): the planner, the
host emulation of the route against the reference goldens, the oracle and k_xa, and the oracle against the new goldens.  (The grid
architecture's forwards at N = 49 and the sizes between, N = 18 and N = 32, run in the GPU suite: the dense E x E layers take
minutes on the emulation there.)"""
import numpy as np
import pytest
import torch

from oracle import ccsd_oracle as O
from tests import base_cc_route_cases as bc
from tests import test_oracle_golden as OG
from tests.emu_util import emu_library
from tests.helpers import load_golden, rng_matches

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_planner(lib, monkeypatch):
    bc.case_planner(lib, DEV, monkeypatch)


@pytest.mark.parametrize("name,counts", [("ccsd_community_small_Base_CC", [20, 11, 2]), ("ccsd_qm9_Base_CC", [9, 5, 2])])
def test_emu_forced_route_vs_xa(lib, monkeypatch, name, counts):
    bc.case_forced_vs_xa(name, lib, DEV, counts, monkeypatch)


def test_forced_route_enzymes_small_base_cc_ineligible(lib, monkeypatch):
    bc.case_forced_ineligible(lib, DEV, monkeypatch)


@pytest.mark.parametrize("ckpt,gname", [(bc.EGO7, bc.EGO7_GOLDEN), (bc.EGO12, bc.EGO12_GOLDEN)])
def test_emu_three_layers_forwards_vs_reference_golden(lib, ckpt, gname):
    bc.case_forwards_vs_golden(ckpt, gname, lib, DEV)


def test_emu_three_layers_sampler_vs_reference_golden(lib):
    bc.case_sampler_vs_golden(lib, DEV)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_emu_three_layers_production_loop(lib, predictor, corrector, snr, seps):
    bc.case_production_loop(lib, DEV, predictor, corrector, snr, seps)


def test_emu_three_layers_nsteps2_library_vs_stepwise(lib):
    bc.case_nsteps2(lib, DEV)


# ---- the oracle against the reference's outputs for the new fixtures, under tests/test_oracle_golden.py's rules
@pytest.mark.parametrize("ckpt,gname", [(bc.GRID, bc.GRID_GOLDEN), (bc.EGO7, bc.EGO7_GOLDEN), (bc.EGO12, bc.EGO12_GOLDEN)])
def test_oracle_vs_reference_g1(ckpt, gname):
    g = load_golden(f"g1_{gname}.npz")
    assert rng_matches(g)
    meta, nets = OG.nets_from_ckpt(ckpt)
    d = meta["config"]["data"]
    N, F, d_min, d_max = d["max_node_num"], d["max_feat_num"], d["d_min"], d["d_max"]
    flags = torch.from_numpy(g["flags"])
    B = flags.shape[0]
    for tag, scale in (("unit", 1.0), ("small", 0.3)):
        x, adj, rank2 = OG.masked_state(int(g["seed"]), B, N, F, True, d_min, d_max, flags, scale)
        assert np.array_equal(x.numpy(), g[f"{tag}/x"]) and np.array_equal(adj.numpy(), g[f"{tag}/adj"])
        with torch.no_grad():
            # (the grid fixture's rank-2 network is cc_large/ccsd_grid_small_CC's, pinned by tests/test_cc_large_graph.py: minutes at N = 49)
            for p, net in list(zip(bc.NAMES, nets))[:2 if ckpt == bc.GRID else 3]:
                OG._check(net(x, adj, rank2, flags).numpy(), g, f"{tag}/net_{p}", f"{gname} {tag} net_{p}")
            if tag == "unit":
                for ti, tval in enumerate([1.0, 0.5, 1e-4]):
                    for p, net in list(zip(bc.NAMES, nets))[:2]:
                        fn = O.make_score_fn(O.load_sde(meta["config"]["sde"][p]), net)
                        OG._check(fn(x, adj, rank2, flags, torch.ones(B) * tval).numpy(), g, f"unit/score_{p}_t{ti}", f"{gname} score_{p} t{ti}")


def test_oracle_vs_reference_g5_three_layers():
    OG.test_g5_pc_sampler_identical_seed(bc.EGO7_GOLDEN, bc.EGO7, ["n4_first2"])
