"""CPU suite for the tiled graph-network route (graph-only plans above 64 nodes; ccsd_amd/csrc/ccsd_k_lg.h): the oracle against the
reference goldens of gdss_enzymes / gdss_grid, the planner, and the host emulation of the k_lg_* kernels against the oracle."""
import glob
import math
import os

import numpy as np
import pytest
import torch

from oracle import ccsd_oracle as O
from tests import large_graph_cases as lc
from tests import parity_cases as pc
from tests import test_oracle_golden as OG
from tests.emu_util import emu_library
from tests.helpers import CKPT, GOLDEN_CKPT, load_ckpt_np, load_golden, rng_matches

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_oracle_vs_reference_g1_enzymes():
    """The oracle reproduces the reference's gdss_enzymes forwards (N = 125) and score functions at three t (g1)."""
    OG.test_g1_network_forward_and_score_fn("gdss_enzymes")


@pytest.mark.parametrize("gname", sorted(lc.LARGE))
def test_oracle_vs_reference_g5(gname):
    """The oracle's sampler reproduces the reference's first three 1000-scale steps (g5; grid's 361 x 361 outputs as sha256 + subsample
    + row sums, which the oracle must match bit for bit), the step count, the trajectory length and the quantised adjacency."""
    g = load_golden(f"g5_{gname}.npz")
    assert rng_matches(g)
    case = "n1000_first3"
    fn, nets, flags, parts = OG.oracle_sampler_from_golden(g, gname, case)
    torch.manual_seed(int(g["seed"]))
    res = fn(*nets, flags)
    for p, v in zip(parts, res):
        OG._check(v.numpy(), g, f"{case}/{p}", f"{gname} {case} {p}")
    assert int(res[len(parts)]) == int(g[f"{case}/nfe"])
    assert len(res[-1]) == int(g[f"{case}/traj_len"])
    OG._check(res[-1][-1][1].numpy(), g, f"{case}/traj_last_adj", "traj_last_adj")
    OG._check(O.quantize(res[1]).numpy(), g, f"{case}/quantize_adj", "quantize_adj", exact=True)
    OG._check(O.quantize_mol(res[1].clone()), g, f"{case}/quantize_mol_adj", "quantize_mol_adj", exact=True)


@pytest.mark.parametrize("name", sorted(lc.LARGE))
def test_planner_large_checkpoints(lib, name):
    meta, parts = load_ckpt_np(name)
    assert meta["params_adj"]["max_node_num"] == lc.LARGE[name]
    eng = lc.engine(meta, parts, lib, DEV)
    assert eng.query("large_graph") == 1


def _planned_before():
    names = set()
    for d in (CKPT, GOLDEN_CKPT):
        names |= {os.path.basename(f)[:-5] for f in glob.glob(os.path.join(d, "*.json"))}
    return sorted(names - set(lc.LARGE))


# k_xa variant of every checkpoint that planned before the tiled route existed, as the parent tree's planner selects it
XA_VARIANT = {"ccsd_community_small_Base_CC": 1, "ccsd_community_small_CC": 8, "ccsd_ego_small_CC": 0, "ccsd_ego_small_CC_v2": 0,
              "ccsd_enzymes_small_Base_CC": 1, "ccsd_enzymes_small_CC": 10, "ccsd_qm9_Base_CC": 1, "ccsd_qm9_CC": 7,
              "gdss_community_small": 5, "gdss_ego_small": 0, "gdss_ego_small_retrained": 0, "gdss_enzymes_small_retrained": 3,
              "gdss_qm9": 4, "gdss_qm9_retrained": 4, "gdss_zinc250k": 6, "zinc250k_CC_5b": 6}


def test_planner_pins_every_checkpoint():
    assert set(XA_VARIANT) == set(_planned_before())


@pytest.mark.parametrize("name", _planned_before())
def test_planner_existing_checkpoints_keep_k_xa(lib, name, monkeypatch):
    """Every checkpoint that planned before still plans on k_xa (large_graph == 0) with the same k_xa variant."""
    monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
    eng, meta, _ = pc.engine_from_ckpt(name, lib, DEV)
    assert eng.query("large_graph") == 0
    assert eng.query("xa_variant") == XA_VARIANT[name]


def test_emu_no_xa_layout_takes_the_route(lib):
    """N <= 64 without a k_xa LDS layout: gdss_community_small's networks at N = 64 (eight 64 x 64 attention channels alone are 128 KB)
    plan on the tiled route instead of failing, and match the oracle."""
    meta, parts = lc.resized("gdss_community_small", 64, seed=64)
    lc.case_forward_vs_oracle_src(meta, parts, lib, DEV, [64, 40], "community_small@64 (no k_xa layout)")


def test_planner_rejections(lib):
    lc.case_planner_rejects(lib, DEV)


def test_emu_forward_enzymes(lib):
    """gdss_enzymes (N = 125) at B = 2 through the emulated tiled kernels against the oracle, a full and a one-node graph."""
    meta, parts = load_ckpt_np("gdss_enzymes")
    lc.case_forward_vs_oracle_src(meta, parts, lib, DEV, [125, 1], "gdss_enzymes")


@pytest.mark.parametrize("N", [67, 97])
def test_emu_forward_random_weights(lib, N):
    """A random-weight ScoreNetworkX / ScoreNetworkA (gdss_community_small's architecture) at node counts that are not multiples of
    any tile, with a full, a one-node and an empty graph."""
    meta, parts = lc.resized("gdss_community_small", N, seed=N)
    lc.case_forward_vs_oracle_src(meta, parts, lib, DEV, [N, 1, 0], f"N={N}")


def test_emu_forced_route_community_small(lib, monkeypatch):
    lc.case_forced_vs_xa("gdss_community_small", lib, DEV, 3, [20, 11, 1], monkeypatch=monkeypatch)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("S4", "None", 0.15, 0.7), ("Reverse", "Langevin", 0.1, 0.7)])
def test_emu_production_loop(lib, predictor, corrector, snr, seps):
    """ccsd_sampler_run (and the step-wise loop, bit for bit) against the oracle's replay of the exported draws at N = 67."""
    src = lc.resized("gdss_community_small", 67, seed=3)
    pc.case_production_loop_vs_oracle("community_small@67", lib, DEV, 2, [67, 30], 2, predictor, corrector, snr, seps, source=src,
                                      expect_route={"large_graph": 1})


# ---- harness: node counts of generic datasets from the user's copy of the dataset (ccsd_amd/sampler.py)
def test_harness_generic_node_counts_from_the_dataset_pickle(tmp_path):
    """ENZYMES / grid have no node_counts.json entry: the counts of the training split come from <folder>/<data.dir>/<data>.pkl
    (data_loader.py:76-81: graph_list[int(test_split * len):], file order), and init_flags draws the reference's indices from them."""
    from ccsd_amd import sampler as S
    from ccsd_amd.loader import AttrDict

    sizes = [125, 3, 17, 64, 2, 99, 125, 40, 7, 88, 61, 12]
    lc.graph_pickle(str(tmp_path / "data" / "ENZYMES.pkl"), sizes)
    cfgt = AttrDict({"folder": str(tmp_path), "data": {"data": "ENZYMES", "dir": "./data", "test_split": 0.2, "max_node_num": 125,
                                                         "batch_size": 64}})
    assert S.train_node_counts(cfgt) is None
    counts, n_test = S.graph_train_node_counts(AttrDict({}), cfgt)
    assert n_test == 2 and counts.tolist() == sizes[2:]
    np.random.seed(7)
    fl = S.init_flags(counts, cfgt, 16)
    np.random.seed(7)
    want = torch.zeros(16, 125)
    for b, i in enumerate(np.random.randint(0, len(counts), 16)):
        want[b, : counts[i]] = 1
    assert torch.equal(fl, want)
    assert S.graph_train_node_counts(AttrDict({}), AttrDict({"folder": str(tmp_path / "nowhere"), "data": {"data": "ENZYMES"}})) == (None, 0)


def test_harness_enzymes_yaml_from_the_dataset_pickle(lib, tmp_path):
    """CCSD(type="sample", config=<yaml with ckpt gdss_enzymes>, folder=<checkout>): node counts from the dataset pickle, the test
    split sets the number of rounds (ceil(n_test / batch_size)), flags as init_flags draws them, the tiled route samples N = 125."""
    from ccsd_amd import sampler as S
    from tests import test_harness as H

    sizes = [int(v) for v in np.random.RandomState(3).randint(2, 126, 700)]
    lc.graph_pickle(str(tmp_path / "data" / "ENZYMES.pkl"), sizes)
    lc.enzymes_folder(tmp_path, batch_size=3)           # (a batch of 3 keeps the emulation short; the shipped config's is 64)
    out, c = H.run_harness(tmp_path, lib, None, "sample_enzymes", lc.ENZYMES_YAML, max_steps=1, rounds=1)
    sm = c.sampler
    assert "training graphs" in sm.node_counts_source and sm.n_test == 140 and list(sm.node_counts) == sizes[140:]
    assert math.ceil(sm.n_test / sm.configt.data.batch_size) == 47         # the rounds sample() runs when `rounds` is not given
    np.random.seed(42)
    want = S.init_flags(sizes[140:], sm.configt, 3)
    assert torch.equal(out["flags"].cpu(), want)
    a, fl = out["adj_int"].cpu(), out["flags"].cpu()
    assert a.shape == (3, 125, 125) and torch.equal(a, a.transpose(1, 2)) and not torch.diagonal(a, dim1=1, dim2=2).any()
    assert not (a * (1 - fl[:, :, None] * fl[:, None, :])).any()


def test_harness_node_counts_argument_without_the_dataset(lib, tmp_path):
    """Without the dataset file, `node_counts=` still drives the flags (and nothing else is needed); without either the error says
    what to provide."""
    from tests import test_harness as H

    lc.enzymes_folder(tmp_path, batch_size=2)
    out, c = H.run_harness(tmp_path, lib, None, "sample_enzymes", lc.ENZYMES_YAML, max_steps=1, node_counts=[125, 30])
    assert "node_counts=" in c.sampler.node_counts_source and set(out["flags"].sum(1).long().tolist()) <= {125, 30}
    with pytest.raises(FileNotFoundError, match="ENZYMES.pkl"):
        H.run_harness(tmp_path, lib, None, "sample_enzymes", lc.ENZYMES_YAML, max_steps=1)
