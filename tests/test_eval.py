"""CPU suite for the evaluation of finished samples (ccsd_cluster_hist, ccsd_mmd, ccsd_amd/evaluation.py, Sampler.evaluate) over the host
emulation of k_cluster_hist / k_mmd_prep / k_mmd_pairs / k_mmd_final: clustering histograms bit-exact against the reference's
clustering_worker (tests/golden/e1_eval.npz) and a numpy restatement, MMD scores against a float64 restatement and the reference's own
scores, and the host layer against the reference's rounded dicts."""
import math

import numpy as np
import pytest
import torch

from tests import eval_cases as ec
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_fixture_lists_the_graph_sets():
    z, meta = ec.e1()
    assert set(meta["graph_sets"]) == set(ec.GRAPH_SETS)
    assert meta["lp_vs_closed_kernel"] == max(meta["lp_vs_closed"].values())
    # integer histograms: the linear programs and the closed form agree to rounding
    assert max(v for k, v in meta["lp_vs_closed"].items() if k.startswith(("degree", "cluster", "mmd/ragged", "mmd/n65"))) < 1e-12


@pytest.mark.parametrize("bins", ec.BINS)
@pytest.mark.parametrize("name", ec.GRAPH_SETS)
def test_emu_cluster_hist(lib, name, bins):
    ec.case_cluster(lib, DEV, name, bins)


def test_emu_cluster_landmarks(lib):
    ec.case_cluster_landmarks(lib, DEV)


def test_emu_cluster_raw_samples_and_null_outputs(lib):
    ec.case_cluster_raw_and_null(lib, DEV)


def test_emu_bad_dims(lib):
    ec.case_bad_dims(lib, DEV)


@pytest.mark.parametrize("name", list(ec.MMD_SHAPES))
def test_emu_mmd_against_restatement(lib, name):
    ec.case_mmd_restatement(lib, DEV, name)


@pytest.mark.parametrize("name", ["n3_l2", "n64_l33", "n130_l33"])
def test_emu_mmd_of_identical_sets_is_zero(lib, name):
    ec.case_mmd_identical(lib, DEV, name)


@pytest.mark.parametrize("name", ec.mmd_fixture_sets())
def test_emu_mmd_against_reference_scores(lib, name):
    ec.case_mmd_reference(lib, DEV, name)


def test_emu_eval_torch_batch(lib):
    ec.case_eval_torch_batch(lib, DEV)


def test_emu_eval_cc_batch(lib):
    ec.case_eval_cc_batch(lib, DEV)


def test_emu_unsupported_methods_raise(lib):
    ec.case_unsupported(lib, DEV)


GRAPH_YAML = {
    "is_cc": False,
    "data": {"data": "community_small", "dir": "./data"},
    "ckpt": "gdss_community_small",
    "sampler": {"predictor": "Euler", "corrector": "Langevin", "snr": 0.05, "scale_eps": 0.7, "n_steps": 1},
    "sample": {"use_ema": False, "noise_removal": True, "probability_flow": False, "eps": 1.0e-4, "seed": 42},
}


def test_sampler_evaluate_on_a_graph_only_run(lib, tmp_path):
    """Sampler.evaluate on a short graph-only harness run: finite scores against a held-out adjacency batch of another node count, and
    0 within 1e-12 when the run is scored against itself -- as a dict and as the .npz that sample(save=True) wrote."""
    import os

    from tests.test_harness import run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_community_small", GRAPH_YAML, max_steps=2, rounds=1)
    keys = set(out)
    z, _ = ec.e1()
    scores = c.sampler.evaluate(out, torch.from_numpy(z["graphs/eval_ref/adj"]))
    assert set(scores) == {"degree", "cluster"} and all(math.isfinite(v) and -1e-12 <= v <= 2.0 for v in scores.values()), scores
    assert set(out) == keys                                                          # (the result dict is not written to)
    (fname,) = os.listdir(tmp_path / "samples")
    for ref in (out, str(tmp_path / "samples" / fname)):
        same = c.sampler.evaluate(out, ref)
        assert set(same) == {"degree", "cluster"} and all(abs(v) <= 1e-12 for v in same.values()), same
    d = ec.ev.describe(out["adj"], device=DEV, lib=lib)
    t = ec.ev.mmd_terms(d["cluster_hist"], d["cluster_hist"], sigma=0.1, distance_scaling=100, device=DEV, lib=lib)
    assert abs(t[3].item()) <= 1e-12 and 0.0 < t[0].item() <= 1.0


def test_sampler_evaluate_on_a_complex_run(lib, tmp_path):
    """The combinatorial-complex branch of Sampler.evaluate on a short qm9_CC harness run: rank1_distrib and rank2_distrib ride on
    the run's own descriptors (0 within 1e-12 against itself), equal eval_CC_batch called by hand against a different set, fall back
    to the molecule default 1..3 when the config names no edge values, rank2_distrib is left out when the held-out side is a bare
    adjacency batch, cc_methods selects, and a rank other than 0 of a sharded run does not evaluate."""
    from tests.test_harness import QM9_CC_YAML, run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2)
    s = c.sampler
    assert s.is_cc and s.is_mol
    assert int(out["n_nodes"].min()) > 0                                             # (no complex is dropped as empty)
    same = s.evaluate(out, out)
    assert set(same) == {"degree", "cluster", "rank1_distrib", "rank2_distrib"} and all(abs(v) <= 1e-12 for v in same.values()), same
    # a different held-out set: the first three complexes of the run
    held = {k: out[k][:3] for k in ("adj", "degree_hist", "edge_hist", "n_nodes", "rank2_cell_hist")}
    got = s.evaluate(out, held)
    kw = dict(device=DEV, lib=lib)
    by_hand = ec.ev.eval_CC_batch(held, out, {"min_edge_val": 1, "max_edge_val": 3}, ["rank1_distrib", "rank2_distrib"], **kw)
    assert {k: got[k] for k in by_hand} == by_hand and all(math.isfinite(v) for v in got.values()), (got, by_hand)
    assert got["degree"] == ec.ev.eval_torch_batch(ec.ev.describe(held["adj"], mol=True, **kw), ec.ev.describe(out["adj"], mol=True, **kw),
                                                   ["degree"], **kw)["degree"]
    # data.min_edge_val / data.max_edge_val absent: 1..3 for molecules
    for k in ("min_edge_val", "max_edge_val"):
        del s.config["data"][k]
    assert s.evaluate(out, held) == got
    # a bare adjacency batch holds no rank-2 histogram: rank2_distrib is left out; asking for it by name fails loudly
    bare = s.evaluate(out, out["adj"][:3])
    assert set(bare) == {"degree", "cluster", "rank1_distrib"} and bare["rank1_distrib"] == got["rank1_distrib"]
    assert s.evaluate(out, held, cc_methods=["rank2_distrib"]).keys() == {"degree", "cluster", "rank2_distrib"}
    with pytest.raises(KeyError):
        s.evaluate(out, out["adj"][:3], cc_methods=["rank2_distrib"])
    with pytest.raises(NotImplementedError, match="rank0_distrib"):
        s.evaluate(out, held, cc_methods=["rank0_distrib"])
    s.rank = 1
    assert s.evaluate(out, out) == {}
