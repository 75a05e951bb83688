"""GPU suite for molecule post-processing (-m gpu): the case tables of tests/mol_cases.py through the HIP library, every output exact
against the plain Python restatement of tests/mol_ref.py; the call as a pure function of its arguments; and the properties on a real
sample() of the shipped qm9 checkpoint (no golden exists for it)."""
import numpy as np
import pytest
import torch

from tests import mol_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("largest_fragment", [True, False])
@pytest.mark.parametrize("name", ["hand"] + [n for n in mc.CASES if n != "N64_B257"])
def test_gpu_exact(name, largest_fragment):
    mc.case_exact(None, DEV, name, largest_fragment)


def test_gpu_exact_largest_batch():
    mc.case_exact(None, DEV, "N64_B257", True)


def test_gpu_pure():
    mc.case_pure(None, DEV)
    mc.case_pure(None, DEV, "N63")


def test_gpu_invalid():
    from ccsd_amd import _lib

    mc.case_invalid(_lib.get_library(), DEV)


def test_gpu_sampler_molecules_and_evaluate():
    mc.case_sampler(None, DEV)


def test_gpu_real_qm9_sample(tmp_path):
    """Twenty PC steps of the shipped qm9_CC checkpoint: the samples are far from molecules, so there is plenty to correct."""
    from ccsd_amd import evaluation as ev
    from tests.test_harness import QM9_CC_YAML, run_harness

    out, c = run_harness(tmp_path, None, None, "sample_qm9_CC", dict(QM9_CC_YAML, sample=dict(QM9_CC_YAML["sample"], n_samples=64)), max_steps=20)
    keys = set(out)
    table = ev.MOL_TABLES["QM9"]
    for lf in (True, False):
        mols = c.sampler.molecules(out, largest_fragment=lf)
        got = {k: mols[k].cpu().numpy() for k in mc.OUTPUTS}
        mc.check_properties(got, table, lf, f"qm9 sample, largest_fragment={lf}")
        mc.check_fixed_point(None, DEV, got, table, lf, "qm9 sample")
        want = mc.mol_ref.mol_correct(out["adj"].cpu().numpy(), ev.mol_labels(out["x"]).cpu().numpy(), table["max_valence"], table["charge_base"], lf)
        mc.assert_equal(got, want, "qm9 sample")
        assert 0.0 <= mols["validity_wo_correction"] <= 1.0 and mols["validity_wo_correction"] == float(np.mean(want["mol_no_correct"]))
    assert set(out) == keys
    res = c.sampler.evaluate(out, {"adj": out["adj"], "x": out["x"]}, nspdk=True, correct=True)
    assert set(res) == {"degree", "cluster", "nspdk", "rank1_distrib", "validity_wo_correction"} and all(np.isfinite(v) for v in res.values())
