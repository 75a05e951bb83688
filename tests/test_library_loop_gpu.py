"""GPU suite (-m gpu): the library loop with a reduce hook and with sampler.n_steps > 1 on a real MI355X, and the exact mode over
a 1-rank RCCL group in a process of its own (tests/library_loop_cases.py; CPU twin: tests/test_library_loop.py)."""
import pytest
import torch

from tests import library_loop_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib

    L = _lib.get_library()
    assert L.is_hip and torch.cuda.is_available()
    return L


@pytest.mark.parametrize("form,B,steps", [("qm9_langevin_fused_merged", 1024, 4), ("community_small_cc_tiled_fuse", 512, 2),
                                          ("graph_only_langevin", 64, 3), ("enzymes_small_cc_s4", 250, 2), ("zinc5b_ew1", 4, 2),
                                          ("qm9_corrector_free", 64, 3)])
def test_hook_identity(lib, form, B, steps):
    """1. A hook that only counts changes nothing, in every loop form at its shipped batch, and fires once per norms pass."""
    lc.case_hook_identity(form, lib, DEV, B, steps)


@pytest.mark.parametrize("predictor", ["Reverse", "S4"])
def test_hook_values_are_what_the_kernels_consume(lib, predictor):
    """2. Half a batch fed with the full batch's sums reproduces the full batch's rows at 2e-6 (the bound of the gloo test: the
    threads per graph of k_xa depend on the batch); with its own sums it does not."""
    lc.case_hook_values_are_consumed(lib, DEV, 1024, 3, predictor, rtol=2e-6)


@pytest.mark.parametrize("n_steps", [2, 3])
@pytest.mark.parametrize("name,B,counts,predictor,snr", [("ccsd_qm9_CC", 256, lc.QM9_MIX, "Reverse", 0.2),
                                                         ("ccsd_community_small_CC", 32, lc.CS_MIX, "Euler", 0.05),
                                                         ("gdss_community_small", 64, [20, 12, 16, 18, 14], "Euler", 0.05)])
def test_nsteps_in_the_library_loop(lib, name, B, counts, predictor, snr, n_steps):
    """3. n_steps = 2, 3: last_loop == "library", bit for bit the step-wise driver, ccsd_sampler_run returns CCSD_OK."""
    lc.case_nsteps_library_vs_stepwise(name, lib, DEV, B, counts, 2, predictor, snr, 0.7, n_steps, keep_traj=name == "ccsd_qm9_CC")


def test_nsteps2_vs_oracle(lib):
    """3. qm9_CC, n_steps = 2 against the oracle on the exported draws (target-major within a step)."""
    lc.case_nsteps_vs_oracle(lib, DEV, B=12, counts=(9, 7, 8, 0, 4, 9, 1, 2, 6, 9, 5, 3))


def test_hook_failure(lib):
    """5. An exception in the hook comes out of PCEngine.run as itself; the engine stays usable."""
    lc.case_hook_failure(lib, DEV)


def test_rccl_single_rank_exact_mode_in_a_child_process(lib):
    """6. qm9_CC B = 1024 for eight steps and community_small_CC B = 512 for two, shipped samplers: load_sampling_fn_sharded
    (exact=True) on a forced 1-rank RCCL group == the plain closure bit for bit, on the library loop."""
    lc.case_rccl_single_rank_child()
