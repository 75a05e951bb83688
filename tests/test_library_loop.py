"""CPU suite: the library loop with a reduce hook (ccsd_sampler_run_ex), sampler.n_steps > 1 inside it, and the exact multi-rank
mode on that route -- through the host emulation of the kernel source (tests/library_loop_cases.py; GPU twin:
tests/test_library_loop_gpu.py)."""
import pytest

from tests import library_loop_cases as lc
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


@pytest.mark.parametrize("form,B,steps", [("qm9_langevin_fused_merged", 5, 3), ("community_small_cc_tiled_fuse", 2, 2),
                                          ("graph_only_langevin", 3, 3), ("enzymes_small_cc_s4", 3, 2), ("zinc5b_ew1", 2, 2),
                                          ("qm9_corrector_free", 5, 3)])
def test_hook_identity(lib, form, B, steps):
    """1. A hook that only counts changes nothing, in every loop form, and fires once per norms pass."""
    lc.case_hook_identity(form, lib, DEV, B, steps)


@pytest.mark.parametrize("predictor", ["Reverse", "S4"])
def test_hook_values_are_what_the_kernels_consume(lib, predictor):
    """2. Half a batch fed with the full batch's sums reproduces the full batch's rows bit for bit; with its own sums it does not."""
    lc.case_hook_values_are_consumed(lib, DEV, 8, 3, predictor, rtol=0)


@pytest.mark.parametrize("n_steps", [2, 3])
@pytest.mark.parametrize("name,B,counts,predictor,snr", [("ccsd_qm9_CC", 5, [9, 7, 8, 0, 4], "Reverse", 0.2),
                                                         ("ccsd_community_small_CC", 2, [20, 13], "Euler", 0.05),
                                                         ("gdss_community_small", 3, [20, 12, 16], "Euler", 0.05)])
def test_nsteps_in_the_library_loop(lib, name, B, counts, predictor, snr, n_steps):
    """3. n_steps = 2, 3: last_loop == "library", bit for bit the step-wise driver, ccsd_sampler_run returns CCSD_OK."""
    lc.case_nsteps_library_vs_stepwise(name, lib, DEV, B, counts, 2, predictor, snr, 0.7, n_steps, keep_traj=name == "ccsd_qm9_CC")


def test_nsteps2_vs_oracle(lib):
    """3. qm9_CC, n_steps = 2 against the oracle on the exported draws (target-major within a step)."""
    lc.case_nsteps_vs_oracle(lib, DEV)


def test_two_gloo_ranks_take_the_library_loop(lib):
    """4. n_steps = 1, n_steps = 2 and S4 on ENZYMES_small_CC over two gloo ranks: library loop on both, == single process at 2e-6."""
    lc.case_two_gloo_ranks(lib)


def test_hook_failure(lib):
    """5. An exception in the hook comes out of PCEngine.run as itself; the engine stays usable."""
    lc.case_hook_failure(lib, DEV)
