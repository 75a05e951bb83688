"""Host-emulation suite of the input classes (tests/state_class_cases.py): flags with holes, unmasked states, a non-zero adjacency
diagonal -- through ccsd_score on every route, the step calls, the production loop and the noise stream.  The emulation runs the same
kernel source, so the mask products, the bit tables of k_flagbits / k_masktab and the hodge-projection loader's re-masking are the
device's; its MFMA and wave-level forms, the baked instances and the GPU-only kernels are tests/test_gpu_state_classes.py's."""
import pytest

from tests import noise_cases as nc
from tests import state_class_cases as sc
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_flag_and_state_builders():
    """make_flags_holes: the counts of make_flags, never a prefix, both edge patterns; make_state: the three kinds share their draws."""
    import torch

    from oracle import ccsd_oracle as O
    from tests.helpers import make_flags, make_flags_holes, make_state

    for N in (5, 9, 33, 64, 70):
        counts = sc.counts_of(N)
        f = make_flags_holes(len(counts), N, counts, 3)
        assert torch.equal(f.sum(1), make_flags(len(counts), N, counts).sum(1))
        assert torch.equal(f, make_flags_holes(len(counts), N, counts, 3)) and not torch.equal(f, make_flags_holes(len(counts), N, counts, 4))
        assert ((f == 0) | (f == 1)).all()
    flags = make_flags_holes(6, 9, sc.counts_of(9), 3)
    m, u, d = (make_state(k, 11, 6, 9, 4, True, 3, 9, flags) for k in ("masked", "unmasked", "diag"))
    assert torch.equal(m[0], O.mask_x(u[0], flags)) and torch.equal(m[1], O.mask_adjs(u[1], flags))
    assert torch.equal(m[2], O.mask_rank2(u[2], 9, 3, 9, flags))
    assert torch.equal(u[1], u[1].transpose(1, 2)) and not u[1].diagonal(dim1=1, dim2=2).any()
    assert (u[0][flags == 0] != 0).any() and (u[2] != m[2]).any()
    off = d[1] - m[1]
    assert torch.equal(off, torch.diag_embed(off.diagonal(dim1=1, dim2=2))) and (off.diagonal(dim1=1, dim2=2)[flags == 1] != 0).all()
    assert torch.equal(d[0], m[0]) and torch.equal(d[2], m[2])


def test_forward_qm9_instances(lib):
    sc.case_forward_qm9_instances(lib, DEV)


@pytest.mark.parametrize("name", list(sc.CHECKPOINTS))
def test_forward_checkpoint(lib, name):
    sc.case_forward_checkpoint(name, lib, DEV)


def test_forward_ew1(lib):
    sc.case_forward_ew1(lib, DEV)


def test_forward_hodge_general(lib):
    sc.case_forward_hodge_general(lib, DEV)


def test_forward_hodge_wide(lib):
    sc.case_forward_hodge_wide(lib, DEV)


@pytest.mark.parametrize("name", list(sc.FORCED))
def test_forward_forced_tiled_route(lib, name):
    sc.case_forward_forced_tiled(name, lib, DEV)


def test_forward_tiled_route_n70(lib):
    sc.case_forward_n70(lib, DEV)


@pytest.mark.parametrize("N", [33, 64])
def test_forward_word_edge_graph(lib, N):
    sc.case_forward_word_edge_graph(N, lib, DEV)


def test_forward_word_edge_complex(lib):
    sc.case_forward_word_edge_complex(33, lib, DEV)


@pytest.mark.parametrize("cls", ["H", "HU"])
@pytest.mark.parametrize("name", list(sc.STEP_PLANS))
def test_step_calls(lib, name, cls):
    sc.case_step_calls(name, cls, lib, DEV)


@pytest.mark.parametrize("form", list(sc.LOOPS))
def test_production_loop_holes(lib, form):
    sc.case_production_loop(form, lib, DEV)


def test_one_step_holes(lib):
    sc.case_one_step_holes("ccsd_qm9_CC", lib, DEV, "Reverse", "Langevin", 0.2, 0.7)
    sc.case_one_step_holes("gdss_community_small", lib, DEV, "Euler", "Langevin", 0.05, 0.7)


@pytest.mark.parametrize("plan", list(sc.NOISE_SLOTS))
def test_noise_holes(lib, plan):
    sc.case_noise(plan, lib, DEV, nc.BOUND_EMU)


def test_complex_masks_small_twin(lib):
    """tests/test_gpu_state_classes.py runs this case at N = 64 (E K = 8.4 10^7 per sample: minutes here); N = 12 runs its logic."""
    sc.case_complex_masks(12, (3, 4), lib, DEV)
