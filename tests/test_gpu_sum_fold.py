"""GPU suite of the folded batch norm sums (tests/sum_fold_cases.py): the folded loop against the loop with k_normsum launches, bit
for bit, at the batches where the in-kernel reduction takes another shape -- nv = normsum_threads(B) virtual threads on k_r2's 512:
  B = 1, 2    workgroup 0 is all there is
  B = 200     nv = 256: half of the waves have no virtual wave
  B = 300     nv = 512
  B = 600     nv = 1024, two virtual waves per wave; more workgroups than the chip holds at once (two per CU): late workgroups start
              after early ones have written the next step's partials -- what the two alternating buffers are for
  B = 1100    virtual threads with two samples; the batch bucket of the baked qm9 instance
with 5 and 6 steps each (both parities of the buffers at the end of a call)."""
import pytest
import torch

from ccsd_amd import _lib
from tests import sum_fold_cases as sf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGES = [(0, 5), (0, 6)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _lib.get_library()


@pytest.mark.parametrize("B", [1, 2, 200, 300, 600])
def test_fold_equals_normsum_launches(lib, B):
    sf.case_on_off(sf.QM9, lib, DEV, B, RANGES)


def test_fold_equals_normsum_launches_b1100_and_repeats(lib):
    sf.case_on_off(sf.QM9, lib, DEV, 1100, RANGES, twice=True)


def test_fold_qm9_base_cc(lib):
    """k_r2<3, 0, false, false, 1>: the non-affine ScoreNetworkF instance, un-merged launches."""
    sf.case_on_off(sf.QM9_BASE, lib, DEV, 600, RANGES)


def test_reduce_hook_keeps_normsum(lib):
    sf.case_reduce_hook_keeps_normsum(sf.QM9, lib, DEV, 600, 0, 5)


def test_route(lib):
    sf.case_route(lib, DEV)
