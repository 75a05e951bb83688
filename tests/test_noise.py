"""CPU suite of the noise stream: the host emulation of the kernel source (libm's logf / sqrtf / sinf / cosf in place of the
hardware transcendentals) against tests/philox_ref.py over the whole grid of tests/noise_cases.py, every element."""
import pytest
import torch

from tests import noise_cases as nc
from tests.emu_util import emu_library

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


CALLS = [(plan, hs) for plan in nc.PLANS for hs in nc.slots(plan)]


@pytest.mark.parametrize("sample_offset", nc.OFFSETS, ids=lambda v: f"off{v:#x}")
@pytest.mark.parametrize("seed", nc.SEEDS, ids=lambda v: f"seed{v:#x}")
@pytest.mark.parametrize("plan,hs", CALLS, ids=[f"{p}-{nc.slot_id(h)}" for p, h in CALLS])
def test_emu_stream_vs_reference(lib, plan, hs, seed, sample_offset):
    nc.case_stream(plan, lib, DEV, seed, sample_offset, hs, nc.BOUND_EMU)


@pytest.mark.parametrize("plan", list(nc.PLANS))
def test_emu_sample_offset_tiles_the_stream(lib, plan):
    nc.case_offset_tiling(plan, lib, DEV)
