"""GPU suite (-m gpu) of the noise stream: what ccsd_init_state / ccsd_noise_draws write on the MI355X (v_log_f32, v_sqrt_f32,
v_sin_f32, v_cos_f32) against tests/philox_ref.py over the whole grid of tests/noise_cases.py, every element; and the production
loop at the node counts between N = 43 and N = 49 whose flat groups FastDiv(K) used to split into the wrong row."""
import pytest

from tests import cc_large_graph_cases as cc
from tests import noise_cases as nc
from tests import parity_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


CALLS = [(plan, hs) for plan in nc.PLANS for hs in nc.slots(plan)]


@pytest.mark.parametrize("sample_offset", nc.OFFSETS, ids=lambda v: f"off{v:#x}")
@pytest.mark.parametrize("seed", nc.SEEDS, ids=lambda v: f"seed{v:#x}")
@pytest.mark.parametrize("plan,hs", CALLS, ids=[f"{p}-{nc.slot_id(h)}" for p, h in CALLS])
def test_stream_vs_reference(lib, plan, hs, seed, sample_offset):
    nc.case_stream(plan, lib, DEV, seed, sample_offset, hs, nc.BOUND_GPU)


@pytest.mark.parametrize("plan", list(nc.PLANS))
def test_sample_offset_tiles_the_stream(lib, plan):
    nc.case_offset_tiling(plan, lib, DEV)


@pytest.mark.parametrize("N", cc.SPLIT_NODE_COUNTS)
def test_production_loop_at_split_shapes(lib, N):
    cc.case_split_shape_production_loop(lib, DEV, N)


def test_ew1_production_loop_n30_d3_4(lib):
    pc.case_ew1_odd_k_production_loop(lib, DEV)
