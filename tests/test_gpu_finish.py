"""GPU suite (-m gpu) for the one-pass finish of a sampling run on the MI355X: the cases of tests/test_finish.py on k_finish_rank2 /
k_finish_graph themselves, and the condition that finish() allocates nothing beyond what it returns."""
import pytest
import torch

from tests import finish_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("name", list(fc.GEOMETRIES))
def test_bitwise_against_existing_entry_points(lib, name):
    fc.case_bitwise(lib, DEV, name)


@pytest.mark.parametrize("name", list(fc.GEOMETRIES))
def test_descriptors_against_numpy(lib, name):
    fc.case_descriptors(lib, DEV, name)


@pytest.mark.parametrize("name,case", fc.f1_cases())
def test_descriptors_against_reference_fixture(lib, name, case):
    fc.case_reference_fixture(lib, DEV, name, case)


def test_null_outputs(lib):
    fc.case_null_outputs(lib, DEV)


def test_bad_dims(lib):
    fc.case_bad_dims(lib, DEV)


def test_sample_ops_need_no_plan(lib, monkeypatch):
    fc.case_no_plan(lib, DEV, monkeypatch)


def test_no_int64_temporary(lib):
    """At N = 38, d = 3, B = 2 the device peak rises by at most the bytes of the returned tensors plus 1 MB (the three separate calls
    exceed that by the int64 copy of rank2, 8 B E K bytes).  A condition on the allocations, not a measurement."""
    B, N, F, d = 2, 38, 9, 3
    E, K = N * (N - 1) // 2, 8436
    gen = torch.Generator(device=DEV).manual_seed(3)
    x, adj, rank2 = (torch.randn(s, device=DEV, generator=gen) for s in ((B, N, F), (B, N, N), (B, E, K)))
    eng = fc.sample_ops(lib, DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = eng.finish(x, adj, rank2, None, mol=True, d_min=d, d_max=d)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    returned = sum(v.numel() * v.element_size() for v in res.values())
    assert returned >= B * E * K and rise <= returned + (1 << 20), (rise, returned)
    assert 8 * B * E * K > (1 << 20)          # (what the int64 copy would have added is well above the allowance)
