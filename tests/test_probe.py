"""The device helpers behind the noise stream, compiled for the host (tests/emu/ccsd_probe.cpp), against tests/philox_ref.py and
plain integer arithmetic: philox4, philox_normal4, FastDiv at the edge of its stated domain, the flat split of k_noise_norm /
k_langevin_apply / k_ew1 exhaustively at every (E, K) of SHAPES, and k_noise_norm's masks on [full, empty] batches."""
import ctypes as C

import numpy as np
import pytest

from oracle import ccsd_oracle as O
from tests import philox_ref as R
from tests.emu_util import probe_library
from tests.test_philox_ref import KAT

# (N, d_min, d_max): the architecture shapes at which FastDiv(K) split flat groups wrongly (E K > 2^22) with the number of groups it
# split with the quotient one low / one high, their neighbours where it happened to be right, and the shipped geometries
SHAPES = {
    (43, 3, 3): (0, 0), (44, 3, 3): (206, 0), (45, 3, 3): (125, 0), (47, 3, 3): (0, 15), (49, 3, 3): (0, 0),
    (30, 3, 4): (28, 0), (31, 3, 4): (12, 0),
    (9, 3, 9): (0, 0), (20, 3, 3): (0, 0), (12, 3, 4): (0, 0), (38, 3, 3): (0, 0), (18, 3, 5): (0, 0), (7, 3, 5): (0, 0),
}
LL = C.c_longlong


@pytest.fixture(scope="module")
def probe():
    lib = probe_library()
    lib.probe_fastdiv_errors.restype = LL
    lib.probe_split_errors.restype = LL
    return lib


def _u32(a):
    a = np.ascontiguousarray(a, np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint))


def device_philox4(probe, ctr, key):
    ctr, pc = _u32(ctr)
    key, pk = _u32(key)
    out, po = _u32(np.zeros_like(ctr))
    probe.probe_philox4(LL(len(ctr)), pc, pk, po)
    return out


def test_philox4_known_answers_and_reference(probe):
    got = device_philox4(probe, [k[0] for k in KAT], [k[1] for k in KAT])
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, (20000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (20000, 2), dtype=np.uint64)
    ctr[:4] = [[0xFFFFFFFF, 0, 0, 0], [0, 0xFFFFFFFF, 0, 0], [0, 0, 0xFFFFFFFF, 0], [0, 0, 0, 0xFFFFFFFF]]   # one word at a time
    assert np.array_equal(device_philox4(probe, ctr, key), R.philox4x32_10(ctr, key))


# libm's logf / sqrtf / sinf / cosf in fp32 against float64 Box-Muller: the radius is at most 5.77 (ulp 4.8e-7), 2 pi u2 is rounded
# to fp32 before sinf / cosf (|d arg| <= 2.4e-7 at arg -> 6.28, times the radius: 1.4e-6) and -2 logf(u1) carries ~1 ulp (3e-7 on
# the radius near its maximum): a few 1e-6 in all.  tests/noise_cases.py holds the measured value and the bound derived from it.
@pytest.mark.parametrize("seed,draw,b", [(0, 0, 0), (1, 5, 7), (1 << 32, 3002, (1 << 32) - 1), ((1 << 64) - 1, 8999, (1 << 40) + 3)])
def test_philox_normal4(probe, seed, draw, b):
    """The keying of philox_normal4 -- counter (group, low32 b, draw, high32 b), key (low32 seed, high32 seed) -- and its Box-Muller
    lanes, on 50000 groups including the last ones of the 32-bit range."""
    from tests.noise_cases import BOUND_EMU

    g = np.concatenate([np.arange(49990, dtype=np.uint64), np.arange((1 << 32) - 10, 1 << 32, dtype=np.uint64)])
    gg, pg = _u32(g)
    out = np.zeros((len(g), 4), np.float32)
    probe.probe_philox_normal4(LL(len(g)), C.c_ulonglong(seed), C.c_uint(draw), LL(b), pg, out.ctypes.data_as(C.POINTER(C.c_float)))
    want = R.normals(g, b, draw, seed)
    err = np.abs(out.astype(np.float64) - want).max()
    print(f"philox_normal4 (host libm) vs float64: max |diff| = {err:.3e}")
    assert err <= BOUND_EMU


def test_fastdiv_domain_edge(probe):
    """FastDiv's stated domain, 0 <= t <= 2^22 - 1 for every 1 <= d <= 2^24: exact over the whole of it for a spread of divisors
    (every d up to 128, the E and K of SHAPES and their neighbours, powers of two and their neighbours up to 2^24), over the last
    2^16 values below the edge for every d up to 4096 -- and not beyond it: t = 4243964, d = 255 is a miss."""
    first = LL()
    ds = set(range(1, 129)) | {255, 1000, 4095, 4097, (1 << 22) - 1, 1 << 22, (1 << 24) - 1, 1 << 24}
    for N, d_min, d_max in SHAPES:
        E, K = O.get_rank2_dim(N, d_min, d_max)
        ds |= {E, K, K - 1, K + 1, K >> 1}
    ds |= {(1 << s) + o for s in range(8, 24) for o in (-1, 0, 1)}
    for d in sorted(ds):
        assert probe.probe_fastdiv_errors(d, LL(0), LL(1 << 22), C.byref(first)) == 0, f"FastDiv({d}) misses t = {first.value} inside its domain"
    for d in range(1, 4097):
        assert probe.probe_fastdiv_errors(d, LL((1 << 22) - (1 << 16)), LL(1 << 22), C.byref(first)) == 0, f"FastDiv({d}) misses t = {first.value}"
    assert probe.probe_fastdiv_errors(255, LL(1 << 22), LL(4243965), C.byref(first)) == 1 and first.value == 4243964


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "N%d_d%d_%d" % s)
def test_flat_split_exhaustive(probe, shape):
    """flat_split at the first element of EVERY flat group of the block, against integer division; and the check itself against the
    split it replaced: FastDiv(K) in its place shows the recorded number of wrongly split groups at this shape."""
    E, K = O.get_rank2_dim(*shape)
    assert E * K < 1 << 31
    low, high = LL(), LL()
    assert probe.probe_split_errors(E, K, 0, LL(0), LL(4), C.byref(low), C.byref(high)) == 0, f"flat_split wrong at E = {E}, K = {K}: {low.value} low, {high.value} high"
    bad = probe.probe_split_errors(E, K, 1, LL(0), LL(4), C.byref(low), C.byref(high))
    assert (low.value, high.value) == SHAPES[shape] and bad == sum(SHAPES[shape])


def test_flat_split_domain_edge(probe):
    """The helper's own domain, every t < 2^31, at the largest blocks an int can index (divisors 1, 2, 3, the largest ones and the
    square): the last 2^20 groups below E K one by one, and every 1021st group of the whole block."""
    low, high = LL(), LL()
    for E, K in (((1 << 31) - 1, 1), ((1 << 30) - 1, 2), (715827882, 3), (1, (1 << 31) - 1), (2, (1 << 30) - 1), (46340, 46340)):
        top = (E * K - (1 << 22)) & ~3
        assert probe.probe_split_errors(E, K, 0, LL(top), LL(4), C.byref(low), C.byref(high)) == 0, (E, K)
        assert probe.probe_split_errors(E, K, 0, LL(0), LL(4 * 1021), C.byref(low), C.byref(high)) == 0, (E, K)


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "N%d_d%d_%d" % s)
def test_noise_norm_counts(probe, shape):
    """k_noise_norm<0, 0> with all-ones draws on [full, empty] and [empty, full]: the full complex counts E K entries with mask 1,
    the empty one none -- a group split into the wrong row reads the neighbour's mask bytes (or the row padding) instead."""
    E, K = O.get_rank2_dim(*shape)
    counts = (C.c_double * 2)()
    for full in (0, 1):
        probe.probe_noise_norm_counts(E, K, full, counts)
        assert counts[full] == E * K and counts[1 - full] == 0, f"E = {E}, K = {K}, full complex {full}: counts {list(counts)}"
