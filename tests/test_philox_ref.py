"""tests/philox_ref.py against the world outside this repository (the Random123 known answers of Philox4x32-10), and the
draw-id schedule of the documented keying: no two (step, phase, target) of a run, the prior included, share a draw id."""
import itertools

import numpy as np
import pytest

from tests import philox_ref as R

# counter / key -> output, Random123 kat_vectors (philox4x32 10)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_known_answers():
    for ctr, key, want in KAT:
        got = R.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(v) for v in got) == want, (ctr, key, [hex(int(v)) for v in got])
    # vectorised: the three at once, and broadcast of one key over many counters
    got = R.philox4x32_10(np.array([k[0] for k in KAT], np.uint64), np.array([k[1] for k in KAT], np.uint64))
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]
    many = R.philox4x32_10(np.zeros((5, 4), np.uint64), np.zeros(2, np.uint64))
    assert all(tuple(int(v) for v in row) == KAT[0][2] for row in many)


def test_scalar_restatement_agrees():
    """The vectorised rounds against a plain Python-int loop on random counters (a second statement of the same ten rounds)."""
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (64, 2), dtype=np.uint64)
    got = R.philox4x32_10(ctr, key)
    for row, k, g in zip(ctr.tolist(), key.tolist(), got.tolist()):
        c, kk = list(row), list(k)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ kk[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ kk[1], p0 & 0xFFFFFFFF]
            kk = [(kk[0] + 0x9E3779B9) & 0xFFFFFFFF, (kk[1] + 0xBB67AE85) & 0xFFFFFFFF]
        assert c == g


def test_box_muller_lanes():
    """(r0, r1) -> lanes 0, 1 as cos, sin; (r2, r3) -> lanes 2, 3; u1 in (0, 1] keeps the log finite at r = 0 and r = 2^32 - 1."""
    n = R.normals(np.arange(250000), 3, 5, 7)
    # 10^6 samples: the mean's standard error is 1e-3, the std's 7e-4; five of each
    assert np.isfinite(n).all() and abs(n.mean()) < 5e-3 and abs(n.std() - 1) < 3.5e-3
    r = R.philox4x32_10(np.array([12, 3, 5, 0], np.uint64), np.array([7, 0], np.uint64)).astype(np.uint64)
    u1, u2 = (float(r[2] >> 8) + 1) / 2 ** 24, float(r[3] >> 8) / 2 ** 24
    want = np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    assert n[12, 3] == pytest.approx(want, abs=1e-15)
    assert np.abs(n).max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12          # 5.77: the largest radius, u1 = 2^-24


@pytest.mark.parametrize("predictor,corrector,n_steps", [("Reverse", "Langevin", 1), ("Reverse", "Langevin", 2), ("Reverse", "None", 1),
                                                         ("S4", "None", 1)])
def test_draw_ids_pairwise_distinct(predictor, corrector, n_steps):
    """Every (step, phase, target) of a 1000-scale plan, plus the prior: pairwise distinct draw ids, all inside 32 bits."""
    per = R.per_step(predictor, n_steps)
    slots = [(None, 0)] + list(itertools.product(range(1000), range(per)))
    ids = {}
    for step, phase in slots:
        for name, t in R.TARGETS.items():
            d = R.draw_base(step, phase, per) + t
            assert 0 <= d < 1 << 32
            assert d not in ids, f"draw id {d} of {(step, phase, name)} is also that of {ids[d]}"
            ids[d] = (step, phase, name)
    assert len(ids) == 3 * (1 + 1000 * per)
    assert sorted(ids) == list(range(3 * (1 + 1000 * per)))                 # dense: no id of the range is left unused either
