"""philox_normal4 forms the Box-Muller radius' uniform u1 = (n + 1) 2^-24, n = r >> 8, as one FMA, fmaf((float)n, 2^-24, 2^-24),
where it used to add, convert and multiply, (float)(n + 1) * 2^-24.  CPU suite: the two forms are the same fp32 number for every one
of the 2^24 values of n, and the host emulation of the kernel source still writes the draws it wrote before the change.

The recorded draws (tests/golden/n1_emu_draws_qm9_CC.npz) come from the emulation library of the commit before the change, built
as tests/emu_util.py builds it: `python -m tests.test_u1_exact OUT.npz` in a checkout of that commit writes them again."""
import os
import sys

import numpy as np

from tests import noise_cases as nc
from tests.helpers import ROOT, make_flags

GOLDEN = os.path.join(ROOT, "tests", "golden", "n1_emu_draws_qm9_CC.npz")
PLAN, COUNTS, SEED, OFFSET, HALF_STEP = "qm9_CC", [9, 5], 0x1234567887654321, (1 << 32) - 1, (0, 0)


def test_fused_u1_is_the_old_u1_for_every_n():
    n = np.arange(1 << 24, dtype=np.uint32)
    inv24 = np.float32(2.0 ** -24)
    old = (n + np.uint32(1)).astype(np.float32) * inv24
    assert old.dtype == np.float32
    # fmaf rounds the exact a b + c once.  In float64 the product of a 24-bit integer and 2^-24 and the sum with 2^-24 are both exact
    # (25 significant bits at most), so rounding that sum to fp32 is what fmaf returns.
    nf = n.astype(np.float32)
    assert np.array_equal(nf.astype(np.uint32), n), "n < 2^24 is not exact in fp32"
    fused = (nf.astype(np.float64) * 2.0 ** -24 + 2.0 ** -24).astype(np.float32)
    assert np.array_equal(fused.view(np.uint32), old.view(np.uint32)), "the fused form differs from the old form"
    assert fused.min() > 0.0 and fused.max() <= 1.0
    assert fused[0] == inv24 and fused[-1] == np.float32(1.0)
    # ... and it is the exact value: no rounding happens in either form
    assert np.array_equal(fused.astype(np.float64), (n.astype(np.float64) + 1.0) * 2.0 ** -24)


def emu_draws(lib):
    eng, _ = nc.engine_for(PLAN, lib, "cpu")
    flags = make_flags(len(COUNTS), eng.N, COUNTS)
    buf = eng.alloc_state(len(COUNTS))
    for t in buf:
        t.fill_(float("nan"))
    eng.noise_draws(flags, HALF_STEP[0], HALF_STEP[1], buf, SEED, OFFSET)
    return {k: t.numpy().copy() for k, t in zip(("x", "adj", "rank2"), buf)}


def test_emu_noise_draws_unchanged():
    from tests.emu_util import emu_library

    got = emu_draws(emu_library())
    want = np.load(GOLDEN)
    for k in ("x", "adj", "rank2"):
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32
        assert np.count_nonzero(want[k]) > want[k].size // 8, f"{k}: the recorded draws are mostly zero"
        diff = int(np.count_nonzero(got[k].view(np.uint32) != want[k].view(np.uint32)))
        assert diff == 0, f"{k}: {diff} of {got[k].size} draws differ bitwise from the recorded ones"


if __name__ == "__main__":
    from tests.emu_util import emu_library

    np.savez(sys.argv[1], **emu_draws(emu_library()))
