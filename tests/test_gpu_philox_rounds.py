"""GPU suite (-m gpu): the Philox rounds of the kernels against tests/philox_ref.py where the split of the first rounds between the
scalar and the vector ALU can go wrong.  Of the counter (group, low32(b), draw, high32(b)) only the group differs between the lanes
of a wave, so the compiler runs the uniform halves of rounds 1-2 on the scalar ALU, and philox4 (ccsd_dev.h) sums three per-lane
terms in one three-input instruction only from the round at which all three are per-lane.  The cases put every uniform word at both
ends of its range: sample offsets 0, 2^32 - 1 and 2^32 (the high word becomes non-zero, and inside a batch of 2 at 2^32 - 1 it
differs between the two workgroups of one launch) and draw indices 0 and 2^32 - 1 (adj and rank2 then take the wrapped 0 and 1), at
N = 4 for one complex and for a batch of 2, both element -> group maps of the rank-2 draw.  ccsd_noise_draws_at runs k_init_state, i.e.
form 1 of ccsd_dev.h (three-input sums, pinned running keys); the last test takes form 2 (k_r2's units: the multiply's carry-out in VCC)
to the same sample offsets by holding k_r2's in-kernel draws to the exported ones, bit for bit.

As in tests/test_gpu_noise.py the masked entries and the adj diagonal are exactly 0, adj is bit-symmetric, and the live draws lie
within noise_cases.BOUND_GPU of the float64 Box-Muller of the reference's Philox words (a wrong word differs by order 1)."""
import pytest
import torch

from tests import noise_cases as nc
from tests import parity_cases as pc
from tests import philox_ref as R
from tests.helpers import make_flags

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 4
SEED = 0x9E3779B97F4A7C15
OFFSETS = [0, (1 << 32) - 1, 1 << 32]
DRAWS = [0, (1 << 32) - 1]
COUNTS = {1: [4], 2: [4, 3]}
GEOMETRY = {"max_node_num": N, "d_min": 3, "d_max": 4}          # E = 6 edges, K = 4 + 1 = 5 cells: E K % 4 = 2, a ragged last flat group
_engine = {}


def engine(lib, device):
    """qm9_CC's architecture at N = 4 nodes, no weights loaded (the draws depend on the plan's shapes only)."""
    key = (id(lib), device)
    if key not in _engine:
        from ccsd_amd.engine import PCEngine

        meta, _ = pc.load_ckpt_np("ccsd_qm9_CC")
        d = meta["config"]["data"]
        at_n = lambda p: dict(p, **{k: v for k, v in GEOMETRY.items() if k in p})      # (layers whose widths follow the geometry)
        eng = PCEngine(at_n(meta["params_x"]), None, at_n(meta["params_adj"]), None, at_n(meta["params_rank2"]), None, N=N,
                       F=d["max_feat_num"], is_cc=True, d_min=GEOMETRY["d_min"], d_max=GEOMETRY["d_max"], device=device, lib=lib)
        _engine[key] = (eng, GEOMETRY["d_min"], GEOMETRY["d_max"])
    return _engine[key]


def case_draws_at(lib, device, B, sample_offset, draw, flat, bound):
    eng, d_min, d_max = engine(lib, device)
    assert eng.E > 0 and eng.K > 0
    flags = make_flags(B, N, COUNTS[B])
    dflags = flags.to(device)
    buf = eng.alloc_state(B)
    for t in buf:
        t.fill_(float("nan"))                          # every element must be written by the call
    eng.noise_draws_at(dflags, draw, flat, buf, SEED, sample_offset)
    want, masks = R.masked_draws(flags, N, eng.F, True, d_min, d_max, draw, SEED, sample_offset, flat)
    what = f"N {N} B {B} offset {sample_offset:#x} draw {draw:#x} flat {int(flat)}"
    worst = nc.check_draws(buf, want, masks, flags, what, bound)
    print(f"philox rounds {what}: max |device - float64 reference| = {worst:.3e}")
    if draw == 0 and not flat:                         # the prior is this call
        prior = eng.alloc_state(B)
        eng.init_state(dflags, prior, None, SEED, sample_offset)
        for a, b in zip(buf, prior):
            assert torch.equal(a, b), f"{what}: ccsd_init_state differs from draw index 0"
    return worst


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("flat", [False, True], ids=["rows", "flat"])
@pytest.mark.parametrize("draw", DRAWS, ids=lambda v: f"draw{v:#x}")
@pytest.mark.parametrize("sample_offset", OFFSETS, ids=lambda v: f"off{v:#x}")
@pytest.mark.parametrize("B", [1, 2], ids=["one", "batch2"])
def test_rounds_vs_reference(lib, B, sample_offset, draw, flat):
    case_draws_at(lib, DEV, B, sample_offset, draw, flat, nc.BOUND_GPU)


def case_k_r2_draws_in_kernel_vs_supplied(lib, device, sample_offset):
    """The fused rank-2 kernel k_r2 draws inside the kernel (its own translation units: the multiply's carry-out in VCC, form 2 of
    ccsd_dev.h); ccsd_noise_draws exports the same masked draws through k_init_state (form 1), held to the reference above and in
    tests/test_gpu_noise.py.  One predictor half-step and one corrector norms pass of qm9_CC (B = 2, node counts [9, 5]) with NULL
    noise must equal, bit for bit, the same calls fed the exported draws: the kernel multiplies a supplied draw by its 0 / 1 mask
    once more, which changes no bit, and everything else is the same arithmetic in the same order."""
    eng, _ = nc.engine_for("qm9_CC", lib, device)
    assert eng.query("fused_r2") == 1
    B, seed = 2, SEED
    flags = make_flags(B, eng.N, [9, 5]).to(device)
    state = eng.alloc_state(B)
    eng.init_state(flags, state, None, seed, sample_offset)
    n_steps = 1
    for phase, what in ((n_steps, "predictor"), (0, "corrector norms")):
        draws = eng.alloc_state(B)
        eng.noise_draws(flags, 0, phase, draws, seed, sample_offset)
        outs = []
        for noise in (None, draws):
            if phase == n_steps:
                out = eng.alloc_state(B)
                eng.predictor(0, state, flags, noise, seed, sample_offset, out)
                outs.append([t.cpu() for t in out])
            else:
                sums = torch.zeros(6, device=device)
                eng.corrector_norms(0, 0, state, state, flags, noise, seed, sample_offset, sums)
                outs.append([sums.cpu()])
        for a, b in zip(*outs):
            assert torch.isfinite(a).all() and a.abs().sum() > 0
            assert torch.equal(a, b), f"{what} at offset {sample_offset:#x}: in-kernel draws differ from the exported ones"


@pytest.mark.parametrize("sample_offset", OFFSETS, ids=lambda v: f"off{v:#x}")
def test_k_r2_draws_in_kernel_vs_supplied(lib, sample_offset):
    case_k_r2_draws_in_kernel_vs_supplied(lib, DEV, sample_offset)
