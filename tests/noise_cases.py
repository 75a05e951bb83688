"""The device noise stream against tests/philox_ref.py, element by element: what ccsd_init_state and ccsd_noise_draws write, over
plans x sample offsets x seeds x half-steps.  Shared by the CPU suite (host emulation, tests/test_noise.py) and the GPU suite
(tests/test_gpu_noise.py); `lib` / `device` select the backend."""
import numpy as np
import torch

from ccsd_amd import loader
from tests import parity_cases as pc
from tests import philox_ref as R
from tests.helpers import make_flags

# Largest |device draw - float64 Box-Muller of the same Philox words| over the whole grid below (480 calls, every element: about
# 1.1e8 live draws), measured once per backend, and the bound each backend is held to: the measured value times 4 (the error
# grows toward small u1, the tail the grid samples least).  A wrong counter, key, lane or map differs by order 1; the radius is at
# most sqrt(48 ln 2) = 5.77, whose fp32 ulp is 4.8e-7.
#   host emulation (libm logf / sqrtf / sinf / cosf; 2 pi u2 rounded to fp32 before the sine):   2.19e-6 measured (zinc250k_CC_5b)
#   gfx950 (v_log_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32 on u2 in revolutions), on an MI355X:   9.99e-7 measured (community_small_CC,
#                                                                                                zinc250k_CC_5b)
# Both are far below the project's parity tolerance (parity_cases.RTOL = 1e-4).
MEASURED_EMU = 2.19e-6
BOUND_EMU = 4 * MEASURED_EMU
MEASURED_GPU = 9.99e-7
BOUND_GPU = 4 * MEASURED_GPU

# id -> (checkpoint, predictor, corrector, n_steps, predictor draws flat (k_ew1 plan))
PLANS = {
    "qm9_CC": ("ccsd_qm9_CC", "Reverse", "Langevin", 1, False),                          # E = 36, K = 466
    "community_small_CC": ("ccsd_community_small_CC", "Euler", "Langevin", 1, False),    # E = 190: the last row group is partial
    "enzymes_small_CC_S4": ("ccsd_enzymes_small_CC", "S4", "None", 1, False),            # K = 715 odd, E K % 4 = 2
    "zinc250k_CC_5b": ("zinc250k_CC_5b", "Reverse", "Langevin", 1, True),                # k_ew1: flat predictor draws
    "gdss_community_small": ("gdss_community_small", "Euler", "Langevin", 1, False),     # no rank-2 tensor
    "qm9_CC_nsteps2": ("ccsd_qm9_CC", "Reverse", "Langevin", 2, False),
}
OFFSETS = [0, 7, (1 << 32) - 2, (1 << 40) + 3]          # 2^32 - 2: the low counter word wraps inside the batch
SEEDS = [0, 1, 1 << 32, (1 << 64) - 1]
B = 5
DIFF_STEPS = 1000
_engines = {}


def counts_for(N):
    return [N, 0, 1, 2, N - 3]


def half_steps(plan):
    """(step, phase) pairs of a plan: (0, 0), (0, last), (999, last); every phase of both steps for S4 and n_steps = 2."""
    _, predictor, _, n_steps, _ = PLANS[plan]
    per = R.per_step(predictor, n_steps)
    if predictor == "S4" or n_steps > 1:
        return [(s, p) for s in (0, DIFF_STEPS - 1) for p in range(per)]
    return [(0, 0), (0, per - 1), (DIFF_STEPS - 1, per - 1)]


def engine_for(plan, lib, device):
    key = (plan, id(lib), str(device))
    if key not in _engines:
        name, predictor, corrector, n_steps, ew1 = PLANS[plan]
        meta, _ = pc.load_ckpt_np(name)
        names = ["x", "adj"] + (["rank2"] if meta["is_cc"] else [])
        sdes = [loader.load_sde(dict(meta["config"]["sde"][p], num_scales=DIFF_STEPS)) for p in names]
        eng, meta, _ = pc.engine_from_ckpt(name, lib, device, sdes=sdes, predictor=predictor, corrector=corrector, snr=0.1,
                                           scale_eps=0.7, n_steps=n_steps)
        assert eng.query("ew1") == int(ew1), f"{plan}: ew1 = {eng.query('ew1')}"
        _engines[key] = (eng, meta)
    return _engines[key]


def is_flat(plan, phase):
    """Which map the rank-2 draw of a half-step takes: flat for Langevin corrector draws and for the predictor draws of k_ew1 plans."""
    _, predictor, corrector, n_steps, ew1 = PLANS[plan]
    if predictor == "S4":
        return False
    if corrector == "Langevin" and phase < n_steps:
        return True
    return ew1


def check_draws(got, want, masks, flags, what, bound):
    """Every element of one call: masked entries and the adj diagonal exactly 0, adj bit-symmetric, values within `bound` of the
    reference.  Returns the largest distance."""
    worst = 0.0
    names = ["x", "adj", "rank2"]
    for p, g, w, m in zip(names, got, want, masks):
        if w is None:
            continue
        g = g.detach().cpu().numpy()
        assert g.shape == w.shape and g.dtype == np.float32, (what, p, g.shape, w.shape)
        assert np.isfinite(g).all(), f"{what} {p}: non-finite draws"
        dead = m == 0.0
        assert not g[dead].any(), f"{what} {p}: {int(np.count_nonzero(g[dead]))} masked entries are not exactly 0"
        if p == "adj":
            assert np.array_equal(g.view(np.uint32), g.transpose(0, 2, 1).view(np.uint32)), f"{what}: adj is not bit-symmetric"
            assert not g[:, np.arange(g.shape[1]), np.arange(g.shape[1])].any(), f"{what}: adj diagonal is not 0"
        for b in range(g.shape[0]):                     # (sample by sample: the float64 copies of a large rank2 stay small)
            err = float(np.abs(g[b].astype(np.float64) - w[b]).max())
            assert err <= bound, f"{what} {p}[{b}] (nodes {int(flags[b].sum())}): max |device - reference| = {err:.3e} > {bound:.3e}"
            worst = max(worst, err)
    return worst


def slots(plan):
    """The calls of a plan: the prior (None) and its half-steps."""
    return [None] + half_steps(plan)


def slot_id(hs):
    return "prior" if hs is None else "s%dp%d" % hs


def case_stream(plan, lib, device, seed, sample_offset, hs, bound, flags=None):
    """One call -- the prior (hs None) or half-step hs = (step, phase) -- at one (seed, sample_offset), B = 5 with node counts
    [N, 0, 1, 2, N - 3]: every element against the reference.  `flags`: a (B, N) node mask of the caller's (default: those counts,
    the live nodes a prefix).  Returns the largest distance."""
    eng, meta = engine_for(plan, lib, device)
    _, predictor, _, n_steps, _ = PLANS[plan]
    N, F, is_cc = eng.N, eng.F, eng.is_cc
    d = meta["config"]["data"]
    d_min, d_max = (d["d_min"], d["d_max"]) if is_cc else (0, 0)
    if flags is None:
        flags = make_flags(B, N, counts_for(N))
    assert tuple(flags.shape) == (B, N)
    dflags = flags.to(device)
    buf = eng.alloc_state(B)
    for t in buf:
        if t is not None:
            t.fill_(float("nan"))                       # every element must be written by the call
    if hs is None:
        eng.init_state(dflags, buf, None, seed, sample_offset)
        base, flat = 0, False
    else:
        eng.noise_draws(dflags, hs[0], hs[1], buf, seed, sample_offset)
        base, flat = R.draw_base(hs[0], hs[1], R.per_step(predictor, n_steps)), is_flat(plan, hs[1])
    want, masks = R.masked_draws(flags, N, F, is_cc, d_min, d_max, base, seed, sample_offset, flat)
    what = f"{plan} seed {seed:#x} offset {sample_offset:#x} {slot_id(hs)}"
    worst = check_draws(buf, want, masks, flags, what, bound)
    print(f"noise stream {what}: max |device - float64 reference| = {worst:.3e}")
    return worst


def case_offset_tiling(plan, lib, device):
    """sample_offset tiles the stream across the 2^32 boundary: a batch of 3 at offset s + 2 is, bit for bit, rows 2.. of the batch
    of 5 at offset s = 2^32 - 2 (equal flags in every slot: only the global sample index tells the rows apart), and differs from
    the batch at s + 2 - 2^32 (a truncated offset)."""
    eng, _ = engine_for(plan, lib, device)
    s = (1 << 32) - 2
    flags5 = torch.ones(5, eng.N, device=device)
    nt = 3 if eng.is_cc else 2
    for hs in slots(plan)[:3]:
        outs = []
        for nb, off in ((5, s), (3, s + 2), (3, 0)):
            buf = eng.alloc_state(nb)
            if hs is None:
                eng.init_state(flags5[:nb], buf, None, 3, off)
            else:
                eng.noise_draws(flags5[:nb], hs[0], hs[1], buf, 3, off)
            outs.append([t.cpu() for t in buf[:nt]])
        for a, b, c in zip(*outs):
            assert torch.equal(a[2:], b), f"{plan} {hs}: rows 2.. at offset 2^32 - 2 != the batch at offset 2^32"
            assert not torch.equal(b, c), f"{plan} {hs}: offset 2^32 draws the stream of offset 0"
