"""Cases of the folded batch norm sums (Route::fold_sums: the predictor's k_r2 launch of the fused loop reduces the sums itself, no
k_normsum launch), shared by the host-emulation suite (tests/test_sum_fold.py) and the GPU suite (tests/test_gpu_sum_fold.py, -m gpu).
Every comparison is the folded loop against the same loop of a plan created with CCSD_NO_SUM_FOLD set -- k_normsum as a launch of
its own, the summation order the fold restates -- and asks for equal BITS in the state, the result and the trajectory."""
import os

import torch

from tests.helpers import make_flags
from tests.library_loop_cases import Setup

QM9 = ("ccsd_qm9_CC", "Reverse", "Langevin", 0.2, 0.7)
QM9_BASE = ("ccsd_qm9_Base_CC", "Reverse", "Langevin", 0.2, 0.7)
GRAPH_ONLY = ("gdss_community_small", "Euler", "Langevin", 0.05, 0.7)
COUNTS = [9, 7, 8, 0, 4, 9, 5, 6, 1, 9, 3]      # node counts, cycled over the batch: full, partial, empty and cell-free complexes


def engines(cfg, lib, device, B):
    """(folded engine, engine of a plan created with CCSD_NO_SUM_FOLD, setup) for batch B; the environment is left as it was."""
    su = Setup(cfg[0], lib, device, *cfg[1:])
    old = os.environ.pop("CCSD_NO_SUM_FOLD", None)
    try:
        on = su.engine(B)
        os.environ["CCSD_NO_SUM_FOLD"] = "1"
        off = su.engine(B)
    finally:
        os.environ.pop("CCSD_NO_SUM_FOLD", None)
        if old is not None:
            os.environ["CCSD_NO_SUM_FOLD"] = old
    return on, off, su


def run(eng, flags, first, last, seed=17, traj=False, reduce=None):
    """init_state + PCEngine.run over the steps [first, last) on buffers of its own -> host copies of state + result (+ trajectory)."""
    B = flags.shape[0]
    state, scratch, result = (eng.alloc_state(B) for _ in range(3))
    nt = 3 if eng.is_cc else 2
    tr = None
    if traj:
        per = sum(s[1] * s[2] for s in eng.shapes(B)[:nt])
        tr = torch.zeros(last, per, device=eng.device)       # (the loop writes row `step`)
    eng.init_state(flags, state, None, seed, 0)
    if reduce is None:
        eng.run(flags, state, scratch, result, seed, 0, first, last, tr)
    else:
        eng.run(flags, state, scratch, result, seed, 0, first, last, tr, reduce=reduce)
    out = [t.detach().cpu().clone() for t in list(state[:nt]) + list(result[:nt])]
    if traj:
        out.append(tr.detach().cpu().clone())
    return out


def assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.isfinite(u).all(), f"{what}: tensor {k} is not finite"
        assert torch.equal(u, v), f"{what}: tensor {k} differs (max diff {(u - v).abs().max().item():.3e})"


def case_on_off(cfg, lib, device, B, ranges, traj=False, twice=False):
    """The folded loop == the loop with k_normsum launches over every step range of `ranges`; twice: the folded run repeats itself."""
    on, off, su = engines(cfg, lib, device, B)
    assert on.query("fold_sums") == 1 and off.query("fold_sums") == 0
    assert on.query("fused_loop") == 1 and off.query("fused_loop") == 1
    flags = make_flags(B, su.N, [COUNTS[i % len(COUNTS)] for i in range(B)]).to(device)
    for first, last in ranges:
        got = run(on, flags, first, last, traj=traj)
        assert on.query("fold_last_run") == 1
        want = run(off, flags, first, last, traj=traj)
        assert off.query("fold_last_run") == 0
        assert_same_bits(got, want, f"{cfg[0]} B={B} steps [{first}, {last})")
        assert got[0].abs().sum() > 0
        if twice:
            assert_same_bits(run(on, flags, first, last, traj=traj), got, f"{cfg[0]} B={B} steps [{first}, {last}): second folded run")


def case_reduce_hook_keeps_normsum(cfg, lib, device, B, first, last):
    """With a reduce hook the folded plan launches k_normsum as before (the hook sits between the sums and their readers): the
    query says so, the hook sees the sums once per step, and the bits are those of the folded run."""
    on, off, su = engines(cfg, lib, device, B)
    flags = make_flags(B, su.N, [COUNTS[i % len(COUNTS)] for i in range(B)]).to(device)
    seen = []

    def hook(sums):
        seen.append(sums.detach().cpu().clone())

    hooked = run(on, flags, first, last, reduce=hook)
    assert on.query("fold_sums") == 1 and on.query("fold_last_run") == 0
    assert len(seen) == last - first
    assert all(torch.isfinite(s).all() and (s > 0).all() for s in seen), "the hook did not see k_normsum's six sums"
    folded = run(on, flags, first, last)
    assert on.query("fold_last_run") == 1
    assert_same_bits(hooked, folded, f"{cfg[0]} B={B}: hooked run against the folded one")
    assert_same_bits(run(off, flags, first, last), folded, f"{cfg[0]} B={B}: k_normsum launches against the folded run")


def case_route(lib, device):
    """Which plans fold: the two k_r2 checkpoints of the fused loop do, a graph-only plan does not."""
    for cfg, want in ((QM9, 1), (QM9_BASE, 1), (GRAPH_ONLY, 0)):
        su = Setup(cfg[0], lib, device, *cfg[1:])
        assert su.engine(4).query("fold_sums") == want, cfg[0]
