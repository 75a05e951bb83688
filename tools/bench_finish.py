"""Time of the finish of one sampled chunk -- everything Sampler.sample() does to the final tensors -- through the one-call path
(SampleOps.finish: k_finish_graph + k_finish_rank2) against the three-call sequence it replaces (quantize(adj), quantize(rank2).to(uint8),
rank2_cells(rank2)), in the same process on the same tensors, at three shapes:

    qm9_CC                     N =  9, d 3..9  (E =  36, K =   466), B = 1024
    community_small_CC         N = 20, d 3     (E = 190, K =  1140), B =  512
    zinc250k_CC substitute     N = 38, d 3     (E = 703, K =  8436), B =  256   (1.5e9 rank-2 entries: 6 GB of state)

Each figure is the mean of `--iters` back-to-back calls between two HIP events, after a warm-up of both paths; the two paths alternate
`--reps` times and every repetition is printed.  The rank-2 pass is also timed alone (dense output, bitmask and counts; no graph pass) and
its achieved rate is given against the 5 bytes per entry it has to move (4 read, 1 written).  One JSON line per shape; the outputs of the two
paths are compared once per shape before timing.  DESIGN section 6 quotes the figures.  bench.py measures the flagship workload; this tool
covers what follows its loop.  Needs an MI355X; --emulate runs the same calls on the host emulation at B = 2 (a rehearsal of the script: its
times mean nothing).

    python tools/bench_finish.py [--reps 5] [--iters 20] [--shapes qm9_CC,community_small_CC,zinc250k_CC] [--emulate]
"""
import argparse
import json
import os
import sys
import time
from math import comb

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd.samples import SampleOps  # noqa: E402

SHAPES = {       # name -> (B, N, F, d_min, d_max, molecule)
    "qm9_CC": (1024, 9, 4, 3, 9, True),
    "community_small_CC": (512, 20, 11, 3, 3, False),
    "zinc250k_CC": (256, 38, 9, 3, 3, True),
}


def three_calls(eng, adj, rank2, mol):
    """The finish of Sampler.sample() before ccsd_finish."""
    adj_int = eng.quantize(adj, -1.0 if mol else 0.5)
    rank2_int = eng.quantize(rank2, 0.5).to(torch.uint8)
    bits, counts = eng.rank2_cells(rank2, 0.5)
    return {"adj_int": adj_int, "rank2_int": rank2_int, "rank2_cell_bits": bits, "rank2_cell_count": counts}


def timed(fn, iters, gpu):
    if not gpu:
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) / iters * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def bench(name, a, lib, dev, gpu):
    B, N, F, d_min, d_max, mol = SHAPES[name]
    if not gpu:
        B = 2
    E, K = N * (N - 1) // 2, sum(comb(N, d) for d in range(d_min, d_max + 1))
    gen = torch.Generator(device=dev).manual_seed(11)
    # the value range of finished samples: most incidence entries below the threshold, adjacency spread over the four bond bins
    x = torch.rand((B, N, F), device=dev, generator=gen)
    adj = torch.rand((B, N, N), device=dev, generator=gen) * 3.2
    rank2 = torch.rand((B, E, K), device=dev, generator=gen) * 0.56
    eng = SampleOps(dev, lib)
    new = lambda: eng.finish(x, adj, rank2, None, mol=mol, d_min=d_min, d_max=d_max)
    old = lambda: three_calls(eng, adj, rank2, mol)
    r2 = lambda: eng.finish(None, adj, rank2, None, mol=mol, d_min=d_min, d_max=d_max, dense_adj=False, descriptors=False)
    got, want = new(), old()                                     # (also the warm-up of both paths)
    same = all(torch.equal(got[k], want[k]) for k in want)
    del got, want
    r2()
    t_new, t_old, t_r2 = [], [], []
    for _ in range(a.reps):
        t_old.append(timed(old, a.iters, gpu))
        t_new.append(timed(new, a.iters, gpu))
        t_r2.append(timed(r2, a.iters, gpu))
    n = B * E * K
    best = min(t_r2)
    print(json.dumps({"shape": name, "B": B, "E": E, "K": K, "rank2_entries": n, "outputs_equal": same,
                      "three_calls_ms": [round(v, 4) for v in t_old], "finish_ms": [round(v, 4) for v in t_new],
                      "ratio_three_calls_over_finish": round(min(t_old) / min(t_new), 3),
                      "rank2_pass_ms": [round(v, 4) for v in t_r2],
                      "rank2_pass_bytes_per_s_at_5B_per_entry": round(5.0 * n / (best * 1e-3), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--emulate", action="store_true")
    a = ap.parse_args()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, gpu = emu_library(), "cpu", False
        a.reps, a.iters = 1, 1
    else:
        from ccsd_amd import _lib

        assert torch.cuda.is_available(), "tools/bench_finish.py needs an MI355X (or --emulate for a rehearsal)"
        lib, dev, gpu = _lib.get_library(), "cuda:0", True
    for name in a.shapes.split(","):
        bench(name, a, lib, dev, gpu)


if __name__ == "__main__":
    main()
