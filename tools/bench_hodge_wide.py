"""Time of one PC step at the qm9 geometry (N = 9, E = 36, K = 466; Reverse + Langevin, snr 0.2, scale_eps 0.7, B = 1024) of a plan with
hodge MLPs wider than 8 -- qm9_CC.yaml's architecture with c_hid_h 8 and num_linears_h 2, seeded weights (tests/hodge_stack_route_cases.py:
arch_at) -- on the tiled graph-network route with the 16-wide hodge kernels, and beside it two yardsticks on the shipped ccsd_qm9_CC
checkpoint: forced onto the same route (CCSD_LARGE_GRAPH=2, read at plan creation), and as it runs unforced (k_xa + k_r2).  DESIGN section 6
quotes the figures.  bench.py measures the flagship workload; this tool covers plans it does not.

A step's time is (T(K2 steps) - T(K1 steps)) / (K2 - K1) of the sampler closure (in-kernel Philox noise), each call synchronised and
preceded by a warm-up call of the same length; the prior draw and the closure's set-up cancel in the difference.  One JSON line per plan
with the time of every repetition and the route the plan took.  Needs an MI355X; --emulate runs the same calls on the host emulation at
B = 4 (a rehearsal of the script: its times mean nothing).

    python tools/bench_hodge_wide.py [--batch 1024] [--k1 10] [--k2 60] [--reps 3] [--emulate]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd import loader, solver  # noqa: E402
from ccsd_amd.plan import rank2_dim  # noqa: E402
from tests import hodge_stack_route_cases as hs  # noqa: E402
from tests.helpers import load_ckpt_np, make_flags  # noqa: E402

NAMES = ("x", "adj", "rank2")
COUNTS = [9] * 12 + [8, 8, 7, 6]          # (bench.py's QM9 histogram, rounded to sixteenths)
QUERIES = ("h_wide", "large_graph", "r2_family", "loop_form", "h_general")


def step_time(tag, meta, parts, force, a, lib, dev, sync):
    if force:
        os.environ["CCSD_LARGE_GRAPH"] = "2"
    else:
        os.environ.pop("CCSD_LARGE_GRAPH", None)
    cfg = meta["config"]
    N, F, d_min, d_max = (cfg["data"][k] for k in ("max_node_num", "max_feat_num", "d_min", "d_max"))
    ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], dev) for p in NAMES]
    sd = [loader.load_sde(cfg["sde"][p]) for p in NAMES]
    B = a.batch
    flags = make_flags(B, N, COUNTS).to(dev)
    kw = dict(shape_x=(B, N, F), shape_adj=(B, N, N), shape_rank2=(B, *rank2_dim(N, d_min, d_max)), predictor="Reverse",
              corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-4,
              is_cc=True, d_min=d_min, d_max=d_max)
    times, eng, out = [], None, None
    for _ in range(a.reps):
        t = {}
        for K in (a.k1, a.k2):
            fn = solver.get_pc_sampler(sde_x=sd[0], sde_adj=sd[1], sde_rank2=sd[2], device=dev, rng="philox", seed=3, max_steps=K,
                                       lib=lib, **kw)
            fn(*ms, flags)                  # warm-up: plan, workspace, code objects
            sync()
            t0 = time.perf_counter()
            out = fn(*ms, flags)
            sync()
            t[K] = time.perf_counter() - t0
            eng = fn.engine()
        times.append((t[a.k2] - t[a.k1]) / (a.k2 - a.k1) * 1e3)
    print(json.dumps({"plan": tag, "batch": B, "ms_per_pc_step": [round(v, 4) for v in times],
                      "route": {k: eng.query(k) for k in QUERIES},
                      "finite": all(bool(torch.isfinite(v).all()) for v in out[:3])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k1", type=int, default=10)
    ap.add_argument("--k2", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--emulate", action="store_true")
    a = ap.parse_args()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, sync = emu_library(), "cpu", (lambda: None)
        a.batch, a.k1, a.k2, a.reps = 4, 1, 2, 1
    else:
        from ccsd_amd import _lib

        assert torch.cuda.is_available(), "tools/bench_hodge_wide.py needs an MI355X (or --emulate for a rehearsal)"
        lib, dev, sync = _lib.get_library(), "cuda:0", torch.cuda.synchronize
    shipped = load_ckpt_np(hs.QM9)
    wide = hs.arch_at(hs.QM9, 9, seed=303, c_hid_h=8, num_linears_h=2)
    step_time("ccsd_qm9_CC as shipped, CCSD_LARGE_GRAPH=2", *shipped, True, a, lib, dev, sync)
    step_time("qm9_CC architecture, c_hid_h 8, num_linears_h 2 (wide)", *wide, False, a, lib, dev, sync)
    step_time("ccsd_qm9_CC as shipped, unforced", *shipped, False, a, lib, dev, sync)


if __name__ == "__main__":
    main()
