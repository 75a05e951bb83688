"""Throughput of the tiled graph-network route (graph-only plans above 64 nodes): ccsd_sampler_run on the MI355X for the two shipped
checkpoints it serves, at their reference sampling batches and samplers.  Prints one JSON line per workload: complexes/s, ms/step,
as-written GFLOP per forward (from the shapes), achieved TFLOP/s, and the CPU restatement's (oracle) time for one step at the same
batch.  bench.py measures the flagship workload; this tool covers the route it does not.

    python tools/bench_large_graph.py [--steps 1000] [--warmup 20] [--only gdss_enzymes] [--no-cpu]
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
from oracle import ccsd_oracle as O  # noqa: E402
from tests.helpers import load_ckpt_np, make_flags  # noqa: E402

# name -> (batch, sampler of the checkpoint's sample_*.yaml, node counts cycled over the batch)
WORKLOADS = {
    "gdss_enzymes": (64, dict(predictor="S4", corrector="None", snr=0.15, scale_eps=0.7), [125, 96, 64, 37]),
    "gdss_grid": (8, dict(predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7), [361, 324, 256, 196]),
}


def forward_gflop(px, pa, N, F):
    """As-written multiply-adds x 2 of one ScoreNetworkX + ScoreNetworkA forward of one graph (reference formulation)."""
    H, depth = px["nhid"], px["depth"]
    xf = F + depth * H
    fx = sum(2 * N * (F if l == 0 else H) * H + 2 * N * N * H for l in range(depth))
    fx += 2 * N * (xf * 2 * xf + 2 * xf * 2 * xf + 2 * xf * F)
    L, ci, ch, cf, nh, ad, nl = (pa[k] for k in ("num_layers", "c_init", "c_hid", "c_final", "nhid", "adim", "num_linears"))
    fa = (ci - 1) * 2 * N ** 3
    fdim = ci + (L - 1) * ch + cf
    for l in range(L):
        cin, cout = (ci if l == 0 else ch), (cf if l == L - 1 and l else ch)
        fin, a = (F if l == 0 else nh), (nh if l == 0 else ad)
        hid = 2 * max(cin, cout)
        per = 2 * N * fin * (2 * a + nh) + 2 * N * N * (2 * a + nh) + 2 * N * N * a       # Q | K | V, the adjacency GEMMs, Q K^T
        fa += cin * per + 2 * N * (cin * nh * hid + hid * nh)                             # + multi_channel
        fa += 2 * N * N * (2 * cin * hid + (nl - 2) * hid * hid + hid * cout)             # edge MLP
    fa += 2 * N * N * (fdim * 2 * fdim + 2 * fdim * 2 * fdim + 2 * fdim)                  # final MLP
    return fx / 1e9, fa / 1e9


def run(name, steps, warmup, cpu):
    B, smp, counts = WORKLOADS[name]
    meta, parts = load_ckpt_np(name)
    cfg = meta["config"]
    N, F = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"]
    dev = "cuda:0"
    flags = make_flags(B, N, counts)
    sd = [loader.load_sde(cfg["sde"][p]) for p in ("x", "adj")]
    ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], dev) for p in ("x", "adj")]
    kw = dict(shape_x=(B, N, F), shape_adj=(B, N, N), n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-4, **smp)
    make = solver.S4_solver if smp["predictor"] == "S4" else solver.get_pc_sampler
    fn = make(sde_x=sd[0], sde_adj=sd[1], device=dev, rng="philox", seed=1, max_steps=steps, **kw)
    dflags = flags.to(dev)
    fn(*ms, dflags)                                            # plan + workspace
    eng = fn.engine()
    assert eng.query("large_graph") == 1
    state, scratch, result = (eng.alloc_state(B) for _ in range(3))
    eng.init_and_run(dflags, state, scratch, result, 1, 0, 0, warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.init_and_run(dflags, state, scratch, result, 1, 0, 0, steps)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    gx, ga = forward_gflop(meta["params_x"], meta["params_adj"], N, F)
    per_step = 2 if smp["corrector"] == "Langevin" else 1      # network forwards per step (norms pass + predictor, or the S4 pass)
    out = {"workload": name, "N": N, "batch": B, "sampler": f"{smp['predictor']}+{smp['corrector']}", "steps": steps,
           "complexes_per_s": B / (sec * 1000.0 / steps), "ms_per_step": 1e3 * sec / steps,
           "gflop_per_forward": {"x": round(gx, 4), "adj": round(ga, 4)},
           "tflops": per_step * B * (gx + ga) * steps / sec / 1e3}
    if cpu:
        torch.set_num_threads(16)
        x = torch.randn(B, N, F) * flags[:, :, None]
        a = torch.randn(B, N, N).triu(1)
        a = (a + a.transpose(1, 2)) * flags[:, :, None] * flags[:, None, :]
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(per_step):
                for p in ("x", "adj"):
                    O.run_network(meta[f"params_{p}"], parts[p], x, a, None, flags)
        out["cpu_oracle_s_per_step_16_threads"] = time.perf_counter() - t0
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    for name in WORKLOADS:
        if a.only in (None, name):
            run(name, a.steps, a.warmup, not a.no_cpu)


if __name__ == "__main__":
    main()
