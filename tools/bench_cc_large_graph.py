"""Throughput of ccsd_grid_small_CC (N = 49, E = 1176, K = 18424) on the tiled graph-network route: ccsd_sampler_run on the MI355X at
the batch and sampler of sample_grid_small_CC.yaml (8 complexes, Reverse + Langevin, snr 0.1, scale_eps 0.7); --arch base_cc: its
ablation twin, the ScoreNetworkA_Base_CC of grid_small_Base_CC.yaml beside the same X and F networks (k_lg_hb_*); --arch cs_h2: a stack
of TWO HodgeAdjAttentionLayers (k_lg_hd_*) -- the community_small geometry (N = 20, E = 190, K = 1140) with qm9_CC.yaml's hodge settings and
seeded weights (tests/hodge_stack_route_cases.py: cs_h2), community_small_CC's sampler; run it with --batch 512.  Prints one JSON line:
complexes/s, ms/step, the time per launch of the graph-network side (launch_lg: the k_lg_* kernels of one pass, the hodge branch among
them) and of the rank-2 kernels (HIP events around every launch, in a run of their own), and the CPU restatement's (oracle) time
for one PC step at the same batch.  bench.py measures the flagship workload; this tool covers a geometry it does not.

    python tools/bench_cc_large_graph.py [--arch cc|base_cc|cs_h2] [--steps 20] [--warmup 3] [--batch 8] [--no-cpu]
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
from oracle import ccsd_oracle as O  # noqa: E402
from tests.helpers import load_ckpt_np, make_flags  # noqa: E402

# tests/golden/ckpt/: the EMA-applied weights sample_grid_small_CC.yaml samples with; the constructed A-network of the Base_CC twin
CKPTS = {"cc": "cc_large/ccsd_grid_small_CC", "base_cc": "base_cc_route/ccsd_grid_small_Base_CC"}
SAMPLER = dict(predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7)
COUNTS = [49, 42, 36, 30, 25, 49, 35, 28]            # node counts of the grid_small training split
CS_COUNTS = [20, 12, 16, 18, 14, 20]                 # ... of community_small's (bench.py's)
NAMES = ("x", "adj", "rank2")
# graph-network side: one launch_lg pass; rank-2 side: layer-0 projection, H = F F^T, ScoreNetworkF, the corrector's apply
KERNELS = {"graph_network_pass": "k_xa", "k_gemm_p": "k_gemm_p", "k_gemm_h": "k_gemm_h", "k_hf_score": "k_hf_score",
           "k_langevin_apply": "k_langevin_apply"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", choices=sorted(CKPTS) + ["cs_h2"], default="cc")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if a.arch == "cs_h2":
        from tests.hodge_stack_route_cases import cs_h2
        meta, parts = cs_h2()
        meta = dict(meta, name="community_small geometry, two hodge layers (qm9_CC's hodge settings, seeded weights)")
    else:
        meta, parts = load_ckpt_np(CKPTS[a.arch])
    cfg = meta["config"]
    d = cfg["data"]
    N, F, d_min, d_max = d["max_node_num"], d["max_feat_num"], d["d_min"], d["d_max"]
    B, dev = a.batch, "cuda:0"
    E, K = rank2_dim(N, d_min, d_max)
    flags = make_flags(B, N, CS_COUNTS if a.arch == "cs_h2" else COUNTS)
    sd = [loader.load_sde(cfg["sde"][p]) for p in NAMES]
    ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], dev) for p in NAMES]
    kw = dict(shape_x=(B, N, F), shape_adj=(B, N, N), shape_rank2=(B, E, K), is_cc=True, d_min=d_min, d_max=d_max, n_steps=1,
              probability_flow=False, continuous=True, denoise=True, eps=1e-4, **SAMPLER)
    fn = solver.get_pc_sampler(sde_x=sd[0], sde_adj=sd[1], sde_rank2=sd[2], device=dev, rng="philox", seed=1, max_steps=a.warmup, **kw)
    dflags = flags.to(dev)
    fn(*ms, dflags)                                            # plan + workspace + warm-up
    eng = fn.engine()
    assert eng.query("large_graph") == 1 and eng.query("r2_family") == 3
    state, scratch, result = (eng.alloc_state(B) for _ in range(3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.init_and_run(dflags, state, scratch, result, 1, 0, 0, a.steps)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    out = {"workload": meta["name"], "N": N, "E": E, "K": K, "batch": B, "sampler": "Reverse+Langevin", "steps": a.steps,
           "complexes_per_s_at_1000_steps": B / (sec / a.steps * 1000.0), "ms_per_step": 1e3 * sec / a.steps,
           "loop_form": eng.query("loop_form")}
    # per-launch split (events around every launch break back-to-back dispatch: not part of the timed run above)
    for k in KERNELS.values():
        eng.profile_kernel(k)
    eng.profile_stride(1)
    eng.init_and_run(dflags, state, scratch, result, 1, 0, 0, a.steps)
    torch.cuda.synchronize()
    split = {}
    for label, k in KERNELS.items():
        n, msec = eng.profile_read(k)
        split[label] = {"launches_per_step": n / a.steps, "ms_per_launch": msec / n if n else None, "ms_per_step": msec / a.steps}
    eng.profile_kernel(None)
    out["split"] = split
    if not a.no_cpu:
        torch.set_num_threads(16)
        x, adj, r2 = (t.cpu() for t in state)
        t0 = time.perf_counter()
        with torch.no_grad():
            for _ in range(2):                                 # norms pass + predictor pass
                for p in NAMES:
                    O.run_network(meta[f"params_{p}"], parts[p], x, adj, r2, flags)
        out["cpu_oracle_s_per_step_16_threads"] = time.perf_counter() - t0
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
