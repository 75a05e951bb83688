"""Time of the lifting of graphs to combinatorial complexes on the device (SampleOps.lift: k_lift_paths / k_lift_cycles, k_lift_dense):

    paths    1024 graphs at N = 20 and N = 49 (d = 3; mean degree about 4, seeded), the sparse outputs alone and with the dense incidence tensor
    cycles   1024 graphs at N = 12 (d 3..4) and N = 18 (d 3..5), edge probability 0.2

The dense tensor is E K floats per graph: 0.87 MB at N = 20, 86.7 MB at N = 49, so the dense N = 49 line runs --dense-graphs graphs (64:
5.5 GB) instead of 1024 (89 GB).  The device figure is the whole Python call (allocation of the outputs included), timed between two HIP
events after a warm-up: `--repeats` windows of about `--window` seconds each (sized from one call's time), the median and the spread of the
per-call means.  The outputs of the first --check graphs are compared with the Python restatement (tests/lift_ref.py) before timing.
Beside it stands that restatement of the same rule over the same graphs on --threads processes of the machine at hand, timed once: a plain
Python enumeration, context and not a ratio.  One JSON line per workload (appended to --out when given); without an MI355X the device
figures read "not measured".  --emulate runs the device side on the host emulation at 8 graphs (a rehearsal of the script: its times mean
nothing).

    python tools/bench_lift.py [--n 1024] [--out profiles/r20_lift_bench.jsonl] [--emulate]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd import evaluation as ev  # noqa: E402
from tests import lift_ref as lr  # noqa: E402
from tools.bench_orbit import device_ms  # noqa: E402


def graphs(n, N, p, seed):
    rng = np.random.default_rng(seed)
    u = np.triu(rng.random((n, N, N)) < p, 1)
    return (u | u.transpose(0, 2, 1)).astype(np.float32)


def workloads(n, dense_graphs):
    """(tag, procedure, adjacency (B, N, N) float32, d_min, d_max, dense)."""
    out = []
    for N in (20, 49):
        adj = graphs(n, N, 4.0 / (N - 1), N)
        out.append((f"paths_n{N}", "path_based", adj, 3, 3, False))
        out.append((f"paths_n{N}_dense", "path_based", adj if N == 20 else adj[:dense_graphs], 3, 3, True))
    out.append(("cycles_n12", "cycles", graphs(n, 12, 0.2, 12), 3, 4, False))
    out.append(("cycles_n18", "cycles", graphs(n, 18, 0.2, 18), 3, 5, False))
    return out


def _host_chunk(args):
    adj, proc, d_min, d_max = args
    r = lr.lift(adj, proc, d_min, d_max)
    return int(r["rank2_cell_count"].sum()), int(r["lift_dropped"].sum())


def host_seconds(adj, proc, d_min, d_max, threads):
    """The restatement over all graphs on `threads` processes (sparse outputs only), timed once -> (seconds, cells, dropped)."""
    chunks = [(c, proc, d_min, d_max) for c in np.array_split(adj, min(threads * 4, len(adj))) if len(c)]
    t0 = time.perf_counter()
    with ProcessPoolExecutor(threads) as ex:
        parts = list(ex.map(_host_chunk, chunks))
    return time.perf_counter() - t0, sum(p[0] for p in parts), sum(p[1] for p in parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--dense-graphs", type=int, default=64)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulate", action="store_true")
    a = ap.parse_args()
    lib, dev, gpu = None, "cuda:0", torch.cuda.is_available()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, gpu, a.n, a.dense_graphs = emu_library(), "cpu", False, 8, 2
    run = gpu or a.emulate
    name = torch.cuda.get_device_name(0) if gpu else ("host emulation" if a.emulate else None)
    eng = ev._ops(dev, lib) if run else None
    lines = []
    for tag, proc, adj, d_min, d_max, dense in workloads(a.n, a.dense_graphs):
        B, N = adj.shape[:2]
        K = lr.n_columns(N, d_min, d_max)
        rec = {"workload": "lift", "set": tag, "procedure": proc, "graphs": B, "N": N, "d_min": d_min, "d_max": d_max, "K": K, "dense": dense,
               "mean_degree": round(float(adj.sum() / (B * N)), 2), "device": name, "device_ms": "not measured"}
        if dense:
            rec["dense_bytes"] = B * (N * (N - 1) // 2) * K * 4
        if run:
            t = torch.from_numpy(adj).to(dev)
            got = eng.lift(t, proc, d_min=d_min, d_max=d_max, dense=dense)
            nchk = min(a.check, B)
            want = lr.lift(adj[:nchk], proc, d_min, d_max, dense=dense and N <= 20)
            for k, v in want.items():
                g = got[k][:nchk].cpu().numpy()
                assert np.array_equal(g.view(np.uint64) if k == "rank2_cell_bits" else g, v), (tag, k)
            if dense:
                assert int(got["rank2"].sum().item()) == int(got["rank2_nnz"].sum().item()), tag
            del got
            (med, lo, hi), iters = device_ms(lambda: eng.lift(t, proc, d_min=d_min, d_max=d_max, dense=dense), a.window, a.repeats, gpu)
            rec.update(device_ms=round(med, 4), device_ms_min=round(lo, 4), device_ms_max=round(hi, 4), calls_per_window=iters, windows=a.repeats,
                       graphs_per_s=round(B / (med * 1e-3), 1))
            if dense:
                rec["dense_GBps"] = round(rec["dense_bytes"] / (med * 1e-3) / 1e9, 1)
        if not dense:
            sec, cells, dropped = host_seconds(adj, proc, d_min, d_max, a.threads)
            rec["host_restatement"] = {"label": "tests/lift_ref.py (plain Python) over the same graphs on the machine at hand, timed once",
                                       "processes": a.threads, "seconds": round(sec, 3)}
            rec.update(cells=cells, dropped=dropped)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
