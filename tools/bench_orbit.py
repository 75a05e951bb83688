"""Time of the orbit counts on the device (SampleOps.orbit_counts: k_orbit_counts, one launch):

    sparse   1024 graphs at N = 9, 20 and 125, mean degree about 4 (seeded)
    dense    one complete graph on 512 nodes (the largest graph the kernel takes, at its worst case)

The device figure is the whole call (the per-graph sums and node counts; no per-node rows), timed between two HIP events after a warm-up:
`--repeats` windows of about `--window` seconds each (sized from one call's time), the median and the spread of the per-call means.  The counts are checked
against a numpy restatement of three orbits (edges, 3-path middles, triangles) before timing.  One JSON line per workload (appended to
--out when given); without an MI355X the device figures read "not measured".  --emulate runs the device side on the host emulation at
8 graphs (a rehearsal of the script: its times mean nothing).

What stood here before is the reference's way: the orca program, one process and one temporary edge list per graph (evaluation/stats.py:
343-379).  --orca BIN times exactly that over the same graphs ONCE on the machine at hand and writes --host-file; a later run copies
those figures into its lines under "host_orca", labelled as host numbers of another machine.  They are context, not a ratio.

    python tools/bench_orbit.py [--n 1024] [--out profiles/r16_orbit_bench.jsonl] [--emulate]
    python tools/bench_orbit.py --orca /path/to/orca          # host figures only -> profiles/r16_orbit_host_orca.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd import evaluation as ev  # noqa: E402

HOST_FILE = os.path.join(ROOT, "profiles", "r16_orbit_host_orca.json")


def workloads(n):
    """(tag, adjacency (B, N, N) float32)."""
    out = []
    for N in (9, 20, 125):
        rng = np.random.default_rng(N)
        u = np.triu(rng.random((n, N, N)) < 4.0 / (N - 1), 1)
        out.append((f"sparse_n{N}", (u | u.transpose(0, 2, 1)).astype(np.float32)))
    out.append(("dense_k512", (1 - np.eye(512, dtype=np.float32))[None]))
    return out


def restated(adj):
    """orbits 0, 2 and 3 per graph in numpy: sum d, sum C(d, 2) - t, sum t."""
    A = adj.astype(np.int64)
    d = A.sum(-1)
    t = (A * (A @ A)).sum(-1) // 2
    return d.sum(-1), (d * (d - 1) // 2 - t).sum(-1), t.sum(-1)


def orca_seconds(binary, adj):
    """The reference's call per graph: write `nodes edges` and the edge list of the nodes that have an edge, run `orca node 4 file std`."""
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "g.txt")
        for a in adj:
            keep = np.nonzero(a.sum(1) > 0)[0]
            idx = {int(v): i for i, v in enumerate(keep)}
            ii, jj = np.nonzero(np.triu(a, 1))
            with open(path, "w") as f:
                f.write(f"{max(len(keep), 1)} {len(ii)}\n" + "".join(f"{idx[int(i)]} {idx[int(j)]}\n" for i, j in zip(ii, jj)))
            subprocess.check_output([binary, "node", "4", path, "std"])
    return time.perf_counter() - t0


def device_ms(fn, window, repeats, gpu):
    """Per-call milliseconds: [median, min, max] over `repeats` windows of about `window` seconds, after a warm-up call."""
    fn()
    if not gpu:
        t0 = time.perf_counter()
        fn()
        return [(time.perf_counter() - t0) * 1e3] * 3, 1
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    iters = int(min(max(window * 1e3 / max(a.elapsed_time(b), 1e-3), 1), 20000))
    means = []
    for _ in range(repeats):
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        means.append(a.elapsed_time(b) / iters)
    return [float(np.median(means)), min(means), max(means)], iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulate", action="store_true")
    ap.add_argument("--orca", default=None)
    ap.add_argument("--host-file", default=HOST_FILE)
    a = ap.parse_args()
    if a.orca:
        host = {"what": "the reference's orbit counter, one process and one edge-list file per graph, timed once", "graphs": a.n,
                "cpu": next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown")}
        for tag, adj in workloads(a.n):
            host[tag] = {"graphs": len(adj), "seconds": round(orca_seconds(a.orca, adj), 3)}
            print(tag, host[tag], flush=True)
        with open(a.host_file, "w") as f:
            json.dump(host, f, indent=1)
        return
    lib, dev, gpu = None, "cuda:0", torch.cuda.is_available()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, gpu, a.n = emu_library(), "cpu", False, 8
    run = gpu or a.emulate
    name = torch.cuda.get_device_name(0) if gpu else ("host emulation" if a.emulate else None)
    eng = ev._ops(dev, lib) if run else None
    host = json.load(open(a.host_file)) if os.path.exists(a.host_file) else {}
    lines = []
    for tag, adj in workloads(a.n):
        B, N = adj.shape[:2]
        rec = {"workload": "orbit_counts", "set": tag, "graphs": B, "N": N, "mean_degree": round(float(adj.sum() / (B * N)), 2), "device": name,
               "device_ms": "not measured"}
        if run:
            t = torch.from_numpy(adj).to(dev)
            got = eng.orbit_counts(t)["orbit_counts"].cpu().numpy()
            want = restated(adj)
            assert all(np.array_equal(got[:, k], w) for k, w in zip((0, 2, 3), want)), tag
            (med, lo, hi), iters = device_ms(lambda: eng.orbit_counts(t), a.window, a.repeats, gpu)
            rec.update(device_ms=round(med, 4), device_ms_min=round(lo, 4), device_ms_max=round(hi, 4), calls_per_window=iters,
                       windows=a.repeats, graphs_per_s=round(B / (med * 1e-3), 1), orbit14_total=int(got[:, 14].sum()))
        if tag in host and host[tag]["graphs"] == B:
            rec["host_orca"] = {"label": "host numbers from another machine: the reference's orca program, one process per graph, timed once",
                                "cpu": host.get("cpu"), "seconds": host[tag]["seconds"]}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
