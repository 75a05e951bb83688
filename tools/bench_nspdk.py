"""Time of the NSPDK score on the device (SampleOps.nspdk_features: k_nspdk_features and the CSR compaction; SampleOps.nspdk_mmd: three
small kernels):

    mol_n9, mol_n38   1024 seeded molecule-like graphs (a tree plus a few chords, degree <= 4, bond orders 1..3, four or six labels)
    n64               the two graphs of the test set n64: K64 and one sparse 64-node graph

The device figures are whole Python calls -- workspace allocation, the memset of the tables, the compaction to CSR with its one host
round trip -- timed between two HIP events after a warm-up: `--repeats` windows of about `--window` seconds each (sized from one call's
time), the median and the spread of the per-call means.  nspdk_mmd is timed on the first half of the rows against the rest.  The first
graphs of every workload are checked against the pure-Python restatement (tests/nspdk_ref.py) before timing.  One JSON line per
workload (appended to --out when given); without an MI355X the device figures read "not measured".  --emulate runs the device side on
the host emulation at 8 graphs (a rehearsal of the script: its times mean nothing).

What stood here before is the reference's vectoriser, pure Python over networkx graphs (evaluation/eden.py).  --reference times
vectorize(graphs, complexity=4, discrete=True) over the same graphs ONCE on the machine at hand (where the reference is installed) and
writes --host-file; a later run copies those figures into its lines under "host_reference", labelled as host numbers from another
machine.  They are context, not a ratio.

    python tools/bench_nspdk.py [--n 1024] [--out profiles/r17_nspdk_bench.jsonl] [--emulate]
    python tools/bench_nspdk.py --reference                    # host figures only -> profiles/r17_nspdk_host.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd import evaluation as ev  # noqa: E402
from tests import nspdk_cases as nc  # noqa: E402
from tests import nspdk_ref  # noqa: E402

HOST_FILE = os.path.join(ROOT, "profiles", "r17_nspdk_host.json")


def workloads(n):
    """(tag, adjacency (B, N, N) int8 with bond orders, labels (B, N) int32)."""
    out = []
    for N, extra, labels in ((9, 2, [6, 7, 8, 9]), (38, 4, [6, 7, 8, 9, 16, 17])):
        rng = np.random.default_rng(1000 + N)
        adj = np.stack([nc._adj(N, nc._sparse(rng, N, extra)) for _ in range(n)])
        out.append((f"mol_n{N}", adj, rng.choice(labels, (n, N)).astype(np.int32)))
    adj, lab = nc.graph_sets()["n64"]
    out.append(("n64", adj, lab))
    return out


def reference_seconds(adj, lab):
    """The reference's vectoriser over the same graphs as networkx graphs with integer labels."""
    import networkx as nx

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import refshim

    refshim.install()
    sys.modules.setdefault("pyemd", type(sys)("pyemd"))
    from ccsd.src.evaluation import eden

    graphs = []
    for a, l in zip(adj, lab):
        g = nx.Graph()
        for i in np.nonzero(l >= 0)[0]:
            g.add_node(int(i), label=int(l[i]))
        for i, j in zip(*np.nonzero(np.triu(a, 1))):
            g.add_edge(int(i), int(j), label=int(a[i, j]))
        graphs.append(g)
    t0 = time.perf_counter()
    X = eden.vectorize(graphs, complexity=4, discrete=True)
    return time.perf_counter() - t0, int(X.nnz)


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
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--host-file", default=HOST_FILE)
    a = ap.parse_args()
    if a.reference:
        host = {"what": "the reference's vectorize(graphs, complexity=4, discrete=True), pure Python on one core, timed once", "graphs": a.n,
                "cpu": next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown")}
        for tag, adj, lab in workloads(a.n):
            sec, nnz = reference_seconds(adj, lab)
            host[tag] = {"graphs": len(adj), "seconds": round(sec, 3), "nnz": nnz}
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
    for tag, adj, lab in workloads(a.n):
        B, N = adj.shape[:2]
        rec = {"workload": "nspdk", "set": tag, "graphs": B, "N": N, "device": name, "features_ms": "not measured", "mmd_ms": "not measured"}
        if run:
            t, l = torch.from_numpy(adj.astype(np.float32)).to(dev), torch.from_numpy(lab).to(dev)
            f = eng.nspdk_features(t, l, mol=True)
            ip, ix, vl = (f[k].cpu().numpy() for k in nc.KEYS)
            k = min(B, 4) if N < 64 else 0                                  # (K64 in pure Python takes a while: the sparse graph alone)
            sel = slice(0, k) if k else slice(1, 2)
            wp, wx, wv = nspdk_ref.rows(adj[sel].astype(np.int64), lab[sel])
            lo, hi = int(ip[sel.start]), int(ip[sel.stop])
            assert np.array_equal(ix[lo:hi], wx) and np.abs(vl[lo:hi] / wv - 1).max() <= 1e-12, tag
            half = B // 2
            s1, s2 = nc.rows_slice(f, slice(0, half)), nc.rows_slice(f, slice(half, B))
            mmd = float(eng.nspdk_mmd(s1, s2)[3])
            (med, lo_, hi_), iters = device_ms(lambda: eng.nspdk_features(t, l, mol=True), a.window, a.repeats, gpu)
            (mm, ml, mh), miters = device_ms(lambda: eng.nspdk_mmd(s1, s2), a.window, a.repeats, gpu)
            rec.update(features_ms=round(med, 4), features_ms_min=round(lo_, 4), features_ms_max=round(hi_, 4), features_calls_per_window=iters,
                       mmd_ms=round(mm, 4), mmd_ms_min=round(ml, 4), mmd_ms_max=round(mh, 4), mmd_calls_per_window=miters, windows=a.repeats,
                       graphs_per_s=round(B / (med * 1e-3), 1), nnz=int(ip[-1]), max_row_nnz=int(np.diff(ip).max()), mmd=mmd)
        if tag in host and host[tag]["graphs"] == B:
            rec["host_reference"] = {"label": "host numbers from another machine: the reference's pure-Python vectoriser on one core, timed once",
                                     "cpu": host.get("cpu"), "seconds": host[tag]["seconds"]}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
