"""Time of a sample-and-score cycle's scoring half on the device (ccsd_amd/evaluation.py) against a float64 numpy restatement on the host:

    eval_torch_batch   degree + cluster of 1024 x 1024 graphs of N = 20 (describe() of both sets, then two ccsd_mmd calls)
    compute_mmd        gaussian_emd / gaussian_tv / gaussian at 1024 x 1024 histograms of L = 100 (one ccsd_mmd call each)

The baseline is NOT the reference's path (networkx graphs and one pyemd linear program per pair: 3 x 10^6 programs at this size) but
the same closed form in numpy float64 -- A @ A for the triangles, np.histogram, cumulative sums, |cdf_x - cdf_y| summed per pair -- on
`--threads` host threads (row blocks of the pair matrix; numpy releases the interpreter lock inside its loops).  Device figures are
the mean of `--iters` calls between two HIP events after a warm-up, host figures wall time of one call; the scores of the two sides are
compared before timing.  One JSON line per workload; without an MI355X the device figures read "not measured".  --emulate runs the
device side on the host emulation at 64 x 64 (a rehearsal of the script: its times mean nothing).

    python tools/bench_eval.py [--n 1024] [--iters 10] [--threads 16] [--emulate]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd import evaluation as ev  # noqa: E402


def np_disc(x, y, kind, sigma, scale, pool, block=32):
    """Mean kernel value over all pairs; x, y: float64 operands (cdfs for "emd", pmfs otherwise)."""
    def part(i0):
        d = x[i0:i0 + block, None, :] - y[None, :, :]
        if kind == "l2":
            dist = np.sqrt((d * d).sum(-1))
        else:
            dist = np.abs(d).sum(-1) * (1.0 / scale if kind == "emd" else 0.5)
        return np.exp(-dist * dist / (2 * sigma * sigma)).sum()
    return sum(pool.map(part, range(0, len(x), block))) / (len(x) * len(y))


def np_mmd(h1, h2, kind, sigma, scale, pool):
    """compute_mmd's closed form for rows that all have mass."""
    ops = []
    for h in (h1, h2):
        p = h / h.sum(1, keepdims=True)
        ops.append(np.cumsum(p, 1) if kind == "emd" else p)
    a, b = ops
    return np_disc(a, a, kind, sigma, scale, pool) + np_disc(b, b, kind, sigma, scale, pool) - 2 * np_disc(a, b, kind, sigma, scale, pool)


def np_describe(adj, bins=100):
    """degree histogram without bin 0 (an edgeless graph: [1]) and clustering histogram per graph, float64."""
    A = (adj >= 0.5) & ~np.eye(adj.shape[1], dtype=bool)[None]
    A = A.astype(np.int64)
    d = A.sum(-1)
    t2 = (A * (A @ A)).sum(-1)
    B, N = d.shape
    deg, clu = np.zeros((B, N)), np.zeros((B, bins))
    for b in range(B):
        keep = d[b] > 0
        if not keep.any():
            deg[b, 0], clu[b, 0] = 1, 1
            continue
        deg[b] = np.bincount(d[b][keep], minlength=N)
        c = np.where(d[b] > 1, t2[b] / np.maximum(d[b] * (d[b] - 1), 1), 0.0)[keep]
        clu[b] = np.histogram(c, bins=bins, range=(0.0, 1.0))[0]
    return deg, clu


def graphs(n, N, p, seed):
    rng = np.random.default_rng(seed)
    u = np.triu(rng.random((n, N, N)) < p, 1)
    return (u | u.transpose(0, 2, 1)).astype(np.float32)


def device_ms(fn, iters, gpu):
    fn()
    if not gpu:
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) / iters * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--emulate", action="store_true")
    a = ap.parse_args()
    lib, dev, gpu = None, "cuda:0", torch.cuda.is_available()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, gpu, a.n, a.iters = emu_library(), "cpu", False, 64, 1
    run = gpu or a.emulate
    kw = dict(device=dev, lib=lib)
    n, N, L = a.n, 20, 100
    pool = ThreadPoolExecutor(a.threads)
    name = torch.cuda.get_device_name(0) if gpu else ("host emulation" if a.emulate else None)

    # ---- eval_torch_batch: degree + cluster
    ref, pred = graphs(n, N, 0.30, 1), graphs(n, N, 0.36, 2)
    t0 = time.perf_counter()
    (dr, cr), (dp, cp) = np_describe(ref), np_describe(pred)
    host = {"degree": np_mmd(dr, dp, "emd", 1.0, 1.0, pool), "cluster": np_mmd(cr, cp, "emd", 0.1, 100.0, pool)}
    host_ms = (time.perf_counter() - t0) * 1e3
    rec = {"workload": "eval_torch_batch", "methods": ["degree", "cluster"], "graphs": [n, n], "N": N, "device": name, "host_threads": a.threads,
           "numpy_closed_form_ms": round(host_ms, 2), "device_ms": "not measured", "device_describe_ms": "not measured"}
    if run:
        tr, tp = torch.from_numpy(ref).to(dev), torch.from_numpy(pred).to(dev)
        got = ev.eval_torch_batch(tr, tp, **kw)
        rec["max_score_difference"] = max(abs(got[k] - host[k]) for k in host)          # (the device dict is rounded to 6 decimals)
        rec["device_ms"] = round(device_ms(lambda: ev.eval_torch_batch(tr, tp, **kw), a.iters, gpu), 4)
        rec["device_describe_ms"] = round(device_ms(lambda: (ev.describe(tr, **kw), ev.describe(tp, **kw)), a.iters, gpu), 4)
        rec["ratio_numpy_over_device"] = round(host_ms / rec["device_ms"], 2)
    print(json.dumps(rec), flush=True)

    # ---- compute_mmd at L = 100
    rng = np.random.default_rng(3)
    h1 = rng.integers(0, 9, (n, L)).astype(np.int32)
    h2 = (rng.integers(0, 9, (n, L)) * (np.arange(L) % 3 > 0)).astype(np.int32)
    h1[:, 0] += 1
    h2[:, 1] += 1
    for kind, sel, sigma, scale in (("emd", ev.gaussian_emd, 0.1, 100.0), ("tv", ev.gaussian_tv, 1.0, 1.0), ("l2", ev.gaussian, 1.0, 1.0)):
        t0 = time.perf_counter()
        host = np_mmd(h1.astype(np.float64), h2.astype(np.float64), kind, sigma, scale, pool)
        host_ms = (time.perf_counter() - t0) * 1e3
        rec = {"workload": "compute_mmd", "kernel": sel.__name__, "rows": [n, n], "L": L, "device": name, "host_threads": a.threads,
               "numpy_closed_form_ms": round(host_ms, 2), "device_ms": "not measured"}
        if run:
            t1, t2 = torch.from_numpy(h1).to(dev), torch.from_numpy(h2).to(dev)
            got = ev.mmd_terms(t1, t2, sel, sigma=sigma, distance_scaling=scale, **kw)[3].item()
            rec["score_difference"] = abs(got - host)
            rec["device_ms"] = round(device_ms(lambda: ev.mmd_terms(t1, t2, sel, sigma=sigma, distance_scaling=scale, **kw), a.iters, gpu), 4)
            rec["pair_bins_per_s"] = round(3.0 * n * n * L / (rec["device_ms"] * 1e-3), 1)
            rec["ratio_numpy_over_device"] = round(host_ms / rec["device_ms"], 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
