"""Time of the two spectral descriptors on the device (PCEngine.spectral_hist, PCEngine.hodge_spectrum) against LAPACK on the host:

    spectral_hist    1024 graphs at N = 20 and at N = 125   (k_norm_laplacian + k_eigvalsh with the histogram in its epilogue)
    hodge_spectrum   1024 complexes at E = 36 (N = 9, cells of 3..5 nodes) and at E = 190 (N = 20, cells of 3..4 nodes)
                     (k_hodge_laplacian + k_eigvalsh)

The host side solves the SAME matrices, built beforehand in numpy and not timed: scipy.linalg.eigvalsh in float64, one matrix per call
on a pool of `--threads` threads (what spectral_worker does per graph), and torch.linalg.eigvalsh in float32, one matrix per call on the
same pool with the reference's fall-backs (what hodge_laplacian_spectrum_worker does per complex).  The device figure is the whole call -- building the
matrices included -- as the mean of `--iters` calls between two HIP events after a warm-up; the eigenvalues of the two sides are
compared before timing (the float32 device spectra against the float64 host ones).  One JSON line per workload (appended to --out when given); without an MI355X the device figures read
"not measured".  --emulate runs the device side on the host emulation at 8 samples (a rehearsal of the script: its times mean nothing).

    python tools/bench_spectrum.py [--n 1024] [--iters 5] [--threads 16] [--out profiles/r15_spectrum_bench.jsonl] [--emulate]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from itertools import combinations

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ccsd_amd import evaluation as ev  # noqa: E402


def graphs(n, N, p, seed):
    rng = np.random.default_rng(seed)
    u = np.triu(rng.random((n, N, N)) < p, 1)
    return (u | u.transpose(0, 2, 1)).astype(np.float32)


def laplacians(adj):
    out = []
    for a in adj:
        keep = a.sum(1) > 0
        w = a[keep][:, keep].astype(np.float64)
        d = w.sum(1)
        out.append(np.eye(len(d)) - w / np.sqrt(d[:, None] * d[None, :]) if keep.any() else np.zeros((1, 1)))
    return out


def complexes(n, N, d_min, d_max, seed):
    """(adj (n, N, N) float32, cell_bits (n, W) int64, H (n, E, E) float64): 2..8 random cells per complex."""
    rng = np.random.default_rng(seed)
    adj = graphs(n, N, 0.5, seed + 1)
    cells = [c for d in range(d_min, d_max + 1) for c in combinations(range(N), d)]
    eidx = {e: i for i, e in enumerate(combinations(range(N), 2))}
    K, E = len(cells), len(eidx)
    bits = np.zeros((n, (K + 63) // 64), np.uint64)
    H = np.zeros((n, E, E))
    for b in range(n):
        for k in rng.choice(K, size=int(rng.integers(2, 9)), replace=False):
            bits[b, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
            el = [eidx[e] for e in combinations(cells[k], 2) if adj[b, e[0], e[1]] != 0]
            H[b][np.ix_(el, el)] += 1
    return adj, bits.view(np.int64), H


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulate", action="store_true")
    a = ap.parse_args()
    from scipy.linalg import eigvalsh as sp_eigvalsh

    lib, dev, gpu = None, "cuda:0", torch.cuda.is_available()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, gpu, a.n, a.iters = emu_library(), "cpu", False, 8, 1
    run = gpu or a.emulate
    torch.set_num_threads(1)              # (the pool's threads are the parallelism: one matrix per call)
    pool = ThreadPoolExecutor(a.threads)
    name = torch.cuda.get_device_name(0) if gpu else ("host emulation" if a.emulate else None)
    eng = ev._ops(dev, lib) if run else None
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    for N, p in ((20, 0.3), (125, 0.08)):
        adj = graphs(a.n, N, p, N)
        L = laplacians(adj)
        t0 = time.perf_counter()
        host = list(pool.map(sp_eigvalsh, L))
        host_ms = (time.perf_counter() - t0) * 1e3
        rec = {"workload": "spectral_hist", "graphs": a.n, "N": N, "device": name, "host_threads": a.threads,
               "scipy_eigvalsh_f64_ms": round(host_ms, 2), "device_ms": "not measured"}
        if run:
            t = torch.from_numpy(adj).to(dev)
            got = eng.spectral_hist(t, eig=True)
            e, ne = got["spectral_eig"].cpu().numpy(), got["spectral_n"].cpu().numpy()
            rec["max_eigenvalue_difference"] = max(float(np.abs(e[b, :ne[b]] - np.clip(host[b], 0, None)).max()) for b in range(a.n))
            rec["device_ms"] = round(device_ms(lambda: eng.spectral_hist(t), a.iters, gpu), 4)
            rec["graphs_per_s"] = round(a.n / (rec["device_ms"] * 1e-3), 1)
            rec["ratio_scipy_over_device"] = round(host_ms / rec["device_ms"], 2)
        emit(rec)

    for N, d_min, d_max in ((9, 3, 5), (20, 3, 4)):
        adj, bits, H = complexes(a.n, N, d_min, d_max, N)
        H32 = torch.from_numpy(H.astype(np.float32))
        failed = []

        def worker(h):               # hodge_laplacian_spectrum_worker's call and its fall-backs (cc_utils.py:1013-1019)
            for uplo in ("L", "U"):
                try:
                    return torch.linalg.eigvalsh(h, uplo).numpy()
                except Exception:
                    pass
            failed.append(1)
            return np.zeros(h.shape[0], np.float32)

        worker(H32[0])
        t0 = time.perf_counter()
        host = np.stack(list(pool.map(worker, list(H32))))
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host64 = np.stack(list(pool.map(sp_eigvalsh, list(H))))
        host64_ms = (time.perf_counter() - t0) * 1e3
        rec = {"workload": "hodge_spectrum", "complexes": a.n, "N": N, "E": N * (N - 1) // 2, "d_min": d_min, "d_max": d_max, "device": name,
               "host_threads": a.threads, "torch_eigvalsh_f32_ms": round(host_ms, 2), "scipy_eigvalsh_f64_ms": round(host64_ms, 2),
               # (LAPACK's float32 divide-and-conquer does fail on some of these matrices; the reference then returns zeros)
               "torch_f32_failed": len(failed), "torch_f32_nan_eigenvalues": int(np.isnan(host).sum()),
               "device_ms": "not measured"}
        if run:
            ta, tb = torch.from_numpy(adj).to(dev), torch.from_numpy(bits).to(dev)
            got, sw = eng.hodge_spectrum(ta, tb, d_min=d_min, d_max=d_max, sweeps=True)
            rec["max_eigenvalue_difference"] = float(np.abs(got.cpu().numpy() - host64).max())          # (against float64: one float32 rounding)
            rec["sweeps_max"] = int(sw.max())
            rec["device_ms"] = round(device_ms(lambda: eng.hodge_spectrum(ta, tb, d_min=d_min, d_max=d_max), a.iters, gpu), 4)
            rec["complexes_per_s"] = round(a.n / (rec["device_ms"] * 1e-3), 1)
            rec["ratio_torch_over_device"] = round(host_ms / rec["device_ms"], 2)
        emit(rec)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
