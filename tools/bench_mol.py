"""Time of molecule post-processing on the device (SampleOps.mol_correct: k_mol_check_labels, k_mol_correct):

    1024 and 10 000 molecules at N = 9 (the QM9 table) and N = 38 (the ZINC250k table), the random molecule-like batches of
    tests/mol_cases.py (about 0.4 of them need no correction; the others carry free bond orders and extra bonds)

The device figure is the whole Python call (allocation of the outputs and the one flag read back included), timed between two HIP events
after a warm-up: `--repeats` windows of about `--window` seconds each (sized from one call's time), the median and the spread of the
per-call means.  The outputs of the first --check molecules are compared with the Python restatement (tests/mol_ref.py) before timing.
Beside it stands that restatement over the same molecules on --threads processes of the machine at hand, timed once: plain Python,
context and not a ratio.  The reference's own path (rdkit's SanitizeMol per added bond, utils/mol_utils.py) cannot be timed here: rdkit is
not installed.  One JSON line per workload (appended to --out when given); without an MI355X the device figures read "not measured".
--emulate runs the device side on the host emulation at 64 molecules (a rehearsal of the script: its times mean nothing).

    python tools/bench_mol.py [--out profiles/r21_mol_bench.jsonl] [--emulate]
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
from tests import mol_cases as mc  # noqa: E402
from tests import mol_ref  # noqa: E402
from tools.bench_orbit import device_ms  # noqa: E402


def _host_chunk(args):
    adj, labels, table = args
    r = mol_ref.mol_correct(adj, labels, table["max_valence"], table["charge_base"])
    return int(r["mol_n_corrections"].sum()), int(r["mol_no_correct"].sum())


def host_seconds(adj, labels, table, threads):
    """The restatement over all molecules on `threads` processes, timed once -> (seconds, decrements, molecules left alone)."""
    parts = min(threads * 4, len(adj))
    chunks = [(a, l, table) for a, l in zip(np.array_split(adj, parts), np.array_split(labels, parts)) if len(a)]
    t0 = time.perf_counter()
    with ProcessPoolExecutor(threads) as ex:
        got = list(ex.map(_host_chunk, chunks))
    return time.perf_counter() - t0, sum(g[0] for g in got), sum(g[1] for g in got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 10000])
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--emulate", action="store_true")
    a = ap.parse_args()
    lib, dev, gpu = None, "cuda:0", torch.cuda.is_available()
    if a.emulate:
        from tests.emu_util import emu_library

        lib, dev, gpu, a.sizes = emu_library(), "cpu", False, [64]
    run = gpu or a.emulate
    name = torch.cuda.get_device_name(0) if gpu else ("host emulation" if a.emulate else None)
    eng = ev._ops(dev, lib) if run else None
    lines = []
    for N, data in ((9, "QM9"), (38, "ZINC250k")):
        table = ev.MOL_TABLES[data]
        for B in a.sizes:
            adj, labels = mc.random_batch(B, N, table, seed=N)
            rec = {"workload": "mol_correct", "set": f"{data.lower()}_n{N}_b{B}", "molecules": B, "N": N, "labels": len(table["charge_base"]),
                   "device": name, "device_ms": "not measured"}
            if run:
                ta, tl = torch.from_numpy(adj).to(dev), torch.from_numpy(labels).to(dev)
                got = eng.mol_correct(ta, tl, dataset=data)
                nchk = min(a.check, B)
                want = mol_ref.mol_correct(adj[:nchk], labels[:nchk], table["max_valence"], table["charge_base"])
                for k, v in want.items():
                    assert np.array_equal(got[k][:nchk].cpu().numpy(), v), (rec["set"], k)
                (med, lo, hi), iters = device_ms(lambda: eng.mol_correct(ta, tl, dataset=data), a.window, a.repeats, gpu)
                rec.update(device_ms=round(med, 4), device_ms_min=round(lo, 4), device_ms_max=round(hi, 4), calls_per_window=iters,
                           windows=a.repeats, molecules_per_s=round(B / (med * 1e-3), 1))
            sec, dec, alone = host_seconds(adj, labels, table, a.threads)
            rec["host_restatement"] = {"label": "tests/mol_ref.py (plain Python) over the same molecules on the machine at hand, timed once",
                                       "processes": a.threads, "seconds": round(sec, 3)}
            rec.update(decrements=dec, no_correct=alone)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
