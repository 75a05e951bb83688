"""Shared cases for the orbit score (ccsd_orbit_counts, SampleOps.orbit_counts, orbit_stats_all and the orbits=True paths of
ccsd_amd/evaluation.py and Sampler.evaluate): run by tests/test_orbit.py over the host emulation and by tests/test_gpu_orbit.py on the
device.

Expected values come from three places.  A brute-force enumeration of all 3- and 4-subsets (below: numpy and itertools, no formula of the
kernel's).  Landmarks written out by hand for the six connected graphs on four nodes.  tests/golden/e3_orbit.npz (tools/make_golden.py
orbit): what the REFERENCE's own orbit counter prints for adjs_to_graphs of every graph set of e1_eval.npz, and the reference's
orbit_stats_all / eval_graph_list on eval_ref against eval_pred.

Tolerances.  Counts are integers: exact.  The rows orbit_stats_all scores are one IEEE division of the same integers: bit-equal.  The score
against the reference's unrounded one: 1e-12, the bound tests/eval_cases.py derives for gaussian scores (the inputs are identical doubles)."""
import ctypes as C
import itertools
import json
import math
import time

import numpy as np
import pytest
import torch

from ccsd_amd import evaluation as ev
from tests.eval_cases import GRAPH_SETS, TOL, e1
from tests.helpers import load_golden, sample_ops

_e3 = {}


def e3():
    if not _e3:
        z = load_golden("e3_orbit.npz")
        _e3["z"], _e3["meta"] = z, json.loads(str(z["meta"]))
    return _e3["z"], _e3["meta"]


def graph_set(name):
    """(adjacency (B, N, N) int8, mol) of a fixture set: six4 lives in e3_orbit.npz, the others in e1_eval.npz."""
    z3, meta = e3()
    if name == "six4":
        return z3["graphs/six4/adj"], False
    return e1()[0][f"graphs/{name}/adj"], meta["graph_sets"][name]["mol"]


# ---- brute force --------------------------------------------------------------------------------------------------------------------
# (sorted degree sequence of a connected graph on 4 nodes) -> {degree of the node inside it: orbit}
_FOUR = {(1, 1, 2, 2): {1: 4, 2: 5}, (1, 1, 1, 3): {1: 6, 3: 7}, (2, 2, 2, 2): {2: 8}, (1, 2, 2, 3): {1: 9, 2: 10, 3: 11},
         (2, 2, 3, 3): {2: 12, 3: 13}, (3, 3, 3, 3): {3: 14}}
_THREE = {(1, 1, 2): {1: 1, 2: 2}, (2, 2, 2): {2: 3}}


def brute_orbits(A):
    """(N, 15) int64 for one 0/1 symmetric adjacency with a zero diagonal: every 3- and 4-subset that induces a connected subgraph
    is classified by its sorted degree sequence (which fixes the edge count and the graphlet), each of its nodes credited by its degree."""
    N = len(A)
    out = np.zeros((N, 15), np.int64)
    out[:, 0] = A.sum(1)
    for k, table in ((3, _THREE), (4, _FOUR)):
        for S in itertools.combinations(range(N), k):
            sub = A[np.ix_(S, S)]
            deg = sub.sum(1)
            seen, stack = {0}, [0]
            while stack:
                u = stack.pop()
                for w in np.nonzero(sub[u])[0]:
                    if w not in seen:
                        seen.add(int(w))
                        stack.append(int(w))
            if len(seen) != k:
                continue
            roles = table[tuple(sorted(int(x) for x in deg))]
            for v, dv in zip(S, deg):
                out[v, roles[int(dv)]] += 1
    return out


def edges_of(adj, mol=False, thr=0.5):
    """The 0/1 adjacency include/ccsd_hip.h defines: a non-zero quantised entry off the diagonal."""
    adj = np.asarray(adj, np.float32)
    on = (adj >= 0.5) if mol else ~(adj < thr)
    return (on & ~np.eye(adj.shape[-1], dtype=bool)).astype(np.int64)


def node_count(A):
    return max(int((A.sum(1) > 0).sum()), 1)


BRUTE_SHAPES = [(2, 1.0), (4, 1.0), (5, 0.5), (8, 0.3), (9, 0.6), (12, 0.5), (14, 0.9), (13, 0.15)]
_brute = {}


def brute_set(key):
    """(adjacency (3, N, N) float32, expected node_orbits (3, N, 15), expected orbit_nodes (3,)); "special": a graph with isolated
    nodes, a graph without any edge, and a diagonal of ones beside a single edge."""
    if key not in _brute:
        if key == "special":
            A = np.zeros((3, 6, 6), np.float32)
            for i, j in ((0, 2), (2, 5), (0, 5)):
                A[0, i, j] = A[0, j, i] = 1
            A[2][np.diag_indices(6)] = 1
            A[2, 1, 4] = A[2, 4, 1] = 1
        else:
            N, p = key
            rng = np.random.default_rng(1000 * N + int(100 * p))
            A = np.zeros((3, N, N), np.float32)
            for b in range(3):
                u = np.triu(rng.random((N, N)) < p, 1)
                A[b] = u + u.T
        E = edges_of(A)
        _brute[key] = (A, np.stack([brute_orbits(e) for e in E]), np.array([node_count(e) for e in E], np.int32))
    return _brute[key]


def check_result(res, want_nodes_rows, want_count, tag):
    assert res["node_orbits"].dtype == torch.int64 and res["orbit_counts"].dtype == torch.int64 and res["orbit_nodes"].dtype == torch.int32
    assert np.array_equal(res["node_orbits"].cpu().numpy(), want_nodes_rows), tag
    assert np.array_equal(res["orbit_counts"].cpu().numpy(), want_nodes_rows.sum(1)), tag
    assert np.array_equal(res["orbit_nodes"].cpu().numpy(), want_count), tag


def case_brute(lib, dev, key):
    A, rows, nodes = brute_set(key)
    res = sample_ops(lib, dev).orbit_counts(torch.from_numpy(A).to(dev), per_node=True)
    check_result(res, rows, nodes, key)
    if key == "special":
        assert nodes.tolist() == [3, 1, 2] and not rows[1].any() and rows[0, [1, 3, 4]].sum() == 0 and rows[0, 0].tolist() == [2, 0, 0, 1] + [0] * 11


# ---- landmarks ----------------------------------------------------------------------------------------------------------------------
# six4, per graph: {node: its one non-zero 4-node orbit} (tools/make_golden.py::e3_six4 states which node is which)
SIX4 = [{0: 14, 1: 14, 2: 14, 3: 14},          # K4
        {0: 8, 1: 8, 2: 8, 3: 8},              # C4
        {0: 7, 1: 6, 2: 6, 3: 6},              # claw, centre 0
        {0: 10, 1: 10, 2: 11, 3: 9},           # paw: triangle 0 1 2, tail 2 -- 3
        {0: 13, 1: 13, 2: 12, 3: 12},          # diamond: 0 and 1 of degree 3
        {0: 4, 1: 5, 2: 5, 3: 4}]              # P4: 0 - 1 - 2 - 3


def case_landmarks(lib, dev):
    adj, _ = graph_set("six4")
    t = torch.from_numpy(adj.astype(np.float32)).to(dev)
    eng = sample_ops(lib, dev)
    per = eng.orbit_counts(t, per_node=True)
    rows = per["node_orbits"].cpu().numpy()
    assert rows.shape == (6, 4, 15)
    for b, roles in enumerate(SIX4):
        four = np.zeros((4, 11), np.int64)
        for v, k in roles.items():
            four[v, k - 4] = 1
        assert np.array_equal(rows[b, :, 4:], four), (b, rows[b])
    sums = eng.orbit_counts(t)
    assert set(sums) == {"orbit_counts", "orbit_nodes"} and sums["orbit_nodes"].tolist() == [4] * 6
    want = np.zeros((6, 11), np.int64)
    for b, roles in enumerate(SIX4):
        for k in roles.values():
            want[b, k - 4] += 1
    got = sums["orbit_counts"].cpu().numpy()
    assert np.array_equal(got[:, 4:], want), got
    assert got[:, 0].tolist() == [12, 8, 6, 8, 10, 6] and got[:, 3].tolist() == [12, 0, 0, 3, 6, 0]      # 2 x edges, 3 x triangles


# ---- the reference's rows -----------------------------------------------------------------------------------------------------------
_runs = {}


def orbit_run(lib, dev, name):
    key = (dev, name)
    if key not in _runs:
        adj, mol = graph_set(name)
        res = sample_ops(lib, dev).orbit_counts(torch.from_numpy(adj.astype(np.float32)).to(dev), mol=mol, per_node=True)
        _runs[key] = {k: v.cpu().numpy() for k, v in res.items()}
    return _runs[key]


def case_reference_rows(lib, dev, name):
    z3, _ = e3()
    got = orbit_run(lib, dev, name)
    want = z3[f"graphs/{name}/orca"].astype(np.int64)
    assert got["node_orbits"].shape == want.shape and np.array_equal(got["node_orbits"], want), name
    assert np.array_equal(got["orbit_counts"], want.sum(1)), name
    assert np.array_equal(got["orbit_nodes"], z3[f"graphs/{name}/nodes"]), name


def case_k512(lib, dev):
    """64-bit sums: the complete graph on 512 nodes.  Prints the time of the call (with its synchronisation)."""
    adj = (1 - torch.eye(512, dtype=torch.float32))[None].to(dev)
    eng = sample_ops(lib, dev)
    t0 = time.perf_counter()
    res = eng.orbit_counts(adj, per_node=True)
    rows = res["node_orbits"].cpu().numpy()
    print(f"orbit_counts of K512 on {dev}: {time.perf_counter() - t0:.3f} s")
    want = np.zeros(15, np.int64)
    want[0], want[3], want[14] = 511, 130305, 22108415
    assert want[3] == math.comb(511, 2) and want[14] == math.comb(511, 3)
    assert np.array_equal(rows[0], np.broadcast_to(want, (512, 15)))
    assert res["orbit_counts"][0].tolist() == (512 * want).tolist() and int(res["orbit_counts"][0, 14]) == 11319508480
    assert res["orbit_nodes"].tolist() == [512]


def case_raw_and_null(lib, dev):
    """Raw (unquantised) samples give the counts of their quantised form; each output alone equals the same output of the full call;
    all three NULL is CCSD_OK."""
    adj = e1()[0]["graphs/r65/adj"].astype(np.float32)
    rng = np.random.default_rng(65)
    raw = np.where(adj != 0, 0.5 + rng.random(adj.shape), 0.5 * rng.random(adj.shape)).astype(np.float32)
    raw = np.nextafter(np.minimum(raw, raw.transpose(0, 2, 1)), np.float32(0))     # symmetric; no-edge entries stay below 0.5
    raw[adj != 0] = np.maximum(raw[adj != 0], np.float32(0.5))
    want = orbit_run(lib, dev, "r65")
    eng = sample_ops(lib, dev)
    t = torch.from_numpy(raw).to(dev)
    got = eng.orbit_counts(t, per_node=True)
    for k in ("node_orbits", "orbit_counts", "orbit_nodes"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    B, N = raw.shape[:2]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    for k, shape, dt in (("node_orbits", (B, N, 15), torch.int64), ("orbit_counts", (B, 15), torch.int64), ("orbit_nodes", (B,), torch.int32)):
        buf = torch.full(shape, -1, dtype=dt, device=dev)
        args = [buf if k == n else None for n in ("node_orbits", "orbit_counts", "orbit_nodes")]
        lib.check(lib.ccsd_orbit_counts(p(t), B, N, 0, 0.5, p(args[0]), p(args[1]), p(args[2]), eng._stream()))
        assert np.array_equal(buf.cpu().numpy(), want[k]), k
    assert lib.ccsd_orbit_counts(p(t), B, N, 0, 0.5, None, None, None, eng._stream()) == 0
    assert lib.ccsd_orbit_counts(None, B, N, 0, 0.5, None, None, None, eng._stream()) != 0


def case_bad_dims(lib, dev):
    eng = sample_ops(lib, dev)
    with pytest.raises(ValueError, match=r"ccsd_orbit_counts: N = 1 outside 2\.\.512"):
        eng.orbit_counts(torch.zeros(1, 1, 1, device=dev))
    with pytest.raises(ValueError, match=r"ccsd_orbit_counts: N = 513 outside 2\.\.512"):
        eng.orbit_counts(torch.zeros(1, 513, 513, device=dev))
    with pytest.raises(ValueError, match=r"orbit_counts: adj must be \(B, N, N\)"):
        eng.orbit_counts(torch.zeros(1, 4, 5, device=dev))
    with pytest.raises(ValueError, match="thr"):
        eng.orbit_counts(torch.zeros(1, 4, 4, device=dev), thr=-1.0)


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def case_scores(lib, dev):
    z3, meta = e3()
    kw = dict(device=dev, lib=lib)
    ref, pred = (torch.from_numpy(e1()[0][f"graphs/{n}/adj"]) for n in ("eval_ref", "eval_pred"))
    for adj, want in ((ref, z3["total_counts_ref"]), (pred, z3["total_counts_pred"])):
        rows = ev.orbit_rows(adj, kw).cpu().numpy()
        assert rows.dtype == np.float64 and np.array_equal(rows, want)
    got = ev.orbit_stats_all(ref, pred, **kw)
    print(f"orbit_stats_all: {got:.17g} reference {meta['orbit_stats_all']:.17g}")
    assert abs(got - meta["orbit_stats_all"]) <= TOL
    assert ev.eval_torch_batch(ref, pred, orbits=True, **kw) == meta["eval_graph_list"]
    assert list(meta["eval_graph_list"]) == ["degree", "cluster", "orbit"]
    dr, dp = ev.describe(ref, orbits=True, **kw), ev.describe(pred, orbits=True, **kw)
    assert dr["orbit_counts"].shape == (12, 15) and dr["orbit_nodes"].dtype == torch.int32
    assert ev.eval_torch_batch(dr, dp, orbits=True, **kw) == meta["eval_graph_list"]
    assert ev.orbit_stats_all(dr, dp, **kw) == got
    # a descriptor dict without the counts but with its adj has them computed; without either it is refused
    assert ev.orbit_stats_all({"adj": ref}, dp, **kw) == got
    with pytest.raises(KeyError, match="orbit_counts"):
        ev.orbit_stats_all({"degree_hist": dr["degree_hist"]}, dp, **kw)
    for side in (ref, pred, dr):
        assert abs(ev.orbit_stats_all(side, side, **kw)) <= TOL
    assert abs(ev.orbit_stats_all(ref, pred, ev.gaussian_tv, **kw) - ev.compute_mmd(z3["total_counts_ref"], z3["total_counts_pred"], ev.gaussian_tv,
                                                                                  is_hist=False, sigma=30.0, **kw)) == 0.0
    with pytest.raises(ValueError, match="is_hist"):
        ev.orbit_stats_all(ref, pred, ev.gaussian_emd, **kw)


def case_opt_in(lib, dev):
    kw = dict(device=dev, lib=lib)
    adj = torch.from_numpy(graph_set("six4")[0])
    for spectra in (False, True):
        with pytest.raises(NotImplementedError, match="orbit.*orbits=True"):
            ev.eval_torch_batch(adj, adj, ["degree", "orbit"], spectra=spectra, **kw)
    assert set(ev.eval_torch_batch(adj, adj, **kw)) == {"degree", "cluster"}
    assert list(ev.eval_torch_batch(adj, adj, orbits=True, **kw)) == ["degree", "cluster", "orbit"]
    assert list(ev.eval_torch_batch(adj, adj, orbits=True, spectra=True, **kw)) == ["degree", "cluster", "orbit", "spectral"]
    assert list(ev.eval_torch_batch(adj, adj, spectra=True, **kw)) == ["degree", "cluster"]              # (spectral alone is never a default)
    assert list(ev.eval_torch_batch(adj, adj, ["orbit"], orbits=True, **kw)) == ["orbit"]
    assert not [k for k in ev.describe(adj, **kw) if k.startswith("orbit")]
    assert {"orbit_counts", "orbit_nodes"} <= set(ev.describe(adj, orbits=True, **kw))
    with pytest.raises(NotImplementedError, match="nspdk"):
        ev.eval_torch_batch(adj, adj, ["nspdk"], orbits=True, **kw)


# ---- Sampler.evaluate ---------------------------------------------------------------------------------------------------------------
GRAPH_YAML = {
    "is_cc": False,
    "data": {"data": "community_small", "dir": "./data"},
    "ckpt": "gdss_community_small",
    "sampler": {"predictor": "Euler", "corrector": "Langevin", "snr": 0.05, "scale_eps": 0.7, "n_steps": 1},
    "sample": {"use_ema": False, "noise_removal": True, "probability_flow": False, "eps": 1.0e-4, "seed": 42},
}


def case_sampler_evaluate(lib, tmp_path):
    """Sampler.evaluate(out, held, orbits=True) on a finished gdss_community_small run of two steps: exactly the "orbit" key is added,
    finite and in [-1e-9, 2]; the saved .npz scores identically; the result dict is not written to."""
    import os

    from tests.test_harness import run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_community_small", GRAPH_YAML, max_steps=2, rounds=1)
    keys = set(out)
    held = torch.from_numpy(e1()[0]["graphs/eval_ref/adj"])
    base = c.sampler.evaluate(out, held)
    assert set(base) == {"degree", "cluster"}
    got = c.sampler.evaluate(out, held, orbits=True)
    assert set(got) == {"degree", "cluster", "orbit"} and {k: got[k] for k in base} == base, (got, base)
    assert math.isfinite(got["orbit"]) and -1e-9 <= got["orbit"] <= 2.0, got
    assert set(out) == keys and not [k for k in keys if k.startswith("orbit")]
    (fname,) = os.listdir(tmp_path / "samples")
    saved = str(tmp_path / "samples" / fname)
    with np.load(saved) as z:
        assert set(z.files) == keys
    assert c.sampler.evaluate(saved, held, orbits=True) == got
    same = c.sampler.evaluate(out, saved, orbits=True)
    assert set(same) == set(got) and all(abs(v) <= 1e-12 for v in same.values()), same
    held_dict = {"adj": held}
    assert c.sampler.evaluate(out, held_dict, orbits=True) == got
