"""Shared cases for the lifting of graphs to combinatorial complexes (ccsd_lift, SampleOps.lift, evaluation.lift_settings and the lift=
paths of describe, eval_CC_batch and Sampler.evaluate): run by tests/test_lift.py over the host emulation and by tests/test_gpu_lift.py on
the device.

Expected values come from two places.  tests/lift_ref.py: a plain Python restatement of both rules (recursive path enumeration with sets,
the cycle-basis walk with dicts, the incidence matrix by loops).  tests/golden/e5_lift.npz (tools/make_golden.py lift): what the REFERENCE's
own convert_graphs_to_CCs(..., "path_based", "basic"), CC_to_incidence_matrices, rank2_distrib_worker, hodge_laplacian_spectrum_worker and
eval_CC_list give for two sets of 24 graphs at N = 12 and at N = 20.

Tolerances.  Every output of the lift is an integer or a 0/1 float: exact.  Hodge spectra against the reference's float32 ones: 4 x the
recorded f32_vs_f64 of the set, the rule of tests/spectrum_cases.py.  Scores: max(4 x the recorded discrepancy of that score, 1e-12) with
the rounding of eval_CC_list, the rule of tests/eval_cases.py and tests/spectrum_cases.py."""
import ctypes as C
import itertools
import json
import math

import numpy as np
import pytest
import torch

from ccsd_amd import _lib
from ccsd_amd import evaluation as ev
from tests import lift_ref as lr
from tests.helpers import load_golden, sample_ops
from tests.spectrum_cases import TOL, score_tol

_e5 = {}


def e5():
    if not _e5:
        z = load_golden("e5_lift.npz")
        _e5["z"], _e5["meta"] = z, json.loads(str(z["meta"]))
    return _e5["z"], _e5["meta"]


def random_graphs(B, N, p, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((B, N, N), np.float32)
    for b in range(B):
        u = np.triu(rng.random((N, N)) < p, 1)
        A[b] = u + u.T
    return A


def check(got, want, tag):
    """Every key of the restatement, exact; the bits as the int64 words finish() writes."""
    assert set(got) == set(want), (tag, set(got) ^ set(want))
    for k, v in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == (np.int64 if k == "rank2_cell_bits" else np.float32 if k == "rank2" else np.int32), (tag, k, g.dtype)
        if k == "rank2_cell_bits":
            g = g.view(np.uint64)
        assert g.shape == v.shape and np.array_equal(g, v), (tag, k)


# ---- paths --------------------------------------------------------------------------------------------------------------------------
# (N, d_min, d_max, B): K = 1; N = 4; K = 56 under one word; K = 84 across a word boundary; K = 1140; K = 18424 with a partial last
# word; K = 41664 = 651 words exactly; d 3..4 at N = 12: the columns of size 4 stay empty
PATH_SHAPES = [(3, 3, 3, 3), (4, 3, 3, 3), (8, 3, 3, 3), (9, 3, 3, 3), (20, 3, 3, 3), (49, 3, 3, 3), (64, 3, 3, 3), (12, 3, 4, 3)]
PATH_DENSITIES = (0.15, 0.5, 1.0)
PATH_CASES = [s + (p,) for s in PATH_SHAPES for p in PATH_DENSITIES] + [(9, 3, 3, 65, 0.5)]
_path_want = {}


def source_sets(N):
    return {"all": None, "zero": [0], "two": [N - 1, 1], "empty": []}


def path_want(case):
    """(adjacency, {source set name: the restatement's outputs}), computed once per case and shared by the CPU and GPU suites."""
    if case not in _path_want:
        N, d_min, d_max, B, p = case
        A = random_graphs(B, N, p, 7000 + 100 * N + int(100 * p) + B)
        _path_want[case] = (A, {name: lr.lift(A, "path_based", d_min, d_max, sources=src) for name, src in source_sets(N).items()})
    return _path_want[case]


def case_paths(lib, dev, case):
    N, d_min, d_max, B, p = case
    A, want = path_want(case)
    eng, t = sample_ops(lib, dev), torch.from_numpy(A).to(dev)
    for name, src in source_sets(N).items():
        got = eng.lift(t, "path_based", d_min=d_min, d_max=d_max, sources=src)
        check(got, want[name], (case, name))
        assert not got["lift_dropped"].any()
    assert not want["empty"]["rank2_cell_count"].any()
    if p == 1.0:                                                    # the complete graph: every triple, three edges each
        assert (want["all"]["rank2_cell_count"] == math.comb(N, 3)).all() and (want["all"]["rank2_nnz"] == 3 * math.comb(N, 3)).all()
        assert (want["zero"]["rank2_cell_count"] == math.comb(N - 1, 2)).all()      # (a path starts at its source: the triples that hold node 0)
    if d_max > 3:
        assert not want["all"]["rank2_cell_hist"][:, 1:].any() and want["all"]["rank2_cell_hist"][:, 0].any()
    if N <= 12:                                                     # with all sources: at least 2 of the 3 pairs are edges
        E0 = lr.edge_matrix(A[0])
        assert lr.path_cells(E0) == {frozenset(c) for c in itertools.combinations(range(N), 3)
                                     if sum(E0[i, j] for i, j in itertools.combinations(c, 2)) >= 2}


def case_golden_paths(lib, dev, name):
    """Bits, size histogram and nnz of the reference's own lifting, exactly; hodge_spectrum of the lifted bits against the reference's
    float32 spectra."""
    z, meta = e5()
    info = meta["sets"][name]
    N = info["N"]
    eng = sample_ops(lib, dev)
    for side in ("ref", "pred"):
        adj = torch.from_numpy(z[f"{name}/{side}/adj"].astype(np.float32)).to(dev)
        got = eng.lift(adj, "path_based", d_min=info["d_min"], d_max=info["d_max"])
        assert np.array_equal(got["rank2_cell_bits"].cpu().numpy().view(np.uint64), z[f"{name}/{side}/bits"]), (name, side)
        assert np.array_equal(got["rank2_cell_hist"].cpu().numpy(), z[f"{name}/{side}/hist"]), (name, side)
        assert np.array_equal(got["rank2_nnz"].cpu().numpy(), z[f"{name}/{side}/nnz"]), (name, side)
        assert np.array_equal(got["rank2_cell_count"].cpu().numpy(), z[f"{name}/{side}/hist"].sum(1)), (name, side)
        spec = eng.hodge_spectrum(adj, got["rank2_cell_bits"], d_min=info["d_min"], d_max=info["d_max"]).cpu().numpy()
        ref32 = z[f"{name}/{side}/spectrum"]
        assert spec.shape == ref32.shape == (24, info["E"])
        worst = float(np.abs(spec.astype(np.float64) - ref32).max())
        print(f"{name}/{side}: hodge spectrum of the lifted bits, largest difference {worst:.3g}, allowed {4 * meta['f32_vs_f64'][name + '/eig']:.3g}")
        assert worst <= 4 * meta["f32_vs_f64"][f"{name}/eig"], (name, side)


def golden_side(lib, dev, name, side):
    """The descriptor dict of a golden graph set as a user holds it: describe() of the adjacency, with adj kept."""
    z, _ = e5()
    adj = torch.from_numpy(z[f"{name}/{side}/adj"].astype(np.float32)).to(dev)
    return dict(ev.describe(adj, device=dev, lib=lib), adj=adj)


def case_golden_scores(lib, dev, name):
    """eval_CC_batch(..., lift=) on the two graph sets against the reference's eval_CC_list on its own lifted complexes."""
    _, meta = e5()
    info = meta["sets"][name]
    wk, nb = info["worker_kwargs"], info["hodge_nb"]
    kw = dict(device=dev, lib=lib)
    lift = dict(ev.lift_settings({"lifting_procedure": "path_based", "lifting_procedure_kwargs": "basic", "max_node_num": info["N"]}, info["N"]),
                d_min=info["d_min"], d_max=info["d_max"])
    assert lift == {"procedure": "path_based", "path_length": 3, "sources": None, "d_min": 3, "d_max": 3}
    ref, pred = golden_side(lib, dev, name, "ref"), golden_side(lib, dev, name, "pred")
    keys = set(ref)
    got = ev.eval_CC_batch(ref, pred, wk, lift=lift, **kw)
    want = meta[f"eval_CC_list/{name}"]
    assert set(got) == set(want) == {"rank1_distrib", "rank2_distrib"} and set(ref) == keys
    for m in got:
        slack = score_tol(meta, f"eval_CC_list/{name}")
        print(f"{name}/{m}: {got[m]:.9g} reference {want[m]:.9g} tolerance {slack:.3g}")
        assert abs(got[m] - want[m]) <= slack + 1.000001e-6 and (got[m] == want[m] or abs(got[m] - want[m]) <= max(slack, 1.000001e-6)), (m, got, want)
    key = f"eval_CC_list/{name}/first{nb}"
    got = ev.eval_CC_batch(ref, pred, wk, ["hodge_laplacian_spectrum", "rank1_distrib", "rank2_distrib"], cc_nb_eval=nb, spectra=True, lift=lift, **kw)
    want = meta[key]
    assert set(got) == set(want)
    tol_emd = max(4 * meta["lp_vs_closed"][key], 4 * meta["f32_vs_f64"][key], TOL)
    for m in got:
        slack = tol_emd if m == "hodge_laplacian_spectrum" else score_tol(meta, key)
        print(f"{key}/{m}: {got[m]:.9g} reference {want[m]:.9g} tolerance {slack:.3g}")
        assert abs(got[m] - want[m]) <= slack + 1.000001e-6 and (got[m] == want[m] or abs(got[m] - want[m]) <= max(slack, 1.000001e-6)), (m, got, want)
    # without lift= the graph sets have no rank-2 descriptors
    with pytest.raises(KeyError, match="rank2_cell_hist"):
        ev.eval_CC_batch(ref, pred, wk, **kw)


# ---- cycles -------------------------------------------------------------------------------------------------------------------------
def special_graphs():
    """name -> (adjacency (N, N), d_min, d_max, expected (cell_count, dropped) or None)."""
    def graph(N, edges, diag=False):
        A = np.zeros((N, N), np.float32)
        for i, j in edges:
            A[i, j] = A[j, i] = 1
        if diag:
            A[np.diag_indices(N)] = 1
        return A

    k4 = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    return {
        "tree": (graph(7, [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (5, 6)]), 3, 5, (0, 0)),
        "triangle": (graph(5, [(1, 2), (2, 4), (1, 4)]), 3, 5, (1, 0)),
        "k4": (graph(4, k4), 3, 4, None),
        "two_components": (graph(9, [(0, 1), (1, 2), (0, 2), (4, 5), (5, 6), (6, 7), (4, 7), (5, 7)]), 3, 5, None),
        "isolated_last": (graph(6, [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)]), 3, 5, None),
        "no_edges": (graph(5, []), 3, 5, (0, 0)),
        "c6_dropped": (graph(6, [(i, (i + 1) % 6) for i in range(6)]), 3, 5, (0, 1)),
        "diagonal": (graph(6, [(0, 3), (3, 5), (0, 5)], diag=True), 3, 5, (1, 0)),
    }


# (N, d_min, d_max, density): B = 3 each
CYCLE_RANDOM = [(5, 3, 5, 0.6), (12, 3, 4, 0.3), (18, 3, 5, 0.2), (40, 3, 5, 0.08), (64, 3, 5, 0.05), (64, 3, 5, 0.3)]
_cycle_want = {}


def cycle_want(key):
    if key not in _cycle_want:
        if isinstance(key, str):
            A, d_min, d_max, _ = special_graphs()[key]
            A = A[None]
        else:
            N, d_min, d_max, p = key
            A = random_graphs(3, N, p, 9000 + 10 * N + int(100 * p))
        _cycle_want[key] = (A, d_min, d_max, lr.lift(A, "cycles", d_min, d_max))
    return _cycle_want[key]


def case_cycles(lib, dev, key):
    A, d_min, d_max, want = cycle_want(key)
    got = sample_ops(lib, dev).lift(torch.from_numpy(A).to(dev), "cycles", d_min=d_min, d_max=d_max)
    check(got, want, key)
    for b in range(len(A)):                                        # the size of a cycle basis, whatever the basis
        assert int(want["rank2_cell_count"][b]) + int(want["lift_dropped"][b]) == lr.cyclomatic(lr.edge_matrix(A[b])), (key, b)
    if isinstance(key, str) and special_graphs()[key][3] is not None:
        assert (int(want["rank2_cell_count"][0]), int(want["lift_dropped"][0])) == special_graphs()[key][3], key
    if key == "k4":
        assert int(want["rank2_cell_count"][0]) == 3
    if key == "triangle":
        assert int(want["rank2_nnz"][0]) == 3


# ---- dense output -------------------------------------------------------------------------------------------------------------------
DENSE_CASES = [("path_based", 4, 3, 3, 3), ("path_based", 9, 3, 3, 3), ("path_based", 12, 3, 4, 3), ("path_based", 20, 3, 3, 2),
               ("cycles", 9, 3, 5, 3), ("cycles", 12, 3, 4, 3)]


def case_dense(lib, dev, case):
    """rank2 against the restatement; finish() of the dense output gives back the lift's own sparse outputs."""
    proc, N, d_min, d_max, B = case
    A = random_graphs(B, N, 0.4, 500 + N)
    want = lr.lift(A, proc, d_min, d_max, dense=True)
    eng, t = sample_ops(lib, dev), torch.from_numpy(A).to(dev)
    got = eng.lift(t, proc, d_min=d_min, d_max=d_max, dense=True)
    check(got, want, case)
    assert want["rank2"].any()
    back = eng.finish(None, t, got["rank2"], d_min=d_min, d_max=d_max, dense_rank2=False, dense_adj=False)
    for k in ("rank2_cell_bits", "rank2_cell_count", "rank2_cell_hist", "rank2_nnz"):
        assert torch.equal(back[k], got[k]), (case, k)


def case_overwrite(lib, dev):
    """Output buffers filled with 0xFF come back exact, the tail bits of the last word zero; two calls give identical bits."""
    eng = sample_ops(lib, dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    for proc, code, N, d_min, d_max in (("path_based", _lib.LIFT_PATHS, 9, 3, 3), ("path_based", _lib.LIFT_PATHS, 12, 3, 4), ("cycles", _lib.LIFT_CYCLES, 12, 3, 4)):
        A = random_graphs(3, N, 0.5, 77 + N)
        want = lr.lift(A, proc, d_min, d_max, dense=True)
        t = torch.from_numpy(A).to(dev)
        K, E = lr.n_columns(N, d_min, d_max), N * (N - 1) // 2
        W = (K + 63) // 64
        assert K % 64
        bufs = {"rank2_cell_bits": torch.full((3, W), -1, dtype=torch.int64, device=dev), "rank2_cell_count": torch.full((3,), -1, dtype=torch.int32, device=dev),
                "rank2_cell_hist": torch.full((3, d_max - d_min + 1), -1, dtype=torch.int32, device=dev), "rank2_nnz": torch.full((3,), -1, dtype=torch.int32, device=dev),
                "lift_dropped": torch.full((3,), -1, dtype=torch.int32, device=dev),
                "rank2": torch.full((3, E, K), float("nan"), dtype=torch.float32, device=dev)}
        for _ in range(2):
            lib.check(lib.ccsd_lift(p(t), 3, N, 0, 0.5, code, 3, (1 << 64) - 1, d_min, d_max, p(bufs["rank2_cell_bits"]), p(bufs["rank2_cell_count"]),
                                    p(bufs["rank2_cell_hist"]), p(bufs["rank2_nnz"]), p(bufs["lift_dropped"]), p(bufs["rank2"]), eng._stream()))
            check(bufs, want, (proc, N))
        tail = bufs["rank2_cell_bits"].cpu().numpy().view(np.uint64)[:, -1] >> np.uint64(K % 64)
        assert not tail.any()
        # the nullable outputs left out: the required ones are the same
        bits = torch.full((3, W), -1, dtype=torch.int64, device=dev)
        cnt = torch.full((3,), -1, dtype=torch.int32, device=dev)
        lib.check(lib.ccsd_lift(p(t), 3, N, 0, 0.5, code, 3, (1 << 64) - 1, d_min, d_max, p(bits), p(cnt), None, None, None, None, eng._stream()))
        assert torch.equal(bits, bufs["rank2_cell_bits"]) and torch.equal(cnt, bufs["rank2_cell_count"])
    assert lib.ccsd_lift(None, 0, 9, 0, 0.5, 0, 3, 0, 3, 3, None, None, None, None, None, None, eng._stream()) == 0          # B = 0: a no-op
    empty = eng.lift(torch.zeros((0, 9, 9), dtype=torch.float32, device=dev), "cycles", d_min=3, d_max=4)
    assert empty["rank2_cell_bits"].shape == (0, 4) and empty["lift_dropped"].shape == (0,)


def case_quantiser(lib, dev):
    """Raw samples lift like their quantised form; mol mode takes every bond order as a plain edge; only row i of pair (i, j), i < j,
    is read."""
    eng = sample_ops(lib, dev)
    A = random_graphs(3, 12, 0.4, 31)
    rng = np.random.default_rng(32)
    raw = np.where(A != 0, 0.5 + rng.random(A.shape), 0.49 * rng.random(A.shape)).astype(np.float32)
    raw = np.triu(raw, 1) + 7.0 * np.tril(np.ones_like(raw))      # (the lower triangle and the diagonal are never read)
    for proc in ("path_based", "cycles"):
        want = lr.lift(A, proc, 3, 4)
        check(eng.lift(torch.from_numpy(raw).to(dev), proc, d_min=3, d_max=4), want, proc)
        bonds = (A * rng.integers(1, 4, A.shape)).astype(np.float32)
        bonds = np.triu(bonds, 1) + np.triu(bonds, 1).transpose(0, 2, 1)
        check(eng.lift(torch.from_numpy(bonds).to(dev), proc, d_min=3, d_max=4, mol=True), want, (proc, "mol"))


def case_bad_args(lib, dev):
    eng = sample_ops(lib, dev)
    z = lambda N, B=1: torch.zeros((B, N, N), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match=r"ccsd_lift: N = 1 must be >= 2"):
        eng.lift(z(1), "path_based", d_min=1, d_max=1, path_length=1)
    for proc in ("path_based", "cycles"):
        with pytest.raises(NotImplementedError, match=r"ccsd_lift: N = 65 is above 64"):
            eng.lift(z(65), proc, d_min=3, d_max=3)
        with pytest.raises(ValueError, match="bad cell sizes d_min = 4, d_max = 3"):
            eng.lift(z(8), proc, d_min=4, d_max=3)
        with pytest.raises(ValueError, match="bad cell sizes d_min = 3, d_max = 9"):
            eng.lift(z(8), proc, d_min=3, d_max=9)
        with pytest.raises(ValueError, match=r"lift: adj must be \(B, N, N\)"):
            eng.lift(torch.zeros((1, 4, 5), device=dev), proc, d_min=3, d_max=3)
        with pytest.raises(ValueError, match="thr"):
            eng.lift(z(8), proc, d_min=3, d_max=3, thr=-1.0)
    with pytest.raises(NotImplementedError, match=r"path_length = 4"):
        eng.lift(z(8), "path_based", d_min=3, d_max=4, path_length=4)
    with pytest.raises(ValueError, match=r"path_length = 3 outside d_min\.\.d_max = 4\.\.5"):
        eng.lift(z(8), "path_based", d_min=4, d_max=5)
    with pytest.raises(ValueError, match="procedure"):
        eng.lift(z(8), "cliques", d_min=3, d_max=3)
    with pytest.raises(ValueError, match="exceeds 2\\^24"):
        eng.lift(z(64), "cycles", d_min=3, d_max=6)
    p = lambda t: C.c_void_p(t.data_ptr())
    bits, cnt = torch.zeros((1, 1), dtype=torch.int64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    assert lib.ccsd_lift(p(z(8)), 1, 8, 0, 0.5, 7, 3, 0, 3, 3, p(bits), p(cnt), None, None, None, None, None) == _lib.ERR_INVALID
    assert b"procedure" in lib.ccsd_last_error()
    assert lib.ccsd_lift(p(z(8)), 1, 8, 0, 0.5, 0, 3, 0, 3, 3, None, p(cnt), None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.ccsd_lift(p(z(8)), -1, 8, 0, 0.5, 0, 3, 0, 3, 3, p(bits), p(cnt), None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.ccsd_lift(p(z(8)), 1, 8, 0, 0.5, 0, 4, 0, 3, 4, p(bits), p(cnt), None, None, None, None, None) == _lib.ERR_UNSUPPORTED


def case_opt_in(lib, dev):
    kw = dict(device=dev, lib=lib)
    adj = torch.from_numpy(random_graphs(3, 9, 0.4, 5))
    base = ev.describe(adj, **kw)
    assert not [k for k in base if k.startswith("rank2_") or k.startswith("lift_")]
    lift = dict(procedure="cycles", d_min=3, d_max=5)
    got = ev.describe(adj, lift=lift, **kw)
    assert set(got) == set(base) | {"rank2_cell_bits", "rank2_cell_count", "rank2_cell_hist", "rank2_nnz", "lift_dropped"}
    want = lr.lift(adj.numpy(), "cycles", 3, 5)
    check({k: got[k] for k in want}, want, "describe")
    spec = ev.describe(adj, lift=lift, spectra=True, **kw)
    assert set(spec) == set(got) | {"spectral_hist", "hodge_spectrum"} and spec["hodge_spectrum"].shape == (3, 36)
    assert torch.equal(spec["hodge_spectrum"], sample_ops(lib, dev).hodge_spectrum(adj.to(dev), got["rank2_cell_bits"], d_min=3, d_max=5))
    with pytest.raises(ValueError, match="brings its own rank2"):
        ev.describe(adj, rank2=torch.zeros((3, 36, lr.n_columns(9, 3, 5))), d_min=3, d_max=5, lift=lift, **kw)
    # lift_settings: the reference's reading of the config, and its three refusals
    assert ev.lift_settings({"data": "x"}) is None
    assert ev.lift_settings({"lifting_procedure": "cycles"}) == {"procedure": "cycles"}
    assert ev.lift_settings({"lifting_procedure": "cycles", "lifting_procedure_kwargs": {}}, 12) == {"procedure": "cycles"}
    assert ev.lift_settings({"lifting_procedure": "path_based", "lifting_procedure_kwargs": "basic", "max_node_num": 20}, 20) == {
        "procedure": "path_based", "path_length": 3, "sources": None}
    assert ev.lift_settings({"lifting_procedure": "path_based", "lifting_procedure_kwargs": {"sources_nodes": [0, 3, 30], "path_length": 4}}, 20) == {
        "procedure": "path_based", "path_length": 4, "sources": [0, 3]}
    with pytest.raises(NotImplementedError, match="Lifting procedure kwargs fancy not implemented"):
        ev.lift_settings({"lifting_procedure": "path_based", "lifting_procedure_kwargs": "fancy"}, 20)
    with pytest.raises(NotImplementedError, match="Lifting procedure kwargs basic not implemented"):
        ev.lift_settings({"lifting_procedure": "cycles", "lifting_procedure_kwargs": "basic"}, 20)
    with pytest.raises(NotImplementedError, match="Lifting procedure cliques not implemented"):
        ev.lift_settings({"lifting_procedure": "cliques"}, 20)


# ---- Sampler.evaluate ---------------------------------------------------------------------------------------------------------------
_LIFT_DATA = {"max_node_num": 20, "d_min": 3, "d_max": 3, "lifting_procedure": "path_based", "lifting_procedure_kwargs": "basic"}
_SAMPLE = {"use_ema": False, "noise_removal": True, "probability_flow": False, "eps": 1.0e-4, "seed": 42}
_SAMPLER = {"predictor": "Euler", "corrector": "Langevin", "snr": 0.05, "scale_eps": 0.7, "n_steps": 1}
CC_YAML = {"is_cc": True, "data": dict(_LIFT_DATA, data="community_small_CC", dir="./data"), "ckpt": "ccsd_community_small_CC", "sampler": _SAMPLER,
           "sample": _SAMPLE}
GRAPH_YAML = {"is_cc": False, "data": dict(_LIFT_DATA, data="community_small", dir="./data"), "ckpt": "gdss_community_small", "sampler": _SAMPLER,
              "sample": _SAMPLE}


def held_out():
    return torch.from_numpy(e5()[0]["n20/ref/adj"][:6])


def case_sampler_evaluate_cc(lib, tmp_path):
    """On sample_community_small_CC, two steps: lift=True adds exactly rank2_distrib to the keys of lift=False and leaves the other values
    equal; with spectra=True also hodge_laplacian_spectrum; the result dict is not written to."""
    from tests.test_harness import run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_community_small_CC", CC_YAML, max_steps=2, rounds=1)
    keys = set(out)
    held = held_out()
    base = c.sampler.evaluate(out, held)
    assert set(base) == {"degree", "cluster", "rank1_distrib"}                              # (what it returns today)
    got = c.sampler.evaluate(out, held, lift=True)
    assert set(got) == set(base) | {"rank2_distrib"} and {k: got[k] for k in base} == base, (got, base)
    assert math.isfinite(got["rank2_distrib"]) and -1e-9 <= got["rank2_distrib"] <= 2.0, got
    assert c.sampler.evaluate(out, {"adj": held}, lift=True) == got
    # the eigenvalue solves are per complex: the first five samples of the run serve (a descriptor dict is a result like any other)
    few = {k: v[:5] for k, v in out.items() if k in ("adj", "degree_hist", "edge_hist", "n_nodes", "rank2_cell_hist", "rank2_cell_bits")}
    spec_base = c.sampler.evaluate(few, {"adj": held}, spectra=True)
    assert set(spec_base) == {"degree", "cluster", "spectral", "rank1_distrib"}
    spec = c.sampler.evaluate(few, {"adj": held}, spectra=True, lift=True)
    assert set(spec) == set(spec_base) | {"rank2_distrib", "hodge_laplacian_spectrum"} and {k: spec[k] for k in spec_base} == spec_base, (spec, spec_base)
    assert math.isfinite(spec["hodge_laplacian_spectrum"]) and -1e-9 <= spec["hodge_laplacian_spectrum"] <= 2.0, spec
    assert set(out) == keys and not [k for k in keys if k.startswith("lift_")]
    # the held-out side lifted by hand gives the same score
    lifted = dict(ev.describe(held, lift=dict(procedure="path_based", d_min=3, d_max=3), device=c.sampler.device0, lib=lib), adj=held)
    assert c.sampler.evaluate(out, lifted) == got


def case_sampler_evaluate_graph(lib, tmp_path):
    """On graph-only sample_community_small: lift=True adds rank1_distrib and rank2_distrib; a config without a lifting rule and a
    molecule config are refused."""
    from tests.test_harness import QM9_CC_YAML, run_harness, write_cfg
    from ccsd_amd import sampler as S
    from ccsd_amd.diffusion import CCSD

    out, c = run_harness(tmp_path, lib, None, "sample_community_small", GRAPH_YAML, max_steps=2, rounds=1)
    keys = set(out)
    held = held_out()
    base = c.sampler.evaluate(out, held)
    assert set(base) == {"degree", "cluster"}
    got = c.sampler.evaluate(out, held, lift=True)
    assert set(got) == {"degree", "cluster", "rank1_distrib", "rank2_distrib"} and {k: got[k] for k in base} == base, (got, base)
    assert all(math.isfinite(v) and -1e-9 <= v <= 2.0 for v in got.values()), got
    assert set(out) == keys
    same = c.sampler.evaluate(out, out, lift=True)
    assert all(abs(v) <= 1e-12 for v in same.values()), same
    for name, cfg, err in (("no_rule", dict(GRAPH_YAML, data={"data": "community_small", "dir": "./data", "d_min": 3, "d_max": 3}), ValueError),
                           ("mol", QM9_CC_YAML, NotImplementedError)):
        write_cfg(tmp_path, name, cfg)
        s = S.get_sampler_from_config(CCSD("sample", name + ".yaml", folder=str(tmp_path), seed=42).cfg)
        s.extra = dict(lib=lib, max_steps=1)
        with pytest.raises(err, match="lift"):
            s.evaluate(out, held, lift=True)
