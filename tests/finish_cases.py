"""Shared cases for ccsd_finish / SampleOps.finish (k_finish_rank2, k_finish_graph): run by tests/test_finish.py over the host emulation
and by tests/test_gpu_finish.py on the device.  Every comparison is between integers and exact.

Geometries: the smallest that reach each hazard of the rank-2 pass -- K < 64 with B E K not a multiple of 4 (n5), K % 64 != 0 and K % 4 = 2
with seven size bins and two column slabs (n9, the qm9_CC geometry), many slabs (n18, the ego_small_CC geometry: K = 12444), E = 703 rows
(n38, the zinc250k_CC substitute) -- and graph-only calls at N = 2, 64, 65 (one lane past a wave) and 361 (the grid checkpoint)."""
import json
from itertools import combinations
from math import comb

import numpy as np
import pytest
import torch

from ccsd_amd.samples import cells_from_bits
from tests.helpers import load_golden, sample_ops

# name -> (B, N, F, d_min, d_max); d_min = 0: graph-only
GEOMETRIES = {
    "n5": (3, 5, 3, 3, 4),
    "n9": (5, 9, 4, 3, 9),
    "n18": (2, 18, 17, 3, 5),
    "n38": (1, 38, 9, 3, 3),
    "g2": (2, 2, 1, 0, 0),
    "g64": (2, 64, 3, 0, 0),
    "g65": (2, 65, 2, 0, 0),
    "g361": (2, 361, 5, 0, 0),
}
CC = [g for g, v in GEOMETRIES.items() if v[3]]
NEW_GRAPH = ("degree", "degree_hist", "edge_hist", "n_nodes", "x_hist")
NEW_RANK2 = ("rank2_cell_hist", "rank2_nnz")


def special_values():
    """-0.0 and the quantisation thresholds 0.5, 1.5, 2.5, each with its two fp32 neighbours."""
    out = [np.float32(-0.0), np.float32(0.0)]
    for t in (0.5, 1.5, 2.5):
        t = np.float32(t)
        out += [np.nextafter(t, np.float32(-10)), t, np.nextafter(t, np.float32(10))]
    return np.array(out, np.float32)


_inputs = {}


def inputs(name):
    """Random x / adj / rank2 (CPU tensors, made once per geometry) with ragged node flags; the special values are sprinkled over
    adj and rank2, and written once more at the very first and last entries (the packed-store head and tail)."""
    if name in _inputs:
        return _inputs[name]
    B, N, F, d_min, d_max = GEOMETRIES[name]
    rng = np.random.default_rng(1000 + len(name) + N)
    counts = [max(1, N - (3 * b) % N) for b in range(B)]
    flags = np.zeros((B, N), np.float32)
    for b, c in enumerate(counts):
        flags[b, :c] = 1
    sp = special_values()
    x = (rng.standard_normal((B, N, F)).astype(np.float32) * 0.8 + 0.3) * flags[:, :, None]
    x[0, 0, :] = 0.0                                             # an unmasked node without features: not a node by cc_from_incidence's rule
    adj = rng.standard_normal((B, N, N)).astype(np.float32) * 1.3 + 0.6
    pos = rng.choice(adj.size, size=min(adj.size, 4 * len(sp)), replace=False)
    adj.reshape(-1)[pos] = np.resize(sp, len(pos))
    adj = adj * flags[:, :, None] * flags[:, None, :]
    rank2 = None
    if d_min:
        E, K = N * (N - 1) // 2, sum(comb(N, d) for d in range(d_min, d_max + 1))
        # sparse enough that some columns of every size stay empty: most entries below the threshold
        rank2 = rng.standard_normal((B, E, K)).astype(np.float32) * 0.25 + (rng.random((B, 1, K)) < 0.3).astype(np.float32) * 0.3
        pos = rng.choice(rank2.size, size=8 * len(sp), replace=False)
        rank2.reshape(-1)[pos] = np.resize(sp, len(pos))
        rank2.reshape(-1)[:len(sp)] = sp
        rank2.reshape(-1)[-len(sp):] = sp
        rank2[B - 1, :, K - 1] = 0.75                            # the last column of the last complex holds a cell
    t = {"x": torch.from_numpy(x), "adj": torch.from_numpy(adj), "rank2": None if rank2 is None else torch.from_numpy(rank2),
         "flags": torch.from_numpy(flags)}
    _inputs[name] = t
    return t


_runs = {}


def run(lib, dev, name, mol):
    """finish() of the geometry's inputs on `dev`, results as CPU tensors (made once per device, geometry and mode)."""
    key = (dev, name, mol)
    if key not in _runs:
        B, N, F, d_min, d_max = GEOMETRIES[name]
        t = inputs(name)
        eng = sample_ops(lib, dev)
        mv = lambda v: None if v is None else v.to(dev)
        res = eng.finish(mv(t["x"]), mv(t["adj"]), mv(t["rank2"]), mv(t["flags"]), mol=mol, d_min=d_min, d_max=d_max)
        _runs[key] = {k: v.cpu() for k, v in res.items()}
    return _runs[key]


def case_bitwise(lib, dev, name):
    """Test 1: adj_int, rank2_int, the cell bitmask and the cell counts against ccsd_quantize / ccsd_rank2_cells."""
    B, N, F, d_min, d_max = GEOMETRIES[name]
    t = inputs(name)
    eng = sample_ops(lib, dev)
    adj = t["adj"].to(dev)
    for mol in (False, True):
        got = run(lib, dev, name, mol)
        want = eng.quantize(adj, -1.0 if mol else 0.5).cpu()
        assert got["adj_int"].dtype == torch.int64 and torch.equal(got["adj_int"], want), (name, mol)
    assert name == "g2" or set(run(lib, dev, name, True)["adj_int"].unique().tolist()) == {0, 1, 2, 3}
    if d_min:
        got = run(lib, dev, name, False)
        r = t["rank2"].to(dev)
        want = eng.quantize(r, 0.5).to(torch.uint8).cpu()
        assert got["rank2_int"].dtype == torch.uint8 and got["rank2_int"].shape == r.shape
        assert torch.equal(got["rank2_int"], want), name
        bits, counts = eng.rank2_cells(r, 0.5)
        assert got["rank2_cell_bits"].dtype == torch.int64 and torch.equal(got["rank2_cell_bits"], bits.cpu()), name
        assert got["rank2_cell_count"].dtype == torch.int32 and torch.equal(got["rank2_cell_count"], counts.cpu()), name
    else:
        assert "rank2_int" not in run(lib, dev, name, False)


def numpy_descriptors(x, adj, rank2, d_min, d_max, mol, thr=0.5):
    """Plain numpy restatement of every descriptor (the definitions of include/ccsd_hip.h)."""
    x, adj = np.asarray(x), np.asarray(adj)
    B, N = adj.shape[:2]
    if mol:
        q = (adj >= 0.5).astype(np.int64) + (adj >= 1.5) + (adj >= 2.5)
    else:
        q = np.where(adj < thr, 0, 1).astype(np.int64)
    off = ~np.eye(N, dtype=bool)
    out = {"degree": ((q != 0) & off[None]).sum(-1).astype(np.int32)}
    out["degree_hist"] = np.stack([np.bincount(out["degree"][b], minlength=N) for b in range(B)]).astype(np.int32)
    iu = np.triu_indices(N, 1)
    out["edge_hist"] = np.stack([np.bincount(q[b][iu], minlength=4) for b in range(B)]).astype(np.int32)
    out["n_nodes"] = (x != 0).any(-1).sum(-1).astype(np.int32)
    out["x_hist"] = (x > 0.5).sum(1).astype(np.int32)
    if rank2 is not None:
        on = np.asarray(rank2) >= thr
        size = np.concatenate([np.full(comb(N, d), d) for d in range(d_min, d_max + 1)])
        active = on.any(1)
        out["rank2_cell_count"] = active.sum(-1).astype(np.int32)
        out["rank2_cell_hist"] = np.stack([np.bincount(size[active[b]] - d_min, minlength=d_max - d_min + 1) for b in range(B)]).astype(np.int32)
        out["rank2_nnz"] = on.sum((1, 2)).astype(np.int32)
    return out


def case_descriptors(lib, dev, name):
    """Test 2: every new output against the numpy restatement, in both adjacency modes."""
    B, N, F, d_min, d_max = GEOMETRIES[name]
    t = inputs(name)
    for mol in (False, True):
        got = run(lib, dev, name, mol)
        want = numpy_descriptors(t["x"], t["adj"], t["rank2"], d_min, d_max, mol)
        for k, w in want.items():
            assert got[k].dtype == torch.int32 and tuple(got[k].shape) == w.shape, (name, k, got[k].shape, w.shape)
            assert np.array_equal(got[k].numpy(), w), (name, mol, k)
        assert set(NEW_GRAPH) <= set(got) and (not d_min or set(NEW_RANK2) <= set(got))
    if d_min:       # the histograms are consistent with the bitmask's cells
        got = run(lib, dev, name, False)
        cells = cells_from_bits(got["rank2_cell_bits"][B - 1], N, d_min, d_max)
        assert len(cells) == int(got["rank2_cell_count"][B - 1]) and tuple(range(N - d_max, N)) in cells
        assert [sum(len(c) == d for c in cells) for d in range(d_min, d_max + 1)] == got["rank2_cell_hist"][B - 1].tolist()


# ---- the reference's functions on the reference's samples (tests/golden/f1_finish.npz, tools/make_golden.py::f1_finish)
def f1_cases():
    meta = json.loads(str(load_golden("f1_finish.npz")["meta"]))
    return [(name, case) for name, m in meta.items() for case in m["cases"]]


def case_reference_fixture(lib, dev, name, case):
    """Test 3: degree_hist[:, 1:] is the reference's nx.degree_histogram (which trims trailing zeros, and is [1] for the one-node
    stand-in of an empty graph); rank2_cell_hist, edge_hist, n_nodes (and x_hist, rank2_nnz) are exact."""
    f1 = load_golden("f1_finish.npz")
    m = json.loads(str(f1["meta"]))[name]
    g5 = load_golden(f"g5_{name}.npz")
    pre = f"{name}/{case}/"
    x = torch.from_numpy(g5[f"{case}/x"])
    if f"{case}/adj" in g5.files:
        adj = torch.from_numpy(g5[f"{case}/adj"])
    else:       # kept by f1 as quantize_mol(adj): every descriptor is a function of it
        adj = torch.from_numpy(f1[pre + "adj_qmol"].astype(np.float32))
    rank2 = None
    if m["is_cc"]:
        if f"{case}/rank2" in g5.files:
            rank2 = torch.from_numpy(g5[f"{case}/rank2"])
        else:   # kept by f1 as the bits of quantize(rank2)
            shape = tuple(f1[pre + "rank2_shape"].tolist())
            rank2 = torch.from_numpy(np.unpackbits(f1[pre + "rank2_bits"])[:int(np.prod(shape))].reshape(shape).astype(np.float32))
    eng = sample_ops(lib, dev)
    mv = lambda v: None if v is None else v.to(dev)
    got = {k: v.cpu().numpy() for k, v in eng.finish(mv(x), mv(adj), mv(rank2), None, mol=m["mol"], d_min=m["d_min"], d_max=m["d_max"],
                                                     dense_rank2=False, dense_adj=False).items()}
    B, N = adj.shape[:2]
    ref_hist, ref_len = f1[pre + "degree_hist"], f1[pre + "degree_len"]
    for b in range(B):
        ours = got["degree_hist"][b]
        if ours[1:].any():
            top = int(np.nonzero(ours)[0].max())
            assert ref_len[b] == top + 1 and ref_hist[b][0] == 0, (name, case, b)         # trimmed at the largest degree; no isolated nodes kept
            assert np.array_equal(ours[1:], ref_hist[b][1:]), (name, case, b)
        else:   # no edge at all: the reference's graph is its one-node stand-in
            assert ref_hist[b].tolist() == [1] + [0] * (N - 1) and ref_len[b] == 1, (name, case, b)
    for k in ("edge_hist", "n_nodes", "x_hist"):
        assert np.array_equal(got[k], f1[pre + k]), (name, case, k)
    if m["is_cc"]:
        assert np.array_equal(got["rank2_cell_hist"], f1[pre + "cell_hist"]), (name, case)
        assert np.array_equal(got["rank2_nnz"], f1[pre + "rank2_nnz"]), (name, case)
        assert np.array_equal(got["rank2_cell_count"], f1[pre + "cell_hist"].sum(-1)), (name, case)


def case_null_outputs(lib, dev, name="n9"):
    """Test 4: a graph-only call, dense_rank2=False and descriptors only give the same values for what remains."""
    B, N, F, d_min, d_max = GEOMETRIES[name]
    t = inputs(name)
    eng = sample_ops(lib, dev)
    x, adj, rank2, flags = (t[k].to(dev) for k in ("x", "adj", "rank2", "flags"))
    full = run(lib, dev, name, True)
    graph = eng.finish(x, adj, None, flags, mol=True)
    assert set(graph) == {"adj_int", *NEW_GRAPH}
    sparse = eng.finish(x, adj, rank2, flags, mol=True, d_min=d_min, d_max=d_max, dense_rank2=False)
    assert set(sparse) == set(full) - {"rank2_int"}
    desc = eng.finish(x, adj, rank2, None, mol=True, d_min=d_min, d_max=d_max, dense_rank2=False, dense_adj=False)
    assert set(desc) == set(full) - {"rank2_int", "adj_int"}
    plain = eng.finish(x, adj, rank2, flags, mol=True, d_min=d_min, d_max=d_max, descriptors=False)
    assert set(plain) == {"adj_int", "rank2_int", "rank2_cell_bits", "rank2_cell_count"}
    only_r = eng.finish(None, adj, rank2, None, mol=True, d_min=d_min, d_max=d_max, dense_adj=False, descriptors=False, dense_rank2=False)
    assert set(only_r) == {"rank2_cell_bits", "rank2_cell_count"}
    for res in (graph, sparse, desc, plain, only_r):
        for k, v in res.items():
            assert torch.equal(v.cpu(), full[k]), k


def case_bad_dims(lib, dev):
    """K that is not sum C(N, d), E that is not N (N - 1) / 2: ValueError with the library's message, nothing launched."""
    eng = sample_ops(lib, dev)
    t = inputs("n5")
    x, adj, rank2 = (t[k].to(dev) for k in ("x", "adj", "rank2"))
    with pytest.raises(ValueError, match=r"K = 15 is not sum C\(N, d\) for d = 3\.\.5 = 16"):
        eng.finish(x, adj, rank2, None, d_min=3, d_max=5)
    with pytest.raises(ValueError, match=r"K = 14 is not sum C\(N, d\)"):
        eng.finish(x, adj, rank2[:, :, :14].contiguous(), None, d_min=3, d_max=4)
    with pytest.raises(ValueError, match=r"E = 9 is not N \(N - 1\) / 2 = 10"):
        eng.finish(x, adj, rank2[:, :9].contiguous(), None, d_min=3, d_max=4)
    with pytest.raises(ValueError, match="bad cell sizes"):
        eng.finish(x, adj, rank2, None, d_min=0, d_max=4)


# ---- the operations on finished samples build no network plan
def sample_calls(eng, ev_kw=None):
    """Every SampleOps method on `eng` at N = 5, d = 3..4 (E = 10, K = 15), B = 3 with the second complex without a cell, and eigvalsh at
    n = 3 -> {name: tensor}.  With ev_kw, evaluation.describe(..., spectra=True) and evaluation.compute_mmd as well."""
    B, N, F, d_min, d_max = GEOMETRIES["n5"]
    dev = eng.device
    t = {k: v.clone().to(dev) for k, v in inputs("n5").items()}           # (the shared inputs stay as they are)
    x, flags, rank2 = t["x"], t["flags"], t["rank2"]
    adj = (t["adj"] + t["adj"].transpose(1, 2)) / 2                        # cluster_hist and the spectra take a symmetric adjacency
    rank2[1] = 0.0
    assert rank2.shape == (3, 10, 15)
    cell = dict(d_min=d_min, d_max=d_max)
    out = {"quantize": eng.quantize(adj, -1.0), "quantize_rank2": eng.quantize(rank2, 0.5)}
    out["cells_bits"], out["cells_count"] = eng.rank2_cells(rank2, 0.5)
    fin = eng.finish(x, adj, rank2, flags, mol=True, **cell)
    assert int(fin["rank2_cell_count"][1]) == 0 and int(fin["rank2_cell_count"][2]) > 0
    out.update({"finish/" + k: v for k, v in fin.items()})
    out.update(eng.cluster_hist(adj, mol=True))
    out["mmd"] = eng.mmd(fin["degree_hist"], fin["degree_hist"][:2].contiguous(), "emd", degree=True)
    a = torch.tensor([[[2.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 2.0]], [[1.0, 0.5, 0.25], [0.5, -3.0, 0.0], [0.25, 0.0, 0.0]]],
                     dtype=torch.float64, device=dev)
    out["eig"], out["eig_sweeps"] = eng.eigvalsh(a, sweeps=True)
    out.update(eng.spectral_hist(adj, mol=True, eig=True))
    out["hodge"], out["hodge_sweeps"] = eng.hodge_spectrum(adj, fin["rank2_cell_bits"], mol=True, sweeps=True, **cell)
    assert not out["hodge"][1].any() and out["hodge"][2].any()            # exact zeros for the complex without a cell
    if ev_kw is not None:
        from ccsd_amd import evaluation as ev

        desc = ev.describe(adj, x, rank2, mol=True, spectra=True, **cell, **ev_kw)
        out.update({"describe/" + k: v for k, v in desc.items()})
        out["compute_mmd"] = torch.tensor(ev.compute_mmd(fin["degree_hist"], fin["degree_hist"][:2], degree=True, **ev_kw), dtype=torch.float64)
    return {k: v.cpu() for k, v in out.items()}


def case_no_plan(lib, dev, monkeypatch):
    """SampleOps, evaluation.describe and evaluation.compute_mmd run with ccsd_plan_create out of reach, and give what the same calls
    give on a PCEngine that owns a plan (created before the entry point is taken away)."""
    from ccsd_amd import evaluation as ev
    from ccsd_amd.engine import PCEngine

    real = PCEngine(None, None, None, None, None, None, N=5, F=1, is_cc=False, device=dev, lib=lib)
    assert real.handle and real.query("loop_form") >= 0                   # (it owns a plan, and the plan answers)
    want = sample_calls(real)
    fin = {k[len("finish/"):]: v for k, v in want.items() if k.startswith("finish/")}
    for k in ("degree", "degree_hist", "edge_hist", "n_nodes", "x_hist", "rank2_cell_bits", "rank2_cell_count", "rank2_cell_hist", "rank2_nnz"):
        want["describe/" + k] = fin[k]
    for k in ("cluster_hist", "tri2", "spectral_hist"):
        want["describe/" + k] = want[k]
    want["describe/hodge_spectrum"] = want["hodge"]
    want["compute_mmd"] = want["mmd"][3]

    def no_plan(*a):
        raise AssertionError("ccsd_plan_create called by an operation on finished samples")

    monkeypatch.setattr(lib.c, "ccsd_plan_create", no_plan)
    monkeypatch.setattr(ev, "_sample_ops", {})
    got = sample_calls(sample_ops(lib, dev), ev_kw=dict(device=dev, lib=lib))
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and torch.equal(got[k], w), k


def case_sample_builds_no_plan_for_the_finish(lib, tmp_path):
    """Sampler.sample() through the harness of tests/test_harness.py creates the plans its sampling function needs and none for the
    finish: ONE ccsd_plan_create for sample_qm9_CC.  Before SampleOps the count, measured on the commit before it with this very
    counter, was 2 (the second one the plan of the dummy engine that finish() hung off)."""
    from tests.test_harness import QM9_CC_YAML, run_harness

    real, calls = lib.c.ccsd_plan_create, []

    def counting(*a):
        calls.append(1)
        return real(*a)

    lib.c.ccsd_plan_create = counting
    try:
        out, _ = run_harness(tmp_path, lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2)
    finally:
        lib.c.ccsd_plan_create = real
    assert "rank2_cell_hist" in out and len(calls) == 2 - 1, len(calls)
