"""Shared cases for the NSPDK score (ccsd_nspdk_features, ccsd_nspdk_mmd, SampleOps.nspdk_features / nspdk_mmd, nspdk_stats and the
nspdk=True paths of ccsd_amd/evaluation.py and Sampler.evaluate): run by tests/test_nspdk.py over the host emulation and by
tests/test_gpu_nspdk.py on the device.

Expected values come from two places.  tests/golden/e4_nspdk.npz (tools/make_golden.py nspdk): the rows the REFERENCE's own
vectorize(graphs, complexity=4, discrete=True) gives for the graph sets below, built as networkx graphs that carry the same integers as
node and edge labels, and its compute_nspdk_mmd for a fixed split of each set.  tests/nspdk_ref.py: a pure-Python restatement.

The graph sets are generated here by seeded numpy (the fixture holds a copy, compared in test_nspdk.py) and are the smallest shapes at
which each part can go wrong:
  mol9    64 graphs, N = 9, labels from {6, 7, 8, 9}, bond orders 1..3; graph 0 a single atom, 1 without bonds, 2 two components,
          3 absent slots in the middle, 4 a bond to an absent slot
  mol38   16 sparse graphs, N = 38, degree <= 4, diameter > 8: all 25 blocks exist and the depth cap bites (the `2 rr < len` rule bites in mol9 and shapes)
  shapes  path of 20, cycle of 12, star of 9, K12, two triangles sharing a node -- in 20 slots, the unused ones absent
  n64     K64 (an edge layer of 1953, four blocks) and one sparse 64-node graph with several thousand non-zeros, where blocks share
          indices and the "block created last wins" rule decides

Tolerances, derived and not measured.  Index sets: identical.  Values: relative 1e-12 -- a sum of at most 40 960 non-negative doubles
moves by at most 40 960 x 2^-53 = 4.5e-12 relative with the order of its terms, and the square root halves that.  MMD: absolute 1e-12 for
these sets of at most 64 x 64 graphs -- 4 n1 n2 2^-53 on sums of terms in [0, 1] is 1.8e-12 at 64 x 64 and the largest split here is
32 x 32 (4.5e-13).  The fixture records how far the reference's own pairwise form is from the mean form of its own rows; it is printed."""
import json
import math

import numpy as np
import pytest
import torch

from ccsd_amd import evaluation as ev
from tests import nspdk_ref as R
from tests.helpers import load_golden, sample_ops

VAL_RTOL = 1e-12
MMD_ATOL = 1e-12
SET_NAMES = ("mol9", "mol38", "shapes", "n64")
KEYS = ("nspdk_indptr", "nspdk_indices", "nspdk_values")

_e4 = {}


def e4():
    if not _e4:
        z = load_golden("e4_nspdk.npz")
        _e4["z"], _e4["meta"] = z, json.loads(str(z["meta"]))
    return _e4["z"], _e4["meta"]


# ---- the graph sets -----------------------------------------------------------------------------------------------------------------
def _sparse(rng, n, extra, max_deg=4, back=3):
    """A connected graph on n nodes of degree <= max_deg: node i hangs on one of the `back` nodes before it, then `extra` chords
    between nodes at most 2 `back` apart (so the graph stays long).  {(i, j): bond order}."""
    deg, e = [0] * n, {}
    for i in range(1, n):
        cand = [j for j in range(max(0, i - back), i) if deg[j] < max_deg]
        j = int(rng.choice(cand))
        e[(j, i)] = int(rng.integers(1, 4))
        deg[i] += 1
        deg[j] += 1
    for _ in range(extra):
        i = int(rng.integers(0, n))
        j = int(rng.integers(max(0, i - 2 * back), min(n, i + 2 * back + 1)))
        i, j = min(i, j), max(i, j)
        if i != j and (i, j) not in e and deg[i] < max_deg and deg[j] < max_deg:
            e[(i, j)] = int(rng.integers(1, 4))
            deg[i] += 1
            deg[j] += 1
    return e


def _adj(n, edges):
    a = np.zeros((n, n), np.int8)
    for (i, j), l in edges.items():
        a[i, j] = a[j, i] = l
    return a


def diameter(adj, labels):
    nodes, edges = R.graph_of(adj.tolist(), labels.tolist())
    nb = {i: set() for i in nodes}
    for (i, j) in edges:
        nb[i].add(j)
        nb[j].add(i)
    best = 0
    for r in nodes:
        dist, front = {r: 0}, [r]
        while front:
            nxt = []
            for i in front:
                for j in nb[i]:
                    if j not in dist:
                        dist[j] = dist[i] + 1
                        nxt.append(j)
            front = nxt
        best = max(best, max(dist.values()))
    return best


_sets = {}


def graph_sets():
    """name -> (adj (B, N, N) int8 with the bond orders, labels (B, N) int32)."""
    if _sets:
        return _sets
    rng = np.random.default_rng(20261019)
    # mol9
    B, N = 64, 9
    adj, lab = np.zeros((B, N, N), np.int8), rng.choice([6, 7, 8, 9], (B, N)).astype(np.int32)
    for b in range(B):
        adj[b] = _adj(N, _sparse(rng, N, 2))
    adj[0] = 0
    lab[0] = -1
    lab[0, 4] = 8                                              # a single atom
    adj[1] = 0                                                 # nine atoms, no bond
    adj[2] = _adj(N, {(0, 1): 1, (1, 2): 2, (2, 0): 1, (3, 4): 3, (4, 5): 1, (5, 6): 1, (6, 7): 2, (7, 8): 1})      # two components
    lab[3, [3, 4]] = -1                                        # absent slots in the middle (their bonds are ignored)
    adj[4] = _adj(N, {(0, 1): 1, (1, 2): 2, (2, 3): 1, (3, 8): 3, (1, 8): 1})
    lab[4, 4:8] = -1
    adj[4, 2, 5] = adj[4, 5, 2] = 2                            # a bond to an absent slot
    _sets["mol9"] = (adj, lab)
    # mol38
    B, N = 16, 38
    adj, lab = np.zeros((B, N, N), np.int8), rng.choice([6, 7, 8, 9, 16, 17], (B, N)).astype(np.int32)
    for b in range(B):
        adj[b] = _adj(N, _sparse(rng, N, 4))
    _sets["mol38"] = (adj, lab)
    # shapes, in 20 slots
    N = 20
    shapes = [{(i, i + 1): 1 for i in range(19)}, {(i, (i + 1) % 12) if i < 11 else (0, 11): 1 for i in range(12)}, {(0, i): 1 for i in range(1, 9)},
              {(i, j): 1 for i in range(12) for j in range(i + 1, 12)}, {(0, 1): 1, (1, 2): 1, (0, 2): 1, (2, 3): 1, (3, 4): 1, (2, 4): 1}]
    sizes = [20, 12, 9, 12, 5]
    adj, lab = np.zeros((5, N, N), np.int8), np.full((5, N), -1, np.int32)
    for b, (es, n) in enumerate(zip(shapes, sizes)):
        adj[b] = _adj(N, es)
        lab[b, :n] = 6
    _sets["shapes"] = (adj, lab)
    # n64
    N = 64
    adj, lab = np.zeros((2, N, N), np.int8), np.zeros((2, N), np.int32)
    adj[0] = 1 - np.eye(N, dtype=np.int8)
    adj[1] = _adj(N, _sparse(rng, N, 30, max_deg=6))
    lab[1] = rng.choice([6, 7, 8], N)
    _sets["n64"] = (adj, lab)
    return _sets


def split(name):
    """The fixed split the fixture's compute_nspdk_mmd was recorded for: the first half of the set against the rest."""
    B = graph_sets()[name][0].shape[0]
    return slice(0, B // 2), slice(B // 2, B)


def case_fixture_matches_generator():
    z, meta = e4()
    assert set(meta["sets"]) == set(SET_NAMES)
    for name, (adj, lab) in graph_sets().items():
        assert np.array_equal(z[f"{name}/adj"], adj) and z[f"{name}/adj"].dtype == np.int8, name
        assert np.array_equal(z[f"{name}/labels"], lab), name
        ip = z[f"{name}/indptr"]
        assert ip.shape == (adj.shape[0] + 1,) and ip[-1] == len(z[f"{name}/indices"]) == len(z[f"{name}/values"]), name
    adj, lab = graph_sets()["mol38"]
    assert all(diameter(a, l) > 8 for a, l in zip(adj, lab)) and int(np.abs(adj).sum(-1).max()) <= 12 and int((adj != 0).sum(-1).max()) <= 4


def case_restatement_against_reference(name):
    """tests/nspdk_ref.py against the reference's rows: identical index sets, values within VAL_RTOL."""
    z, _ = e4()
    adj, lab = graph_sets()[name]
    sel = slice(1, 2) if name == "n64" else slice(None)          # (K64 in pure Python takes a while; the device cases cover it)
    ip, ix, vl = R.rows(adj[sel].astype(np.int64), lab[sel])
    lo, hi = (z[f"{name}/indptr"][1], z[f"{name}/indptr"][2]) if name == "n64" else (0, None)
    assert np.array_equal(ix, z[f"{name}/indices"][lo:hi]), name
    rel = np.abs(vl / z[f"{name}/values"][lo:hi] - 1).max()
    print(f"restatement vs reference, {name}: max relative value difference {rel:.3g}")
    assert rel <= VAL_RTOL


def case_structure_of_the_sets():
    """mol38: every graph creates all 25 blocks and every root's layers stop at the depth cap (9 layers) with nodes left beyond it;
    roots with fewer layers, where `2 rr < len` decides, are in mol9 and shapes (the star's centre against its leaves).
    n64: K64 has four blocks; the sparse graph's merged row holds fewer non-zeros than its blocks hold distinct features together
    (asserted on the reference's own row): the merge rule is exercised.  mol9: the single atom's row has two features at most."""
    z, _ = e4()
    adj, lab = graph_sets()["mol38"]
    for a, l in zip(adj, lab):
        _, order, _ = R.features(a.tolist(), l.tolist())
        assert len(order) == 25 and len(set(order)) == 25
        nodes, layers, ngh = R.neighbourhoods(a.tolist(), l.tolist())
        assert {len(h) for h in ngh.values()} == {9}              # every root is cut by the depth cap ...
        assert all(sum(len(x) for x in layers[r][::2]) < len(nodes) for r in nodes)      # ... with nodes left beyond distance 4
    # the `2 rr < len` rule bites in the small sets: roots whose layers end before the cap, pairs of roots of unequal length
    for name in ("mol9", "shapes"):
        short = mixed = 0
        for a, l in zip(*graph_sets()[name]):
            lens = {len(h) for h in R.neighbourhoods(a.tolist(), l.tolist())[2].values()}
            short += max(lens) < 9
            mixed += len(lens) > 1
            if max(lens) < 9:
                assert len(R.features(a.tolist(), l.tolist())[1]) < 25
        assert short >= 3 and mixed >= 2, (name, short, mixed)     # graphs that end before the cap; graphs whose roots differ in length
    adj, lab = graph_sets()["n64"]
    ip = z["n64/indptr"]
    _, order, blocks = R.features(adj[1].tolist(), lab[1].tolist())
    distinct = sum(len(b) for b in blocks.values())
    nnz = int(ip[2] - ip[1])
    print(f"n64 sparse graph: {nnz} non-zeros in the reference's row, {distinct} distinct features over {len(order)} blocks")
    assert nnz >= 2000 and nnz < distinct
    # K64: layers 0..3 (root, 63 edges, 63 nodes, 1953 edges): radii 0 and 1, distances 0 and 1
    assert 1 <= int(ip[1] - ip[0]) <= 8
    ip9 = z["mol9/indptr"]
    assert 1 <= int(ip9[1] - ip9[0]) <= 2


# ---- feature rows -------------------------------------------------------------------------------------------------------------------
_runs = {}


def feature_run(lib, dev, name):
    key = (dev, name)
    if key not in _runs:
        adj, lab = graph_sets()[name]
        _runs[key] = sample_ops(lib, dev).nspdk_features(torch.from_numpy(adj.astype(np.float32)).to(dev), torch.from_numpy(lab).to(dev), mol=True)
    return _runs[key]


def check_rows(got, ip, ix, vl, tag):
    assert got["nspdk_indptr"].dtype == torch.int64 and got["nspdk_indices"].dtype == torch.int32 and got["nspdk_values"].dtype == torch.float64
    g = [got[k].cpu().numpy() for k in KEYS]
    assert np.array_equal(g[0], ip), tag
    assert np.array_equal(g[1], ix), tag
    rel = float(np.abs(g[2] / vl - 1).max()) if len(vl) else 0.0
    print(f"{tag}: {len(ix)} non-zeros, max relative value difference {rel:.3g}")
    assert rel <= VAL_RTOL, (tag, rel)


def case_reference_rows(lib, dev, name):
    z, _ = e4()
    got = feature_run(lib, dev, name)
    check_rows(got, z[f"{name}/indptr"], z[f"{name}/indices"], z[f"{name}/values"], f"{name} on {dev}")
    ip, ix, vl = (got[k].cpu().numpy() for k in KEYS)
    for b in range(len(ip) - 1):
        row = ix[ip[b]:ip[b + 1]]
        assert (np.diff(row) > 0).all() and (len(row) == 0 or (row[0] >= 1 and row[-1] <= 65536)), (name, b)
        if len(row):
            assert abs(float((vl[ip[b]:ip[b + 1]] ** 2).sum()) - 1) <= 1e-12, (name, b)


def case_two_calls_same_bits(lib, dev):
    eng = sample_ops(lib, dev)
    for name in ("mol9", "n64"):
        adj, lab = graph_sets()[name]
        a, l = torch.from_numpy(adj.astype(np.float32)).to(dev), torch.from_numpy(lab).to(dev)
        one, two = eng.nspdk_features(a, l, mol=True), eng.nspdk_features(a, l, mol=True)
        for k in KEYS:
            assert torch.equal(one[k], two[k]), (name, k)
        assert torch.equal(one["nspdk_values"].view(torch.int64), feature_run(lib, dev, name)["nspdk_values"].view(torch.int64))
    f = feature_run(lib, dev, "mol9")
    g = feature_run(lib, dev, "mol38")
    m1, m2 = eng.nspdk_mmd(f, g), eng.nspdk_mmd(f, g)
    assert m1.dtype == torch.float64 and m1.shape == (4,) and torch.equal(m1.view(torch.int64), m2.view(torch.int64))


def random_graphs(count=200, seed=7):
    """`count` graphs of 1 to 12 slots, grouped by the slot count: {N: (adj (b, N, N) int8, labels (b, N) int32)}."""
    rng = np.random.default_rng(seed)
    groups = {}
    for _ in range(count):
        N = int(rng.integers(1, 13))
        p = float(rng.choice([0.15, 0.3, 0.6, 1.0]))
        u = np.triu((rng.random((N, N)) < p) * rng.integers(1, 4, (N, N)), 1).astype(np.int8)
        lab = rng.choice([6, 7, 8, 9, 70000, -1], N, p=[0.3, 0.25, 0.2, 0.1, 0.05, 0.1]).astype(np.int32)
        groups.setdefault(N, []).append((u + u.T, lab))
    return {N: (np.stack([g[0] for g in gs]), np.stack([g[1] for g in gs])) for N, gs in groups.items()}


def case_random_against_restatement(lib, dev):
    eng = sample_ops(lib, dev)
    n = 0
    for N, (adj, lab) in sorted(random_graphs().items()):
        got = eng.nspdk_features(torch.from_numpy(adj.astype(np.float32)).to(dev), torch.from_numpy(lab).to(dev), mol=True)
        check_rows(got, *R.rows(adj.astype(np.int64), lab), f"random N = {N} on {dev}")
        n += len(adj)
    assert n == 200


def case_labels_and_modes(lib, dev):
    """labels=None is label 0 in every slot; without `mol` every bond order is the edge label 1; raw samples give the rows of their
    quantised form; a graph without a node has an empty row."""
    eng = sample_ops(lib, dev)
    adj, _ = graph_sets()["mol9"]
    a = torch.from_numpy(adj[:8].astype(np.float32)).to(dev)
    zero = torch.zeros((8, 9), dtype=torch.int64, device=dev)
    none, lab0 = eng.nspdk_features(a, None, mol=True), eng.nspdk_features(a, zero, mol=True)
    for k in KEYS:
        assert torch.equal(none[k], lab0[k]), k
    check_rows(none, *R.rows(adj[:8].astype(np.int64), np.zeros((8, 9), np.int32)), f"labels=None on {dev}")
    plain = eng.nspdk_features(a, None, mol=False, thr=0.5)
    check_rows(plain, *R.rows((adj[:8] != 0).astype(np.int64), np.zeros((8, 9), np.int32)), f"mol=False on {dev}")
    raw = torch.from_numpy((adj[:8].astype(np.float32) + np.float32(0.3)) * (adj[:8] != 0)).to(dev)        # 1.3, 2.3, 3.3 -> 1, 2, 3
    for k in KEYS:
        assert torch.equal(eng.nspdk_features(raw, None, mol=True)[k], none[k]), k
    lab = torch.from_numpy(graph_sets()["mol9"][1][:8].copy()).to(dev)
    lab[5] = -1
    got = eng.nspdk_features(a, lab, mol=True)
    ip = got["nspdk_indptr"].cpu().numpy()
    assert ip[6] == ip[5] and ip[5] > ip[4] and ip[7] > ip[6]


def case_bad_arguments(lib, dev):
    eng = sample_ops(lib, dev)
    with pytest.raises(NotImplementedError, match=r"N = 65 is above CCSD_NSPDK_MAX_NODES = 64"):
        eng.nspdk_features(torch.zeros(1, 65, 65, device=dev))
    assert lib.ccsd_nspdk_row_capacity(65) == 0 and lib.ccsd_nspdk_row_capacity(0) == 0 and lib.ccsd_nspdk_workspace_bytes(0, 9) == 0
    assert lib.ccsd_nspdk_row_capacity(9) == 810 and lib.ccsd_nspdk_row_capacity(64) == 40960 and lib.ccsd_nspdk_row_capacity(1) == 10
    assert lib.ccsd_nspdk_workspace_bytes(3, 9) == 3 * 65536 * 4 and lib.ccsd_nspdk_workspace_bytes(100000, 9) == 512 * 65536 * 4
    with pytest.raises(ValueError, match=r"nspdk_features: adj must be \(B, N, N\)"):
        eng.nspdk_features(torch.zeros(1, 4, 5, device=dev))
    with pytest.raises(ValueError, match="labels must be integer"):
        eng.nspdk_features(torch.zeros(2, 4, 4, device=dev), torch.zeros(2, 5, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="labels must be integer"):
        eng.nspdk_features(torch.zeros(2, 4, 4, device=dev), torch.zeros(2, 4, device=dev))
    with pytest.raises(ValueError, match="thr"):
        eng.nspdk_features(torch.zeros(1, 4, 4, device=dev), thr=-1.0)
    with pytest.raises(KeyError, match="nspdk_values"):
        eng.nspdk_mmd({"nspdk_indptr": torch.zeros(2, dtype=torch.int64), "nspdk_indices": torch.zeros(0, dtype=torch.int32)}, {})
    assert lib.ccsd_nspdk_mmd_workspace_bytes(0, 1) == 0
    assert lib.ccsd_nspdk_mmd(None, None, None, 1, None, None, None, 1, None, 0, None, eng._stream()) != 0


# ---- the MMD ------------------------------------------------------------------------------------------------------------------------
def rows_slice(f, sl):
    """Rows sl of a CSR dict, as a CSR dict of its own."""
    ip = f["nspdk_indptr"]
    lo, hi = int(ip[sl.start]), int(ip[sl.stop])
    return {"nspdk_indptr": ip[sl.start:sl.stop + 1] - lo, "nspdk_indices": f["nspdk_indices"][lo:hi], "nspdk_values": f["nspdk_values"][lo:hi]}


def case_mmd(lib, dev, name):
    z, meta = e4()
    eng = sample_ops(lib, dev)
    f = feature_run(lib, dev, name)
    s1, s2 = split(name)
    got = eng.nspdk_mmd(rows_slice(f, s1), rows_slice(f, s2)).cpu().numpy()
    m = meta["sets"][name]
    print(f"nspdk mmd {name} on {dev}: {got[3]:.17g} reference {m['mmd']:.17g} (difference {got[3] - m['mmd']:.3g}; "
          f"the reference's pairwise form minus the mean form of its own rows: {m['pairwise_minus_mean_form']:.3g})")
    assert abs(got[3] - m["mmd"]) <= MMD_ATOL
    assert abs(got[0] + got[1] - 2 * got[2] - got[3]) == 0.0
    ref_rows = {"nspdk_indptr": torch.from_numpy(z[f"{name}/indptr"]).to(dev), "nspdk_indices": torch.from_numpy(z[f"{name}/indices"]).to(dev),
                "nspdk_values": torch.from_numpy(z[f"{name}/values"]).to(dev)}
    want = R.mmd_mean_form(*[tuple(rows_slice(ref_rows, s)[k].cpu().numpy() for k in KEYS) for s in (s1, s2)])
    assert np.abs(got - np.array(want)).max() <= MMD_ATOL


def case_mmd_self_and_empty_rows(lib, dev):
    """A set against itself gives 0; the fixture's self score of the reference is 0 within the same bound.  Empty rows: left out of
    the second set, zero vectors in the first."""
    _, meta = e4()
    eng = sample_ops(lib, dev)
    f = feature_run(lib, dev, "mol9")
    print(f"nspdk mmd of mol9 against itself: reference {meta['self']['mmd']:.3g}")
    assert abs(meta["self"]["mmd"]) <= MMD_ATOL and meta["self"]["set"] == "mol9"
    for name in SET_NAMES:
        g = feature_run(lib, dev, name)
        assert abs(float(eng.nspdk_mmd(g, g)[3])) <= MMD_ATOL, name
    a, b = rows_slice(f, slice(0, 32)), rows_slice(f, slice(32, 64))
    base = eng.nspdk_mmd(a, b).cpu().numpy()
    ipb = b["nspdk_indptr"]
    b_pad = dict(b, nspdk_indptr=torch.cat([ipb[:5], ipb[4:5], ipb[5:], ipb[-1:]]))                      # two empty rows added to the second set
    assert np.array_equal(eng.nspdk_mmd(a, b_pad).cpu().numpy(), base)
    ipa = a["nspdk_indptr"]
    a_pad = dict(a, nspdk_indptr=torch.cat([ipa, ipa[-1:].expand(32)]))                                  # 32 empty rows added to the first: its mean halves
    got = eng.nspdk_mmd(a_pad, b).cpu().numpy()
    want = np.array([base[0] / 4, base[1], base[2] / 2, base[0] / 4 + base[1] - base[2]])
    assert np.abs(got - want).max() <= MMD_ATOL


# ---- evaluation.py ------------------------------------------------------------------------------------------------------------------
def sides(name, dev):
    adj, lab = graph_sets()[name]
    s1, s2 = split(name)
    return [{"adj": torch.from_numpy(adj[s].astype(np.float32)).to(dev), "nspdk_labels": torch.from_numpy(lab[s]).to(dev)} for s in (s1, s2)]


def case_scores(lib, dev):
    _, meta = e4()
    kw = dict(device=dev, lib=lib, mol=True)
    for name in ("mol9", "shapes"):
        ref, pred = sides(name, dev)
        want = meta["sets"][name]["mmd"]
        got = ev.eval_torch_batch(ref, pred, ["nspdk"], nspdk=True, **kw)
        assert list(got) == ["nspdk"] and abs(got["nspdk"] - want) <= MMD_ATOL and round(got["nspdk"], 6) == round(want, 6), (name, got, want)
        assert ev.nspdk_stats(ref, pred, **kw) == got["nspdk"]
    ref, pred = sides("mol9", dev)
    want = meta["sets"]["mol9"]["mmd"]
    # the rows computed once serve as a side; describe adds them with the keyword
    rows = [ev.nspdk_rows(s, kw) for s in (ref, pred)]
    assert ev.nspdk_stats(rows[0], rows[1], **kw) == ev.nspdk_stats(ref, pred, **kw)
    d = ev.describe(pred["adj"], mol=True, nspdk=True, nspdk_labels=pred["nspdk_labels"], device=dev, lib=lib)
    assert set(KEYS) <= set(d) and all(torch.equal(d[k], rows[1][k]) for k in KEYS)
    assert not [k for k in ev.describe(pred["adj"], mol=True, device=dev, lib=lib) if k.startswith("nspdk")]
    dr = ev.describe(ref["adj"], mol=True, nspdk=True, nspdk_labels=ref["nspdk_labels"], device=dev, lib=lib)
    both = ev.eval_torch_batch(dr, d, ["degree", "nspdk"], nspdk=True, **kw)
    assert list(both) == ["degree", "nspdk"] and both["nspdk"] == ev.nspdk_stats(ref, pred, **kw)
    # labels from x: the first channel above 0.5, -1 where there is none
    lab = graph_sets()["mol9"][1]
    chan = {6: 0, 7: 1, 8: 2, 9: 3}
    x = np.zeros(lab.shape + (4,), np.float32)
    for (b, i), l in np.ndenumerate(lab):
        if l >= 0:
            x[b, i, chan[int(l)]] = 0.9
            x[b, i, 3] = max(x[b, i, 3], 0.6 if chan[int(l)] < 3 and (b + i) % 3 == 0 else 0.0)          # a later channel above 0.5 too
    ml = ev.mol_labels(torch.from_numpy(x))
    assert ml.dtype == torch.int32 and np.array_equal(ml.numpy(), np.vectorize(lambda l: chan.get(int(l), -1))(lab))
    s1, s2 = split("mol9")
    adj = graph_sets()["mol9"][0]
    by_x = [{"adj": torch.from_numpy(adj[s].astype(np.float32)), "x": torch.from_numpy(x[s])} for s in (s1, s2)]
    by_l = [{"adj": torch.from_numpy(adj[s].astype(np.float32)), "nspdk_labels": ml[s]} for s in (s1, s2)]
    assert ev.nspdk_stats(*by_x, **kw) == ev.nspdk_stats(*by_l, **kw)
    assert ev.nspdk_stats(*by_x, **kw) != ev.nspdk_stats(*by_x, device=dev, lib=lib)                     # (without mol: label 0, edge label 1)
    with pytest.raises(KeyError, match="nspdk_indptr"):
        ev.nspdk_stats({"degree_hist": torch.zeros(2, 9)}, pred, **kw)
    # a predicted graph without a node is left out
    lab_e = torch.cat([pred["nspdk_labels"], torch.full((1, 9), -1, dtype=torch.int32, device=dev)])
    adj_e = torch.cat([pred["adj"], torch.zeros(1, 9, 9, device=dev)])
    assert ev.nspdk_stats(ref, {"adj": adj_e, "nspdk_labels": lab_e}, **kw) == ev.nspdk_stats(ref, pred, **kw)
    assert abs(ev.nspdk_stats(ref, ref, **kw)) <= MMD_ATOL and math.isfinite(want)


def case_opt_in(lib, dev):
    kw = dict(device=dev, lib=lib)
    adj = torch.from_numpy((graph_sets()["shapes"][0] != 0).astype(np.float32))
    for extra in ({}, {"spectra": True}, {"orbits": True}, {"spectra": True, "orbits": True}):
        with pytest.raises(NotImplementedError, match="nspdk.*nspdk=True"):
            ev.eval_torch_batch(adj, adj, ["degree", "nspdk"], **extra, **kw)
    assert "nspdk=True" in ev.UNSUPPORTED["nspdk"]
    assert list(ev.eval_torch_batch(adj, adj, nspdk=True, **kw)) == ["degree", "cluster"]                # never a default
    assert list(ev.eval_torch_batch(adj, adj, nspdk=True, orbits=True, spectra=True, **kw)) == ["degree", "cluster", "orbit", "spectral"]
    got = ev.eval_torch_batch(adj, adj, ["nspdk", "degree"], nspdk=True, **kw)
    assert list(got) == ["nspdk", "degree"] and abs(got["nspdk"]) <= MMD_ATOL
    assert list(ev.eval_torch_batch(adj, adj, ["nspdk"], nspdk=True, **kw)) == ["nspdk"]
    # a dict side needs the histograms of the methods asked for and no others
    rows = ev.nspdk_rows(adj, kw)
    assert list(ev.eval_torch_batch(rows, rows, ["nspdk", "nspdk"], nspdk=True, **kw)) == ["nspdk"]
    with pytest.raises(KeyError, match="degree_hist"):
        ev.eval_torch_batch(rows, rows, ["nspdk", "degree"], nspdk=True, **kw)
    with pytest.raises(NotImplementedError, match="rank0_distrib"):
        ev.eval_CC_batch({}, {}, {}, ["rank0_distrib"], **kw)
    with pytest.raises(NotImplementedError, match="CCSD_NSPDK_MAX_NODES"):
        ev.eval_torch_batch(torch.zeros(2, 65, 65), torch.zeros(2, 65, 65), ["nspdk"], nspdk=True, **kw)


# ---- Sampler.evaluate ---------------------------------------------------------------------------------------------------------------
def case_sampler_evaluate(lib, tmp_path):
    """Sampler.evaluate(out, held, nspdk=True) on a finished qm9_CC run of two steps: exactly the "nspdk" key is added, finite and in
    [-1e-9, 2]; labels come from x of each side; the saved .npz scores identically; a side without x or labels is refused; the result
    dict is not written to."""
    import os

    from tests.test_harness import QM9_CC_YAML, run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2)
    assert c.sampler.is_mol
    keys = set(out)
    adj, lab = graph_sets()["mol9"]
    chan = {6: 0, 7: 1, 8: 2, 9: 3}
    x = np.zeros((16, 9, 4), np.float32)
    for (b, i), l in np.ndenumerate(lab[:16]):
        if l >= 0:
            x[b, i, chan[int(l)]] = 1
    held = {"adj": torch.from_numpy(adj[:16].astype(np.float32)), "x": torch.from_numpy(x)}
    base = c.sampler.evaluate(out, held)
    got = c.sampler.evaluate(out, held, nspdk=True)
    assert set(got) == set(base) | {"nspdk"} and {k: got[k] for k in base} == base, (got, base)
    assert math.isfinite(got["nspdk"]) and -1e-9 <= got["nspdk"] <= 2.0, got
    assert set(out) == keys and not [k for k in keys if k.startswith("nspdk")]
    # the same number from the pieces: mol_labels of each side's x, the quantised adjacency as sampled
    kw = dict(device=c.sampler.device0, lib=lib, mol=True)
    want = ev.nspdk_stats({"adj": held["adj"], "nspdk_labels": ev.mol_labels(held["x"])}, {"adj": out["adj"], "nspdk_labels": ev.mol_labels(out["x"])}, **kw)
    assert got["nspdk"] == want
    held_l = {"adj": held["adj"], "nspdk_labels": ev.mol_labels(held["x"])}
    assert c.sampler.evaluate(out, held_l, nspdk=True) == got
    (fname,) = os.listdir(tmp_path / "samples")
    saved = str(tmp_path / "samples" / fname)
    assert c.sampler.evaluate(saved, held, nspdk=True) == got
    same = c.sampler.evaluate(out, saved, nspdk=True)
    assert abs(same["nspdk"]) <= MMD_ATOL, same
    with pytest.raises(KeyError, match="nspdk_labels"):
        c.sampler.evaluate(out, {"adj": held["adj"]}, nspdk=True)
    with pytest.raises(KeyError, match="nspdk_labels"):
        c.sampler.evaluate(out, held["adj"], nspdk=True)
    with pytest.raises(NotImplementedError, match="nspdk"):
        c.sampler.evaluate(out, held, methods=["nspdk"])


def case_sampler_evaluate_generic(lib, tmp_path):
    """Sampler.evaluate(out, held_adjacency_batch, nspdk=True) on a finished gdss_community_small run of two steps -- not a molecule
    sampler: every slot is a node with label 0 and every edge has label 1.  Exactly the "nspdk" key is added; it is
    nspdk_stats(held, out["adj"]); a dict side and the saved .npz score identically."""
    import os

    from tests.orbit_cases import GRAPH_YAML
    from tests.test_harness import run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_community_small", GRAPH_YAML, max_steps=2, rounds=1)
    assert not c.sampler.is_mol
    keys = set(out)
    N = out["adj"].shape[1]
    rng = np.random.default_rng(5)
    u = np.triu(rng.random((12, N, N)) < 0.2, 1)
    held = torch.from_numpy((u | u.transpose(0, 2, 1)).astype(np.float32))
    base = c.sampler.evaluate(out, held)
    got = c.sampler.evaluate(out, held, nspdk=True)
    assert set(got) == set(base) | {"nspdk"} and {k: got[k] for k in base} == base, (got, base)
    assert math.isfinite(got["nspdk"]) and -1e-9 <= got["nspdk"] <= 2.0, got
    assert set(out) == keys and not [k for k in keys if k.startswith("nspdk")]
    kw = dict(device=c.sampler.device0, lib=lib)
    assert got["nspdk"] == ev.nspdk_stats(held, out["adj"], **kw)
    assert c.sampler.evaluate(out, {"adj": held}, nspdk=True) == got
    both = c.sampler.evaluate(out, held, nspdk=True, orbits=True)
    assert list(both) == ["degree", "cluster", "orbit", "nspdk"] and both["nspdk"] == got["nspdk"]
    (fname,) = os.listdir(tmp_path / "samples")
    assert c.sampler.evaluate(str(tmp_path / "samples" / fname), held, nspdk=True) == got
