"""End-to-end distribution check of the production loop against the reference (tests/golden/d1_qm9_CC_n1000.npz: the per-complex
descriptors of ONE reference run of the shipped qm9_CC sampling set-up, 1000 scales, 256 complexes; tools/make_golden.py::d1_qm9_cc_n1000).

Samples cannot be compared value for value (the in-kernel Philox stream is not the reference's generator), so per-complex scalars are
compared in the mean with Welch's statistic:  |m_a - m_b| <= 5 sqrt(s2_a / n_a + s2_b / n_b),  each s2 floored at 1 / n of its sample
(the variance of an event seen once in n: a bin empty in one sample does not fail on a single occurrence in the other).  Five standard
errors over about twenty statistics is a false-alarm rate near 1e-5; the bound is a property of the test."""
import json

import numpy as np

from tests.helpers import load_golden

Z_MAX = 5.0


def fixture():
    g = load_golden("d1_qm9_CC_n1000.npz")
    return {k: g[k] for k in g.files if k != "meta"}, json.loads(str(g["meta"]))


def scalars(d, bins=None):
    """Per-complex scalars of a descriptor set {degree_hist, edge_hist, n_nodes, x_hist, cell_hist, rank2_nnz} -> {name: (n,) float64}.
    `bins`: the cell-size bins to include (default: those that are non-empty in `d`)."""
    eh, dh, ch = (np.asarray(d[k], np.float64) for k in ("edge_hist", "degree_hist", "cell_hist"))
    out = {"edges": eh[:, 1:].sum(-1), "bond_single": eh[:, 1], "bond_double": eh[:, 2], "bond_triple": eh[:, 3],
           "n_nodes": np.asarray(d["n_nodes"], np.float64)}
    for f in range(d["x_hist"].shape[1]):
        out[f"x_hist_{f}"] = np.asarray(d["x_hist"][:, f], np.float64)
    out["max_degree"] = np.array([np.nonzero(r)[0].max() for r in dh], np.float64)      # (bin 0 counts the slots without an edge)
    out["rank2_cells"] = ch.sum(-1)
    out["rank2_nnz"] = np.asarray(d["rank2_nnz"], np.float64)
    if bins is None:
        bins = nonempty_bins(d)
    for i in bins:
        out[f"cell_size_bin_{i}"] = ch[:, i]
    return out


def nonempty_bins(d):
    return [int(i) for i in np.nonzero(np.asarray(d["cell_hist"]).sum(0))[0]]


def welch(a, b):
    """(m_a, m_b, s2_a, s2_b, z): z = |m_a - m_b| / sqrt(s2_a / n_a + s2_b / n_b), variances (ddof 1) floored at 1 / n."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    va, vb = max(a.var(ddof=1), 1.0 / len(a)), max(b.var(ddof=1), 1.0 / len(b))
    return a.mean(), b.mean(), va, vb, abs(a.mean() - b.mean()) / np.sqrt(va / len(a) + vb / len(b))


def compare(sa, sb, label):
    """Prints every statistic, then asserts z <= Z_MAX for all of them."""
    assert set(sa) == set(sb)
    rows = {k: welch(sa[k], sb[k]) for k in sa}
    for k, (ma, mb, va, vb, z) in rows.items():
        print(f"{label} {k:18s} mean {ma:10.4f} vs {mb:10.4f}   var {va:10.4f} vs {vb:10.4f}   z {z:6.3f}")
    bad = {k: round(float(r[4]), 3) for k, r in rows.items() if not r[4] <= Z_MAX}
    assert not bad, f"{label}: means differ by more than {Z_MAX} standard errors: {bad}"
    return rows
