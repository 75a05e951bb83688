"""Shared cases for the spectral scores (ccsd_eigvalsh, ccsd_spectral_hist, ccsd_hodge_spectrum, ccsd_amd/evaluation.py): run by
tests/test_spectrum.py over the host emulation and by tests/test_gpu_spectrum.py on the device.

Expected values come from two places.  tests/golden/e2_spectrum.npz (tools/make_golden.py spectrum) holds small graph and complex sets
with what the REFERENCE's own spectral_worker, spectral_stats, hodge_laplacian_spectrum_worker, hodge_laplacian_spectrum_stats,
eval_graph_list and eval_CC_list return for them, with the discrepancies measured at generation: lp_vs_closed (linear program against
closed form, per score), f32_vs_f64 (the reference's float32 LAPACK eigenvalues and scores against float64 ones) and edge_margin (the
distance of the reference's eigenvalues from the interior bin edges, >= 1e-9 in the sets compared count by count).  The numpy
restatements below need no networkx at test time.

Tolerances.  Solver: |w - numpy.linalg.eigvalsh| <= 64 n 2^-53 ||A||_F per eigenvalue (both solvers are backward stable with constants
of low degree in n; the factor leaves room for another summation order and FMA contraction); the largest ratio seen is printed.
Histogram counts: exact.  Hodge spectra: 1 float32 ulp of the largest eigenvalue against the float64 restatement, 4 x the recorded
f32_vs_f64 of the set against the reference's float32 spectra.  Scores: 1e-12 against float64 restatements and tv scores,
max(4 x the recorded discrepancy of that score, 1e-12) against emd and hodge scores -- the rule of tests/eval_cases.py."""
import ctypes as C
import json
import math
from itertools import combinations

import numpy as np
import pytest
import torch

from ccsd_amd import _lib
from ccsd_amd import evaluation as ev
from tests.helpers import load_golden, sample_ops

TOL = 1e-12
SOLVER_SIZES = (1, 2, 3, 7, 63, 64, 65, 77, 128, 129, 190)      # (77: dynamic + static LDS first pass 64 KB together)
SOLVER_FACTOR = 64.0
BINS = 200
_e2 = {}


def e2():
    if not _e2:
        z = load_golden("e2_spectrum.npz")
        _e2["z"], _e2["meta"] = z, json.loads(str(z["meta"]))
    return _e2["z"], _e2["meta"]


# ---- solver -------------------------------------------------------------------------------------------------------------------------
def norm_laplacian(w):
    """I - D^-1/2 W D^-1/2 over the nodes of positive degree, float64 (the definition of include/ccsd_hip.h); [[0]] without an edge."""
    w = np.asarray(w, np.float64) * (1 - np.eye(len(w)))
    keep = w.sum(1) > 0
    if not keep.any():
        return np.zeros((1, 1))
    w = w[keep][:, keep]
    d = w.sum(1)
    return np.eye(len(d)) - w / np.sqrt(d[:, None] * d[None, :])


def solver_matrices(n, B=5, seed=0):
    """kind -> (B', n, n) float64 symmetric matrices of the kinds the issue lists (those that exist at this n)."""
    rng = np.random.default_rng(1000 * n + seed)
    sym = lambda a: (a + a.transpose(0, 2, 1)) / 2
    out = {"zero": np.zeros((B, n, n))}
    d = np.zeros((B, n, n))
    d[:, np.arange(n), np.arange(n)] = rng.standard_normal((B, n)) * 10.0 ** rng.integers(-3, 4, (B, 1))
    out["diagonal"] = d
    u = rng.standard_normal((B, n, 1))
    out["identity_rank1"] = 3.0 * np.eye(n)[None] + u @ u.transpose(0, 2, 1)
    out["random"] = sym(rng.standard_normal((B, n, n)))
    r = max(1, n // 8)
    f = rng.integers(0, 2, (B, n, r)).astype(np.float64)
    out["integer_psd"] = f @ f.transpose(0, 2, 1)                      # rank <= n / 8: many zero eigenvalues
    if n >= 2:
        path = np.zeros((n, n))
        path[np.arange(n - 1), np.arange(1, n)] = 1
        out["laplacian_path"] = norm_laplacian(path + path.T)[None]
        # the overflow trap: an entry of 1e-200 beside a diagonal gap of 1, met in the first round of the first sweep (pair (1, m - 2) of
        # the round-robin order; the pair (0, 1) at n = 2), the rest random
        t = sym(rng.standard_normal((1, n, n)))
        p, q = (0, 1) if n == 2 else (1, ((n + 1) & ~1) - 2)
        t[0, p, p], t[0, q, q] = 0.0, 1.0
        t[0, p, q] = t[0, q, p] = 1e-200
        out["trap"] = t
    if n == 7:
        k44 = np.zeros((8, 8))
        k44[:4, 4:] = 1
        out["laplacian_k44"] = norm_laplacian(k44 + k44.T)[None]       # (8 x 8: rides with the n = 7 case)
    return out


def check_solver(eng, dev, a, kind, diagonal=False, twice=True):
    """All solver properties on one batch; returns the largest |w - numpy| in units of n 2^-53 ||A||_F."""
    n = a.shape[1]
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = t.clone()
    w, sw = eng.eigvalsh(t, sweeps=True)
    assert torch.equal(t, keep), kind                                                  # the input is not modified
    if twice:
        w2, sw2 = eng.eigvalsh(t, sweeps=True)
        assert torch.equal(w, w2) and torch.equal(sw, sw2), kind                       # two calls: the same bits
    w, sw = w.cpu().numpy(), sw.cpu().numpy()
    assert w.shape == (a.shape[0], n) and w.dtype == np.float64
    assert (np.diff(w, axis=1) >= 0).all(), kind                                       # ascending
    ref = np.linalg.eigvalsh(a)
    fro = np.sqrt((a * a).sum((1, 2)))
    unit = n * 2.0 ** -53 * fro
    bound = SOLVER_FACTOR * unit
    err = np.abs(w - ref).max(1)
    assert (err <= bound).all(), (kind, n, (err / np.maximum(unit, 1e-300)).max())
    assert (np.abs(w.sum(1) - np.trace(a, axis1=1, axis2=2)) <= bound).all(), kind
    assert (np.abs((w * w).sum(1) - fro * fro) <= bound * fro).all(), kind
    off = np.sqrt(np.maximum(fro * fro - (np.diagonal(a, axis1=1, axis2=2) ** 2).sum(1), 0.0))
    assert ((sw >= 0) & (sw < _lib.EIG_MAX_SWEEPS)).all(), (kind, sw)
    if diagonal:
        assert (sw <= 1).all(), (kind, sw)
    else:
        assert (sw[off > 1e-8 * fro] > 0).all(), (kind, sw)                           # an off-diagonal part costs at least one sweep
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


def case_solver(lib, dev, n, B=5, kinds=None, twice=True):
    eng = sample_ops(lib, dev)
    worst = {}
    for kind, a in solver_matrices(n, B).items():
        if kinds is None or kind in kinds:
            worst[kind] = check_solver(eng, dev, a, kind, diagonal=kind in ("zero", "diagonal"), twice=twice)
    print(f"eigvalsh n = {n} on {dev}: largest |w - numpy| / (n 2^-53 ||A||_F) = {max(worst.values()):.3f}  {worst}")
    return max(worst.values())


def case_solver_trap(lib, dev):
    """The 2 x 2 of the issue, a_pq = 1e-200 beside a diagonal gap of 1: eigenvalues 0 and 1, nothing overflows.  NO rotation runs
    here: off(A) is below the stopping threshold from the start (in a 2 x 2 a huge theta always means a converged matrix), so this case
    pins the early exit and the sort only.  The rotation's large-|theta| branch is reached by the "trap" kind of solver_matrices at
    n >= 3, where the tiny entry sits in a pair of the first round while the rest of the matrix keeps the sweep going."""
    a = np.array([[[0.0, 1e-200], [1e-200, 1.0]], [[5.0, 1e-200], [1e-200, 4.0]]])
    w = sample_ops(lib, dev).eigvalsh(torch.from_numpy(a).to(dev)).cpu().numpy()
    assert np.array_equal(w, [[0.0, 1.0], [4.0, 5.0]]), w


def case_solver_bad_dims(lib, dev):
    eng = sample_ops(lib, dev)
    a = torch.zeros((1, 4, 4), dtype=torch.float64, device=dev)
    w = torch.zeros((1, 4), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.ccsd_eigvalsh(p(a), 0, 4, p(w), None, None, 0, None) == _lib.ERR_INVALID
    assert lib.ccsd_eigvalsh(p(a), 1, 0, p(w), None, None, 0, None) == _lib.ERR_INVALID
    assert lib.ccsd_eigvalsh(p(a), 1, 513, p(w), None, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert b"513" in lib.ccsd_last_error() and b"O(n^3)" in lib.ccsd_last_error()
    assert lib.ccsd_eigvalsh(p(a), 1, 129, p(w), None, None, 0, None) == _lib.ERR_WORKSPACE       # (checked before anything is read)
    assert lib.ccsd_eig_workspace_bytes(7, 128) == 0
    slabs = 256 if lib.is_hip else 2                      # CCSD_EIG_MAX_GRID: the emulation walks with two, to reuse a slab in small batches
    assert lib.ccsd_eig_workspace_bytes(min(7, slabs), 129) == min(7, slabs) * 129 * 129 * 8
    assert lib.ccsd_eig_workspace_bytes(100000, 512) == slabs * 512 * 513 * 8                    # does not grow with B
    assert lib.ccsd_eig_workspace_bytes(1, 513) == 0
    with pytest.raises(NotImplementedError, match="600"):
        eng.eigvalsh(torch.zeros((1, 600, 600), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        eng.eigvalsh(torch.zeros((1, 4, 4), dtype=torch.float32, device=dev))
    single = eng.eigvalsh(torch.diag(torch.tensor([3.0, -1.0, 2.0], dtype=torch.float64)).to(dev))
    assert single.tolist() == [-1.0, 2.0, 3.0]


def case_solver_batch_walk(lib, dev):
    """More matrices than workspace slabs at n = 129: a workgroup walks the batch and reuses its slab (260 matrices over the device's
    256 slabs, 5 over the emulation's 2).  Every matrix differs, so a stale slab would show."""
    B, n = (260, 129) if lib.is_hip else (5, 129)
    assert lib.ccsd_eig_workspace_bytes(B, n) < B * n * (n | 1) * 8
    rng = np.random.default_rng(129)
    a = rng.standard_normal((B, n, n)) * (1.0 + np.arange(B))[:, None, None]
    a = (a + a.transpose(0, 2, 1)) / 2
    w, sw = sample_ops(lib, dev).eigvalsh(torch.from_numpy(a).to(dev), sweeps=True)
    w, sw = w.cpu().numpy(), sw.cpu().numpy()
    bound = SOLVER_FACTOR * n * 2.0 ** -53 * np.sqrt((a * a).sum((1, 2)))
    assert (np.abs(w - np.linalg.eigvalsh(a)).max(1) <= bound).all()
    assert ((sw > 0) & (sw < _lib.EIG_MAX_SWEEPS)).all()


# ---- spectral histograms ------------------------------------------------------------------------------------------------------------
def quantised(adj, mol, thr=0.5):
    adj = np.asarray(adj, np.float32)
    if mol:
        return np.where(adj >= 2.5, 3, np.where(adj >= 1.5, 2, np.where(adj >= 0.5, 1, 0)))
    return np.where(adj < thr, 0, 1)


def numpy_spectral(adj, mol, thr=0.5):
    """(counts (B, 200), eigenvalues (B, N), n_eff (B,)) of include/ccsd_hip.h's definition, in float64 numpy."""
    q = quantised(adj, mol, thr)
    edges = np.linspace(-1e-5, 2, BINS + 1)
    cs, es, ns = [], [], []
    for a in q:
        w = np.clip(np.linalg.eigvalsh(norm_laplacian(a)), 0.0, 2.0)
        c = np.histogram(w, bins=BINS, range=(-1e-5, 2))[0]
        by_table = np.minimum(np.searchsorted(edges, w, side="right") - 1, BINS - 1)      # the largest i with edges[i] <= v, last bin closed
        assert np.array_equal(np.bincount(by_table, minlength=BINS), c)
        cs.append(c)
        es.append(np.pad(w, (0, len(a) - len(w))))
        ns.append(len(w))
    return np.stack(cs).astype(np.int32), np.stack(es), np.array(ns, np.int32)


_spectral_runs = {}


def spectral_run(lib, dev, name):
    key = (dev, name)
    if key not in _spectral_runs:
        z, meta = e2()
        adj = torch.from_numpy(z[f"graphs/{name}/adj"].astype(np.float32)).to(dev)
        res = sample_ops(lib, dev).spectral_hist(adj, mol=meta["graph_sets"][name]["mol"], eig=True)
        _spectral_runs[key] = {k: v.cpu().numpy() for k, v in res.items()}
    return _spectral_runs[key]


def exact_graph_sets():
    return [k for k, v in e2()[1]["graph_sets"].items() if v["exact"]]


def case_spectral(lib, dev, name):
    """Counts bit-exact against the reference's spectral_worker (fixture) and the restatement; eigenvalues to the solver's bound."""
    z, meta = e2()
    info = meta["graph_sets"][name]
    assert info["exact"] and info["edge_margin"] >= 1e-9 and not info["bipartite_component"]
    got = spectral_run(lib, dev, name)
    counts, eig, n_eff = numpy_spectral(z[f"graphs/{name}/adj"], info["mol"])
    assert got["spectral_hist"].dtype == np.int32 and got["spectral_hist"].shape == (info["B"], BINS)
    assert np.array_equal(got["spectral_n"], n_eff) and np.array_equal(got["spectral_n"], z[f"graphs/{name}/n_eff"]), name
    assert np.array_equal(got["spectral_hist"], z[f"graphs/{name}/counts"]), name
    assert np.array_equal(got["spectral_hist"], counts), name
    assert (got["spectral_hist"].sum(1) == n_eff).all()
    N = info["N"]
    bound = SOLVER_FACTOR * N * 2.0 ** -53 * math.sqrt(2.0 * N)           # (||L||_F <= sqrt(n + n): unit diagonal, off-diagonal squares sum to <= n)
    assert np.abs(got["spectral_eig"] - eig).max() <= bound
    assert np.abs(got["spectral_eig"] - z[f"graphs/{name}/eig"]).max() <= bound + 4 * info["restated_vs_reference_eig"]
    for b in range(info["B"]):
        assert (got["spectral_eig"][b, n_eff[b]:] == 0).all()


def case_spectral_mol9(lib, dev):
    """mol9: bond orders are the weights.  Its graphs hold bipartite components, so the expected counts are the float64 restatement with
    the clamp; the reference's own counts agree wherever it kept every eigenvalue."""
    z, meta = e2()
    info = meta["graph_sets"]["mol9"]
    assert info["mol"]
    got = spectral_run(lib, dev, "mol9")
    counts, eig, n_eff = numpy_spectral(z["graphs/mol9/adj"], True)
    want = z["graphs/mol9/expected_counts"] if "graphs/mol9/expected_counts" in z.files else z["graphs/mol9/counts"]
    assert np.array_equal(got["spectral_hist"], counts) and np.array_equal(got["spectral_hist"], want)
    assert np.array_equal(got["spectral_n"], z["graphs/mol9/n_eff"])
    for b, kept in enumerate(info["reference_kept_all"]):
        if kept:
            assert np.array_equal(got["spectral_hist"][b], z["graphs/mol9/counts"][b])
    assert np.abs(got["spectral_eig"] - eig).max() <= SOLVER_FACTOR * 9 * 2.0 ** -53 * math.sqrt(18.0)
    unweighted = numpy_spectral((z["graphs/mol9/adj"] != 0).astype(np.float32), False)[1]
    assert np.abs(got["spectral_eig"] - unweighted).max() > 1e-3                        # (the weights matter)


def case_spectral_landmarks(lib, dev):
    """Bipartite landmarks (path, even cycle, star, grid, path + cycle): the eigenvalue 2 counts in bin 199 however it is rounded, as many
    zeros in bin 0 as components; the counts equal the float64 restatement with the clamp (the fixture's expected value)."""
    z, meta = e2()
    got = spectral_run(lib, dev, "bip")
    h = got["spectral_hist"]
    assert np.array_equal(h, z["graphs/bip/expected_counts"]) and np.array_equal(h, numpy_spectral(z["graphs/bip/adj"], False)[0])
    assert h[:, 199].tolist() == [1, 1, 1, 1, 2] and h[:, 0].tolist() == [1, 1, 1, 1, 2]
    assert got["spectral_n"].tolist() == [6, 8, 7, 12, 10] and (h.sum(1) == got["spectral_n"]).all()


def case_spectral_small(lib, dev):
    """Edgeless graph -> one count in bin 0; a single edge -> bins 0 and 199; isolated and masked nodes are not counted; a diagonal of
    ones is ignored; raw samples give the counts of their quantised form; mol mode weighs by bond order."""
    eng = sample_ops(lib, dev)
    a = np.zeros((5, 6, 6), np.float32)
    a[1, 1, 4] = a[1, 4, 1] = 1                                                    # a single edge among isolated nodes
    for i, j in ((0, 1), (1, 2), (0, 2), (2, 3)):                                  # triangle + tail, nodes 4 and 5 masked
        a[2, i, j] = a[2, j, i] = 1
    a[3] = a[2]
    a[3][np.diag_indices(6)] = 1                                                   # ... with a diagonal of ones
    a[4][np.diag_indices(6)] = 1                                                   # a diagonal only: edgeless
    res = eng.spectral_hist(torch.from_numpy(a).to(dev), eig=True)
    h, n = res["spectral_hist"].cpu().numpy(), res["spectral_n"].cpu().numpy()
    assert n.tolist() == [1, 2, 4, 4, 1]
    assert h[0].tolist() == [1] + [0] * 199 and h[4].tolist() == [1] + [0] * 199
    assert h[1, 0] == 1 and h[1, 199] == 1 and h[1].sum() == 2
    assert np.array_equal(h[2], h[3]) and h[2].sum() == 4 and h[2, 0] == 1
    assert np.array_equal(h, numpy_spectral(a, False)[0])
    # raw samples: any values on either side of the threshold
    rng = np.random.default_rng(5)
    raw = np.where(a > 0, 0.5 + 0.5 * rng.random(a.shape), 0.5 * rng.random(a.shape) - 0.01).astype(np.float32)
    raw = np.triu(raw, 1) + np.triu(raw, 1).transpose(0, 2, 1)
    assert np.array_equal(eng.spectral_hist(torch.from_numpy(raw).to(dev))["spectral_hist"].cpu().numpy(), h)
    # bond orders are weights: a triangle with one triple bond has another spectrum than the plain triangle (0, 1.5, 1.5)
    m = np.zeros((1, 3, 3), np.float32)
    m[0, 0, 1] = m[0, 1, 0] = 3
    m[0, 1, 2] = m[0, 2, 1] = m[0, 0, 2] = m[0, 2, 0] = 1
    hm = eng.spectral_hist(torch.from_numpy(m).to(dev), mol=True, eig=True)
    hq = eng.spectral_hist(torch.from_numpy(m).to(dev), mol=False, eig=True)
    assert np.array_equal(hm["spectral_hist"].cpu().numpy(), numpy_spectral(m, True)[0])
    assert np.abs(hm["spectral_eig"].cpu().numpy() - numpy_spectral(m, True)[1]).max() < 1e-14
    assert np.abs(hm["spectral_eig"].cpu().numpy() - hq["spectral_eig"].cpu().numpy()).max() > 0.01


def case_spectral_above_lds(lib, dev):
    """N = 130: the Laplacians go through the workspace-resident placement with per-graph orders (masked graphs: n_eff < N), more
    graphs than the emulation has slabs.  Eigenvalues to the solver's bound against the float64 restatement; the counts are the
    histogram of the returned eigenvalues (no margin was checked for this set, so the restatement's counts are not demanded)."""
    from tests.eval_cases import e1

    adj = np.concatenate([e1()[0]["graphs/r130/adj"]] * 2)[:3].astype(np.float32)
    adj[2, 100:, :] = adj[2, :, 100:] = 0                                              # a third graph with another order
    res = sample_ops(lib, dev).spectral_hist(torch.from_numpy(adj).to(dev), eig=True)
    h, e, n = (res[k].cpu().numpy() for k in ("spectral_hist", "spectral_eig", "spectral_n"))
    counts, eig, n_eff = numpy_spectral(adj, False)
    assert np.array_equal(n, n_eff) and len(set(n.tolist())) == 3 and n.max() > 128
    assert np.abs(e - eig).max() <= SOLVER_FACTOR * 130 * 2.0 ** -53 * math.sqrt(260.0)
    for b in range(3):
        assert np.array_equal(h[b], np.histogram(np.clip(e[b, :n[b]], 0.0, 2.0), bins=BINS, range=(-1e-5, 2))[0])
        assert (e[b, n[b]:] == 0).all()


def case_spectral_bad_dims(lib, dev):
    eng = sample_ops(lib, dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    adj = torch.zeros((1, 4, 4), dtype=torch.float32, device=dev)
    edges = torch.from_numpy(np.linspace(-1e-5, 2, 201)).to(dev)
    hist = torch.zeros((1, 200), dtype=torch.int32, device=dev)
    ws = torch.zeros(1024, dtype=torch.float64, device=dev)
    call = lambda N, bins: lib.ccsd_spectral_hist(p(adj), 1, N, 0, 0.5, p(edges), bins, p(hist), None, None, p(ws), ws.numel() * 8, None)
    assert call(4, 200) == _lib.OK
    for N, bins in ((1, 200), (513, 200), (4, 0), (4, 1025)):
        assert call(N, bins) == _lib.ERR_INVALID, (N, bins)
    assert lib.ccsd_spectral_hist(p(adj), 1, 4, 0, 0.5, p(edges), 200, p(hist), None, None, p(ws), 8, None) == _lib.ERR_WORKSPACE
    assert lib.ccsd_spectral_workspace_bytes(1, 1) == 0 and lib.ccsd_spectral_workspace_bytes(1, 513) == 0
    with pytest.raises(ValueError):
        eng.spectral_hist(torch.zeros((1, 4, 4), dtype=torch.float32, device=dev), bins=0)
    with pytest.raises(ValueError):
        eng.spectral_hist(torch.zeros((1, 1, 1), dtype=torch.float32, device=dev))


# ---- hodge spectra ------------------------------------------------------------------------------------------------------------------
def numpy_hodge(adj, rank2, N, d_min, d_max, thr=0.5):
    """H (B, E, E) int64 by the cell rule: H[e][e'] = the number of present cells (columns of the quantised rank2 with any entry) that
    hold both edges, both edges being in the quantised graph."""
    cells = [c for d in range(d_min, d_max + 1) for c in combinations(range(N), d)]
    eidx = {e: i for i, e in enumerate(combinations(range(N), 2))}
    q = quantised(adj, False, thr)
    H = np.zeros((len(adj), len(eidx), len(eidx)), np.int64)
    for b in range(len(adj)):
        for k in np.nonzero(~(np.asarray(rank2[b], np.float32) < thr).all(0))[0]:
            el = [eidx[e] for e in combinations(cells[k], 2) if q[b, e[0], e[1]] != 0]
            H[b][np.ix_(el, el)] += 1
    return H


def hodge_inputs(name, side):
    z, meta = e2()
    info = meta["complex_sets"][name]
    g = lambda k: z[f"cc/{name}/{side}/{k}"]
    return info, g("x").astype(np.float32), g("adj").astype(np.float32), g("rank2").astype(np.float32), g("spectrum")


_hodge_runs = {}


def hodge_run(lib, dev, name, side):
    """describe(..., spectra=True) of one side of a fixture set: finish's cell bits feed the hodge spectrum."""
    key = (dev, name, side)
    if key not in _hodge_runs:
        info, x, adj, rank2, _ = hodge_inputs(name, side)
        t = lambda a: torch.from_numpy(a).to(dev)
        _hodge_runs[key] = ev.describe(t(adj), t(x), t(rank2), d_min=info["d_min"], d_max=info["d_max"], spectra=True, device=dev, lib=lib)
    return _hodge_runs[key]


def complex_sets():
    return list(e2()[1]["complex_sets"])


def case_hodge(lib, dev, name):
    z, meta = e2()
    for side in ("ref", "pred"):
        info, x, adj, rank2, ref32 = hodge_inputs(name, side)
        got = hodge_run(lib, dev, name, side)["hodge_spectrum"].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == ref32.shape == (len(adj), info["E"])
        assert (np.diff(got, axis=1) >= 0).all()
        H = numpy_hodge(adj, rank2, info["N"], info["d_min"], info["d_max"])
        want = np.linalg.eigvalsh(H.astype(np.float64)).astype(np.float32)
        ulp = np.spacing(np.abs(want).max(1).astype(np.float32))                       # 1 float32 ulp of the largest eigenvalue
        assert (np.abs(got.astype(np.float64) - want).max(1) <= ulp).all(), (name, side)
        assert np.abs(got.astype(np.float64) - ref32).max() <= 4 * meta["f32_vs_f64"][f"cc/{name}/eig"], (name, side)
        empty = ~H.any((1, 2))
        assert empty[1] and (got[empty] == 0).all()                                    # (complex 1 of every side has no cell: exact zeros)
        assert H.any()
    # a second call: the same bits (H is built without atomics, the solver sums in a fixed order)
    info, x, adj, rank2, _ = hodge_inputs(name, "ref")
    d = hodge_run(lib, dev, name, "ref")
    again = sample_ops(lib, dev).hodge_spectrum(torch.from_numpy(adj).to(dev), d["rank2_cell_bits"], d_min=info["d_min"], d_max=info["d_max"])
    assert torch.equal(again, d["hodge_spectrum"])


def case_hodge_small(lib, dev):
    """One, two and N nodes; a cell whose edges are partly absent from the graph; sweeps reported."""
    eng = sample_ops(lib, dev)
    N, d_min, d_max = 5, 3, 4
    cells = [c for d in range(d_min, d_max + 1) for c in combinations(range(N), d)]
    E, K = 10, len(cells)
    adj = np.zeros((5, N, N), np.float32)
    r2 = np.zeros((5, E, K), np.float32)
    adj[1, 0, 1] = adj[1, 1, 0] = 1                                                # two nodes, one edge, no cell can exist
    adj[2] = 1 - np.eye(N)                                                         # N nodes, complete graph, cells (0,1,2) and (0,1,2,3)
    r2[2, 0, cells.index((0, 1, 2))] = r2[2, 3, cells.index((0, 1, 2, 3))] = 1
    adj[3] = adj[2]
    adj[3, 0, 1] = adj[3, 1, 0] = adj[3, 2, 3] = adj[3, 3, 2] = 0                  # ... two of the cells' edges absent from the graph
    r2[3] = r2[2]
    r2[4, 5, cells.index((1, 2, 4))] = 1                                           # a cell over an edgeless graph: F is zero
    bits, _ = eng.rank2_cells(torch.from_numpy(r2).to(dev))
    got, sw = eng.hodge_spectrum(torch.from_numpy(adj).to(dev), bits, d_min=d_min, d_max=d_max, sweeps=True)
    got, sw = got.cpu().numpy(), sw.cpu().numpy()
    H = numpy_hodge(adj, r2, N, d_min, d_max)
    assert H[2].trace() == 3 + 6 and H[3].trace() == 2 + 4 and not H[[0, 1, 4]].any()
    want = np.linalg.eigvalsh(H.astype(np.float64)).astype(np.float32)
    assert (np.abs(got - want).max(1) <= np.spacing(np.abs(want).max(1))).all()
    assert (got[[0, 1, 4]] == 0).all() and sw[[0, 1, 4]].tolist() == [0, 0, 0] and (sw[[2, 3]] > 0).all() and (sw < _lib.EIG_MAX_SWEEPS).all()
    # N = 2: E = 1, no cell of three nodes
    one = eng.hodge_spectrum(torch.ones((1, 2, 2), dtype=torch.float32, device=dev), torch.zeros((1, 1), dtype=torch.int64, device=dev), d_min=2, d_max=2)
    assert one.shape == (1, 1) and one.item() == 0.0
    both = eng.hodge_spectrum(torch.ones((1, 2, 2), dtype=torch.float32, device=dev), torch.ones((1, 1), dtype=torch.int64, device=dev), d_min=2, d_max=2)
    assert both.item() == 1.0


def case_hodge_too_large(lib, dev):
    """E > 512 (N = 33: E = 528): CCSD_ERR_UNSUPPORTED from C, NotImplementedError naming the size from Python."""
    eng = sample_ops(lib, dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    adj = torch.zeros((1, 33, 33), dtype=torch.float32, device=dev)
    bits = torch.zeros((1, (math.comb(33, 3) + 63) // 64), dtype=torch.int64, device=dev)
    out = torch.zeros((1, 528), dtype=torch.float32, device=dev)
    ws = torch.zeros(16, dtype=torch.float64, device=dev)
    assert lib.ccsd_hodge_spectrum(p(adj), p(bits), 1, 33, 3, 3, 0, 0.5, p(out), None, p(ws), 128, None) == _lib.ERR_UNSUPPORTED
    assert b"528" in lib.ccsd_last_error()
    assert lib.ccsd_hodge_workspace_bytes(1, 33) == 0
    assert lib.ccsd_hodge_spectrum(p(adj), p(bits), 1, 1, 3, 3, 0, 0.5, p(out), None, p(ws), 128, None) == _lib.ERR_INVALID
    assert lib.ccsd_hodge_spectrum(p(adj), p(bits), 1, 5, 4, 3, 0, 0.5, p(out), None, p(ws), 128, None) == _lib.ERR_INVALID
    assert lib.ccsd_hodge_spectrum(p(adj), p(bits), 1, 5, 3, 3, 0, 0.5, p(out), None, p(ws), 128, None) == _lib.ERR_WORKSPACE
    with pytest.raises(NotImplementedError, match="528"):
        eng.hodge_spectrum(adj, bits, d_min=3, d_max=3)


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def numpy_mmd_emd(rows1, rows2, f32=False):
    """compute_mmd with gaussian_emd (sigma = 1, no scaling) on rows of equal mass, float64, by the closed form."""
    def pmf(r):
        r = np.asarray(r)
        s = r.sum()
        return (r.astype(np.float32) / np.float32(s)).astype(np.float64) if f32 else r.astype(np.float64) / s

    def disc(a, b):
        return np.mean([[math.exp(-(np.abs(np.cumsum(pmf(x)) - np.cumsum(pmf(y))).sum()) ** 2 / 2.0) for y in b] for x in a])

    return disc(rows1, rows1) + disc(rows2, rows2) - 2 * disc(rows1, rows2)


def score_tol(meta, key, table="lp_vs_closed"):
    return max(4 * meta[table].get(key, 0.0), TOL)


def case_spectral_scores(lib, dev):
    z, meta = e2()
    kw = dict(device=dev, lib=lib)
    t = lambda name: torch.from_numpy(z[f"graphs/{name}/adj"].astype(np.float32)).to(dev)
    for a, b in (("s12a", "s12b"), ("mol9", "s12b")):
        mol = meta["graph_sets"][a]["mol"]
        ra = sample_ops(lib, dev).spectral_hist(t(a), mol=mol)
        rb = sample_ops(lib, dev).spectral_hist(t(b))
        key = f"spectral/{a}_{b}"
        # (the emd scores say little about the histograms: with sigma = 1 and no distance scaling the kernel of two distinct 200-bin
        # histograms is ~0, so the score is ~1/n1 + 1/n2 = 0.58333 for both pairs.  The tv scores and the exact counts carry the check.)
        emd = ev.spectral_stats(ra, rb, ev.gaussian_emd, **kw)
        tv = ev.spectral_stats(ra, rb, ev.gaussian_tv, **kw)
        assert abs(emd - meta["scores"][key + "/emd"]) <= score_tol(meta, key + "/emd"), (key, emd, meta["scores"][key + "/emd"])
        assert abs(tv - meta["scores"][key + "/tv"]) <= TOL, (key, tv)
        assert abs(emd - numpy_mmd_emd(z[f"graphs/{a}/counts"], z[f"graphs/{b}/counts"])) <= TOL
        assert abs(ev.spectral_stats(ra, ra, **kw)) <= TOL                                  # a set against itself
    # raw batches through eval_torch_batch: the reference's rounded dict
    got = ev.eval_torch_batch(t("s12a"), t("s12b"), ["degree", "cluster", "spectral"], spectra=True, **kw)
    want = meta["eval_graph_list"]
    assert set(got) == set(want) == {"degree", "cluster", "spectral"}
    for m in got:
        slack = max(score_tol(meta, "spectral/s12a_s12b/emd" if m == "spectral" else f"eval_graph_list/{m}"), 1e-6 + TOL)
        assert abs(got[m] - want[m]) <= slack and (got[m] == want[m] or abs(got[m] - want[m]) <= 1.000001e-6), (m, got, want)
    # descriptor dicts: with spectral_hist, and with the adjacency to compute it from
    da, db = ev.describe(t("s12a"), spectra=True, **kw), ev.describe(t("s12b"), spectra=True, **kw)
    assert da["spectral_hist"].shape == (4, 200) and da["spectral_hist"].dtype == torch.int32 and "hodge_spectrum" not in da
    assert set(ev.describe(t("s12a"), **kw)) == set(da) - {"spectral_hist"}                 # the default leaves describe() as it was
    assert ev.eval_torch_batch(da, db, ["spectral"], spectra=True, **kw) == {"spectral": got["spectral"]}
    bare = {k: v for k, v in da.items() if k != "spectral_hist"}
    assert ev.eval_torch_batch(dict(bare, adj=t("s12a")), db, ["spectral"], spectra=True, **kw) == {"spectral": got["spectral"]}
    with pytest.raises(KeyError):
        ev.eval_torch_batch(bare, db, ["spectral"], spectra=True, **kw)
    assert set(ev.eval_torch_batch(t("s12a"), t("s12b"), spectra=True, **kw)) == {"degree", "cluster"}      # defaults unchanged


def cc_side(lib, dev, name, side, extra_empty=0):
    """The descriptor dict of one side (adj kept: eval_CC_batch computes the spectrum from adj and rank2_cell_bits), `extra_empty`
    complexes without any cell appended."""
    d = {k: v for k, v in hodge_run(lib, dev, name, side).items() if k != "hodge_spectrum"}
    info, x, adj, rank2, _ = hodge_inputs(name, side)
    d["adj"] = torch.from_numpy(adj).to(dev)
    if extra_empty:
        d = {k: torch.cat([v, torch.zeros((extra_empty,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)]) for k, v in d.items()}
    return d


def case_hodge_scores(lib, dev, name):
    z, meta = e2()
    kw = dict(device=dev, lib=lib)
    info = meta["complex_sets"][name]
    wk = info["worker_kwargs"]
    for tag, extra, nb in (("plain", 0, 1000), ("empties", 1, 1000), ("first2", 0, 2)):
        ref, pred = cc_side(lib, dev, name, "ref", extra), cc_side(lib, dev, name, "pred", extra)
        key = f"cc/{name}/{tag}/hodge"
        emd = ev.hodge_laplacian_spectrum_stats(ref, pred, wk, ev.gaussian_emd, cc_nb_eval=nb, **kw)
        tv = ev.hodge_laplacian_spectrum_stats(ref, pred, wk, ev.gaussian_tv, cc_nb_eval=nb, **kw)
        tol_emd = max(4 * meta["lp_vs_closed"][key + "/emd"], 4 * meta["f32_vs_f64"][key + "/emd"], TOL)
        tol_tv = max(4 * meta["f32_vs_f64"][key + "/tv"], TOL)
        assert abs(emd - meta["scores"][key + "/emd"]) <= tol_emd, (key, emd, meta["scores"][key + "/emd"], tol_emd)
        assert abs(tv - meta["scores"][key + "/tv"]) <= tol_tv, (key, tv, meta["scores"][key + "/tv"], tol_tv)
        got = ev.eval_CC_batch(ref, pred, wk, ["hodge_laplacian_spectrum", "rank1_distrib", "rank2_distrib"], cc_nb_eval=nb, spectra=True, **kw)
        want = meta[f"eval_CC_list/{name}/{tag}"]
        assert set(got) == set(want)
        for m in got:
            slack = tol_emd if m == "hodge_laplacian_spectrum" else score_tol(meta, f"eval_CC_list/{name}/{tag}/{m}")
            assert abs(got[m] - want[m]) <= slack + 1.000001e-6 and (got[m] == want[m] or abs(got[m] - want[m]) <= max(slack, 1.000001e-6)), (m, got, want)
    ref = cc_side(lib, dev, name, "ref")
    assert abs(ev.hodge_laplacian_spectrum_stats(ref, ref, wk, **kw)) <= TOL                    # a set against itself
    # a dict that carries hodge_spectrum is scored as it is
    full = hodge_run(lib, dev, name, "ref")
    assert abs(ev.hodge_laplacian_spectrum_stats(full, ref, wk, **kw)) <= TOL
    assert set(ev.eval_CC_batch(ref, ref, wk, spectra=True, **kw)) == {"rank1_distrib", "rank2_distrib"}      # defaults unchanged


def case_opt_in(lib, dev):
    """Without spectra=True both names still raise NotImplementedError naming the method and the keyword; orbit, nspdk and
    rank0_distrib stay refused either way."""
    kw = dict(device=dev, lib=lib)
    adj = torch.zeros((2, 4, 4), dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError, match="spectral.*spectra=True"):
        ev.eval_torch_batch(adj, adj, ["degree", "spectral"], **kw)
    with pytest.raises(NotImplementedError, match="hodge_laplacian_spectrum.*spectra=True"):
        ev.eval_CC_batch({}, {}, {}, ["hodge_laplacian_spectrum"], **kw)
    for spectra in (False, True):
        for m in ("orbit", "nspdk"):
            with pytest.raises(NotImplementedError, match=m):
                ev.eval_torch_batch(adj, adj, [m], spectra=spectra, **kw)
        with pytest.raises(NotImplementedError, match="rank0_distrib"):
            ev.eval_CC_batch({}, {}, {}, ["rank0_distrib"], spectra=spectra, **kw)
    with pytest.raises(KeyError):
        ev.eval_torch_batch(adj, adj, ["hodge_laplacian_spectrum"], spectra=True, **kw)


def case_sampler_evaluate(out, sampler, saved_path):
    """Sampler.evaluate(..., spectra=True) on a finished qm9_CC run: the two extra keys, finite; identical against the saved .npz; then
    a second run with sample(dense_rank2=False) is scored the same way."""
    keys = set(out)
    base = sampler.evaluate(out, out)
    assert set(base) == {"degree", "cluster", "rank1_distrib", "rank2_distrib"}            # the default is unchanged
    held = {k: out[k][:3] for k in ("adj", "degree_hist", "edge_hist", "n_nodes", "rank2_cell_hist", "rank2_cell_bits")}
    got = sampler.evaluate(out, held, spectra=True)
    assert set(got) == set(base) | {"spectral", "hodge_laplacian_spectrum"}, got
    assert all(math.isfinite(v) and -1e-9 <= v <= 2.0 for v in got.values()), got
    assert set(out) == keys
    same = sampler.evaluate(out, out, spectra=True)
    assert all(abs(v) <= 1e-12 for v in same.values()), same
    assert sampler.evaluate(out, saved_path, spectra=True) == same
    assert sampler.evaluate(saved_path, held, spectra=True) == got
    sparse = sampler.sample(save=False, dense_rank2=False)
    assert "rank2" not in sparse and "rank2_int" not in sparse and "rank2_cell_bits" in sparse
    again = sampler.evaluate(sparse, held, spectra=True)
    assert set(again) == set(got) and all(math.isfinite(v) and -1e-9 <= v <= 2.0 for v in again.values()), again
    assert all(abs(v) <= 1e-12 for v in sampler.evaluate(sparse, sparse, spectra=True).values())
