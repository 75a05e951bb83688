"""Shared cases for the evaluation of finished samples (ccsd_cluster_hist, ccsd_mmd, ccsd_amd/evaluation.py): run by tests/test_eval.py
over the host emulation and by tests/test_gpu_eval.py on the device.

Expected values come from two places.  tests/golden/e1_eval.npz (tools/make_golden.py eval) holds small graph sets and histogram sets with
what the REFERENCE's own clustering_worker, degree_worker, compute_mmd, eval_graph_list and eval_CC_list return for them; its gaussian_emd
ran on a stand-in pyemd (one linear program per pair), and meta["lp_vs_closed"] records, per score, the largest difference between a
program's kernel value and the closed form seen at generation.  The numpy restatements below (A @ A.T in int64, the np.linspace edge
table, float64 cdfs) cover the sizes the linear programs cannot: no networkx at test time.

Tolerances.  Histograms are integers: exact.  MMD against the float64 restatement and against the reference's gaussian_tv / gaussian
scores: 1e-12 absolute -- every disc is a mean of values in [0, 1] whose error is at most about (L + log2(n1 n2) + 10) 2^-53 <= 6e-14 at
L = 512, and the score weights four such terms.  Against the reference's gaussian_emd scores: 4 x the recorded discrepancy of that score,
floored at 1e-12 (measured at generation, not chosen)."""
import json

import numpy as np
import pytest
import torch

from ccsd_amd import evaluation as ev
from tests.helpers import load_golden, sample_ops

TOL = 1e-12
GRAPH_SETS = ("c07", "n17", "k65", "n2", "r65", "r130", "n512", "mol9", "small5", "diag12", "eval_ref", "eval_pred")
BINS = (10, 100)

_e1 = {}


def e1():
    if not _e1:
        z = load_golden("e1_eval.npz")
        _e1["z"], _e1["meta"] = z, json.loads(str(z["meta"]))
    return _e1["z"], _e1["meta"]


# ---- clustering ---------------------------------------------------------------------------------------------------------------------
def numpy_cluster(adj, mol, bins, thr=0.5):
    """(tri2 (B, N), cluster_hist (B, bins)) of include/ccsd_hip.h's definition, in numpy."""
    adj = np.asarray(adj, np.float32)
    B, N = adj.shape[:2]
    on = (adj >= 0.5) if mol else ~(adj < thr)
    A = (on & ~np.eye(N, dtype=bool)[None]).astype(np.int64)
    d = A.sum(-1)
    t2 = (A * (A @ A.transpose(0, 2, 1))).sum(-1)
    edges = np.linspace(0.0, 1.0, bins + 1)
    hist = np.zeros((B, bins), np.int32)
    for b in range(B):
        keep = d[b] > 0
        c = np.where(d[b] > 1, t2[b] / np.maximum(d[b] * (d[b] - 1), 1).astype(np.float64), 0.0)[keep]
        if not keep.any():
            c = np.zeros(1)                                                       # the one-node stand-in of an edgeless graph
        hist[b] = np.histogram(c, bins=bins, range=(0.0, 1.0))[0]
        # the edge-table rule is np.histogram's: the largest i with edges[i] <= c, the last bin closed
        by_table = np.minimum(np.searchsorted(edges, c, side="right") - 1, bins - 1)
        assert np.array_equal(np.bincount(by_table, minlength=bins), hist[b])
    return t2.astype(np.int32), hist


_cluster_runs = {}


def cluster_run(lib, dev, name, bins):
    key = (dev, name, bins)
    if key not in _cluster_runs:
        z, meta = e1()
        adj = torch.from_numpy(z[f"graphs/{name}/adj"].astype(np.float32)).to(dev)
        res = sample_ops(lib, dev).cluster_hist(adj, mol=meta["graph_sets"][name]["mol"], bins=bins)
        _cluster_runs[key] = {k: v.cpu().numpy() for k, v in res.items()}
    return _cluster_runs[key]


def case_cluster(lib, dev, name, bins):
    """tri2 and cluster_hist: bit-exact against the reference's clustering_worker (fixture) and against the restatement."""
    z, meta = e1()
    got = cluster_run(lib, dev, name, bins)
    adj = z[f"graphs/{name}/adj"]
    t2, hist = numpy_cluster(adj, meta["graph_sets"][name]["mol"], bins)
    assert got["cluster_hist"].dtype == np.int32 and got["cluster_hist"].shape == hist.shape
    assert np.array_equal(got["tri2"], t2), name
    assert np.array_equal(got["cluster_hist"], hist), name
    assert np.array_equal(got["cluster_hist"], z[f"graphs/{name}/cluster_hist{bins}"]), name


def case_cluster_landmarks(lib, dev):
    """The bins the issue names: c = 0.7 -> 69 (not 70), c = 0.35 -> 34, K65 -> 99, edgeless -> one count in bin 0, single edge -> two."""
    h = lambda name: cluster_run(lib, dev, name, 100)["cluster_hist"]
    # (the first 7 / 42 pairs among the hub's neighbours give two / three more nodes of the hub's degree and triangle count)
    assert h("c07")[0, 69] == 3 and h("c07")[0, 70] == 0 and cluster_run(lib, dev, "c07", 100)["tri2"][0, 0] == 14
    assert h("n17")[0, 34] == 4 and h("n17")[0, 35] == 0 and cluster_run(lib, dev, "n17", 100)["tri2"][0, 0] == 84
    assert h("k65")[0].tolist() == [0] * 99 + [65]
    s = h("small5")
    assert s[0].tolist() == [1] + [0] * 99 and s[1].tolist() == [2] + [0] * 99 and s[3].tolist() == [1] + [0] * 99
    assert s[2, 99] == 2 and s[2, 33] == 1 and s[2, 0] == 1                       # triangle + tail; its diagonal of ones is ignored
    n2 = h("n2")
    assert n2[:, 0].tolist() == [2, 1, 2] and n2[:, 1:].sum() == 0


def case_cluster_raw_and_null(lib, dev):
    """Raw (unquantised) samples pass through the same quantiser; tri2=False leaves the histogram unchanged; a NULL histogram leaves tri2
    unchanged; the degree histogram of finish() agrees with the reference's degree_worker on the same graphs."""
    import ctypes as C

    z, meta = e1()
    eng = sample_ops(lib, dev)
    adj = z["graphs/r65/adj"].astype(np.float32)
    rng = np.random.default_rng(65)
    raw = np.where(adj != 0, 0.5 + rng.random(adj.shape), 0.5 * rng.random(adj.shape)).astype(np.float32)
    raw = np.nextafter(np.minimum(raw, raw.transpose(0, 2, 1)), np.float32(0))     # symmetric; no-edge entries stay below 0.5
    raw[adj != 0] = np.maximum(raw[adj != 0], np.float32(0.5))
    want = cluster_run(lib, dev, "r65", 100)
    t = torch.from_numpy(raw).to(dev)
    got = eng.cluster_hist(t, bins=100)
    assert torch.equal(got["cluster_hist"].cpu(), torch.from_numpy(want["cluster_hist"]))
    only = eng.cluster_hist(t, bins=100, tri2=False)
    assert set(only) == {"cluster_hist"} and torch.equal(only["cluster_hist"], got["cluster_hist"])
    tri = torch.full((3, 65), -1, dtype=torch.int32, device=dev)
    edges = torch.from_numpy(np.linspace(0.0, 1.0, 101)).to(dev)
    lib.check(lib.ccsd_cluster_hist(C.c_void_p(t.data_ptr()), 3, 65, 0, 0.5, C.c_void_p(edges.data_ptr()), 100, C.c_void_p(tri.data_ptr()), None,
                                    eng._stream()))
    assert torch.equal(tri.cpu(), torch.from_numpy(want["tri2"]))
    for name in ("r65", "eval_pred", "small5"):
        d = ev.describe(torch.from_numpy(z[f"graphs/{name}/adj"]), device=dev, lib=lib)
        dh, ref, ln = d["degree_hist"].cpu().numpy(), z[f"graphs/{name}/degree_hist"], z[f"graphs/{name}/degree_len"]
        for b in range(dh.shape[0]):
            if dh[b, 1:].any():
                assert np.array_equal(dh[b, 1:], ref[b, 1:]) and ref[b, 0] == 0 and ln[b] == np.nonzero(dh[b])[0].max() + 1
            else:
                assert ref[b].tolist() == [1] + [0] * (dh.shape[1] - 1)


def case_bad_dims(lib, dev):
    eng = sample_ops(lib, dev)
    with pytest.raises(ValueError, match=r"N = 1 outside 2\.\.512"):
        eng.cluster_hist(torch.zeros(1, 1, 1, device=dev))
    with pytest.raises(ValueError, match=r"N = 513 outside 2\.\.512"):
        eng.cluster_hist(torch.zeros(1, 513, 513, device=dev))
    with pytest.raises(ValueError, match=r"bins = 0 outside"):
        eng.cluster_hist(torch.zeros(1, 4, 4, device=dev), bins=0)
    with pytest.raises(ValueError, match="must be"):
        eng.cluster_hist(torch.zeros(1, 4, 5, device=dev))
    ok = torch.ones(3, 5, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match=r"L = 0 must be >= 1"):
        eng.mmd(torch.ones(3, 0, dtype=torch.int32, device=dev), torch.ones(2, 0, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match=r"n1 = 0, n2 = 3"):
        eng.mmd(torch.ones(0, 5, dtype=torch.int32, device=dev), ok)
    with pytest.raises(ValueError, match="is_hist"):
        eng.mmd(ok, ok, "emd", is_hist=False)
    with pytest.raises(ValueError, match="sigma"):
        eng.mmd(ok, ok, "tv", sigma=0.0)
    with pytest.raises(ValueError, match="kind"):
        eng.mmd(ok, ok, "cosine")
    with pytest.raises(ValueError, match="int32 or both float64"):
        eng.mmd(ok.float(), ok.float())


# ---- MMD ----------------------------------------------------------------------------------------------------------------------------
def numpy_mmd(rows1, lens1, rows2, lens2, kind, is_hist=True, sigma=1.0, scale=1.0, degree=False, f32=False):
    """[disc11, disc22, disc12, mmd] in float64: compute_mmd of the reference with the closed-form EMD and pyemd's extra-mass rule."""
    def prep(rows, lens):
        r = np.array(rows, np.float64)
        lens = np.array(lens)
        if degree:
            r[:, 0] = 0.0
            empty = ~r.any(1)
            r[empty, 0] = 1.0
            lens = np.array([np.nonzero(x)[0].max() + 1 for x in r])
        s = r.sum(1)
        if is_hist:
            nz = s != 0
            if f32:
                r[nz] = (r[nz].astype(np.float32) / s[nz].astype(np.float32)[:, None]).astype(np.float64)
            else:
                r[nz] = r[nz] / s[nz][:, None]
        return r, (s != 0), lens

    (a, ma, la), (b, mb, lb) = prep(rows1, lens1), prep(rows2, lens2)

    def disc(x, mx, lx, y, my, ly):
        if kind == "emd":
            d = np.abs(np.cumsum(x, 1)[:, None, :] - np.cumsum(y, 1)[None, :, :]).sum(-1) / scale
            pen = (np.maximum(lx[:, None], ly[None, :]) - 1) / scale
            d = np.where(mx[:, None] != my[None, :], pen, np.where(mx[:, None], d, 0.0))
        elif kind == "tv":
            d = np.abs(x[:, None, :] - y[None, :, :]).sum(-1) / 2.0
        else:
            d = np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))
        return float(np.exp(-d * d / (2 * sigma * sigma)).mean())

    d11, d22, d12 = disc(a, ma, la, a, ma, la), disc(b, mb, lb, b, mb, lb), disc(a, ma, la, b, mb, lb)
    return np.array([d11, d22, d12, d11 + d22 - 2 * d12])


# (n1, n2, L, ragged rows, rows without mass): every n of {1, 3, 64, 65, 130} (one tile, one row past it, three tiles with a ragged
# last one) and every L of {1, 2, 33, 100, 200, 512} (below, at and past the 32-bin chunk of the pair kernel) occurs
MMD_SHAPES = {"n1_l1": (1, 1, 1, False, False), "n3_l2": (3, 1, 2, False, True), "n64_l33": (64, 65, 33, True, True),
              "n65_l100": (65, 130, 100, False, False), "n130_l200": (130, 3, 200, True, True), "n3_l512": (3, 64, 512, True, False),
              "n130_l33": (130, 130, 33, False, True)}
MMD_KINDS = [("emd", 1.0, 1.0), ("emd", 0.1, 100.0), ("tv", 1.0, 1.0), ("tv", 0.1, 100.0), ("l2", 1.0, 1.0), ("l2", 0.1, 100.0)]

_sets = {}


def mmd_set(name):
    if name not in _sets:
        n1, n2, L, ragged, zero = MMD_SHAPES[name]
        rng = np.random.default_rng(sum(map(ord, name)))

        def rows(n, side):
            r = rng.integers(0, 6, (n, L)).astype(np.int32)
            lens = rng.integers(1, L + 1, n).astype(np.int32) if ragged else np.full(n, L, np.int32)
            if ragged:
                lens[0] = L
            r[np.arange(L)[None, :] >= lens[:, None]] = 0
            r[~r.any(1), 0] = 1
            if zero:
                r[(1 if n > 1 else 0) if side == 0 else n - 1] = 0
                if side == 0 and n > 70:
                    r[70] = 0
            return r, lens
        _sets[name] = rows(n1, 0) + rows(n2, 1)
    return _sets[name]


def case_mmd_restatement(lib, dev, name):
    """All three kinds and the raw-vector call (gaussian, is_hist=False, sigma=30) against the float64 restatement, and two calls bit-equal."""
    r1, l1, r2, l2 = mmd_set(name)
    eng = sample_ops(lib, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    for kind, sigma, scale in MMD_KINDS:
        want = numpy_mmd(r1, l1, r2, l2, kind, True, sigma, scale)
        got = eng.mmd(t(r1), t(r2), kind, sigma=sigma, distance_scaling=scale, lens1=t(l1), lens2=t(l2))
        again = eng.mmd(t(r1), t(r2), kind, sigma=sigma, distance_scaling=scale, lens1=t(l1), lens2=t(l2))
        assert got.dtype == torch.float64 and torch.equal(got, again), (name, kind)
        err = np.abs(got.cpu().numpy() - want).max()
        print(f"mmd {name} {kind} sigma={sigma} scale={scale}: {got[3].item():.17g} restated {want[3]:.17g} max err {err:.3g}")
        assert err <= TOL, (name, kind, sigma, scale, err)
        # the list interface of compute_mmd (rows cut to their lengths) gives the same score
        if kind == "emd" and sigma == 1.0:
            s = ev.compute_mmd([r[:n] for r, n in zip(r1, l1)], [r[:n] for r, n in zip(r2, l2)], ev.gaussian_emd, device=dev, lib=lib)
            assert s == got[3].item(), (name, s, got[3].item())
    f1, f2 = r1.astype(np.float64) * 7.5, r2.astype(np.float64) * 7.5
    want = numpy_mmd(f1, l1, f2, l2, "l2", False, 30.0)
    got = eng.mmd(t(f1), t(f2), "l2", is_hist=False, sigma=30.0).cpu().numpy()
    assert np.abs(got - want).max() <= TOL, (name, "raw", np.abs(got - want).max())
    # degree convention: bin 0 cleared, an empty row becomes [1], lengths trimmed
    want = numpy_mmd(r1, l1, r2, l2, "emd", True, 1.0, 1.0, degree=True)
    got = eng.mmd(t(r1), t(r2), "emd", degree=True).cpu().numpy()
    assert np.abs(got - want).max() <= TOL, (name, "degree", np.abs(got - want).max())


def case_mmd_identical(lib, dev, name):
    """A set against itself: |mmd| <= 1e-12 (the two symmetric reductions and the full one add the same values in different orders)."""
    r1, l1, _, _ = mmd_set(name)
    t = torch.from_numpy(r1).to(dev)
    for kind in ("emd", "tv", "l2"):
        got = sample_ops(lib, dev).mmd(t, t, kind, sigma=0.1, distance_scaling=100.0, lens1=torch.from_numpy(l1).to(dev), lens2=torch.from_numpy(l1).to(dev))
        assert abs(got[3].item()) <= TOL and abs(got[0].item() - got[2].item()) <= TOL, (name, kind, got)


def mmd_fixture_sets():
    return sorted(e1()[1]["mmd_sets"])


def case_mmd_reference(lib, dev, name):
    """compute_mmd against the reference's own scores of the fixture's histogram sets."""
    z, meta = e1()
    rows = [[r[:n] for r, n in zip(z[f"mmd/{name}/rows{s}"], z[f"mmd/{name}/lens{s}"])] for s in "12"]
    sc = meta["scores"]
    kw = dict(device=dev, lib=lib)
    for sigma, scale in ((1.0, 1.0), (0.1, 100.0)):
        tag = f"mmd/{name}/s{sigma:g}_d{scale:g}"
        for k, sel in (("tv", ev.gaussian_tv), ("l2", ev.gaussian)):
            got = ev.compute_mmd(rows[0], rows[1], sel, sigma=sigma, **kw)
            print(f"{tag}/{k}: {got:.17g} reference {sc[tag + '/' + k]:.17g}")
            assert abs(got - sc[f"{tag}/{k}"]) <= TOL, (tag, k, got, sc[f"{tag}/{k}"])
        if meta["mmd_sets"][name]["emd"]:
            got = ev.compute_mmd(rows[0], rows[1], ev.gaussian_emd, sigma=sigma, distance_scaling=scale, **kw)
            tol = max(4 * meta["lp_vs_closed"][tag + "/emd"], TOL)
            print(f"{tag}/emd: {got:.17g} reference {sc[tag + '/emd']:.17g} tolerance {tol:.3g}")
            assert abs(got - sc[tag + "/emd"]) <= tol, (tag, got, sc[tag + "/emd"], tol)
    raw = [[r.astype(np.float64) * 7.5 for r in side] for side in rows]
    got = ev.compute_mmd(raw[0], raw[1], ev.gaussian, is_hist=False, sigma=30.0, **kw)
    assert abs(got - sc[f"mmd/{name}/raw_s30/l2"]) <= TOL, (name, got)


# ---- host layer ---------------------------------------------------------------------------------------------------------------------
def case_eval_torch_batch(lib, dev):
    """eval_torch_batch reproduces the reference's rounded dict; the unrounded scores are within the bounds above."""
    z, meta = e1()
    kw = dict(device=dev, lib=lib)
    ref, pred = (torch.from_numpy(z[f"graphs/{n}/adj"]) for n in ("eval_ref", "eval_pred"))
    assert ev.eval_torch_batch(ref, pred, **kw) == meta["eval_graph_list"]
    dr, dp = ev.describe(ref, **kw), ev.describe(pred, **kw)
    assert ev.eval_torch_batch(dr, dp, ["cluster", "degree"], **kw) == meta["eval_graph_list"]
    sc, lp = meta["scores"], meta["lp_vs_closed"]
    assert abs(ev.degree_stats(dr, dp, **kw) - sc["degree/emd"]) <= max(4 * lp["degree/emd"], TOL)
    assert abs(ev.clustering_stats(dr, dp, **kw) - sc["cluster/emd"]) <= max(4 * lp["cluster/emd"], TOL)
    assert abs(ev.clustering_stats(ref, pred, bins=10, **kw) - sc["cluster10/emd"]) <= max(4 * lp["cluster10/emd"], TOL)
    assert abs(ev.degree_stats(dr, dp, ev.gaussian_tv, **kw) - sc["degree/tv"]) <= TOL
    assert abs(ev.clustering_stats(dr, dp, ev.gaussian_tv, **kw) - sc["cluster/tv"]) <= TOL
    with pytest.raises(ValueError, match="10 bins"):
        ev.clustering_stats(ev.describe(ref, bins=10, **kw), dp, **kw)


def cc_descriptors(dev, side, extra_empty=0):
    """Descriptor dicts of the reference's samples in tests/golden/f1_finish.npz, as meta["cc_sets"] lists them."""
    z, meta = e1()
    f1 = load_golden("f1_finish.npz")
    out = {}
    for key, src in (("n_nodes", "n_nodes"), ("edge_hist", "edge_hist"), ("rank2_cell_hist", "cell_hist")):
        a = np.concatenate([f1[f"{n}/{c}/{src}"] for n, c in meta["cc_sets"][side]])
        a = np.concatenate([a, np.zeros((extra_empty,) + a.shape[1:], a.dtype)])
        out[key] = torch.from_numpy(a).to(dev)
    return out


def case_eval_cc_batch(lib, dev):
    """eval_CC_batch over the rank-2 (and rank-1) histograms of f1_finish.npz reproduces the reference's rounded dicts: as they are, with
    a complex without cells on each side (kept in the reference set -- a row without mass --, dropped from the predictions), and sliced."""
    z, meta = e1()
    kw = dict(device=dev, lib=lib)
    wk = meta["cc_worker_kwargs"]
    sc, lp = meta["scores"], meta["lp_vs_closed"]
    for tag, extra, nb in (("plain", 0, 1000), ("empties", 1, 1000), ("first5", 0, 5)):
        ref, pred = cc_descriptors(dev, "ref", extra), cc_descriptors(dev, "pred", extra)
        got = ev.eval_CC_batch(ref, pred, wk, cc_nb_eval=nb, **kw)
        assert got == meta[f"eval_CC_list/{tag}"], (tag, got, meta[f"eval_CC_list/{tag}"])
        for m, fn in (("rank1", ev.rank1_distrib_stats), ("rank2", ev.rank2_distrib_stats)):
            s = fn(ref, pred, wk, cc_nb_eval=nb, **kw)
            t = f"cc/{tag}/{m}/emd"
            print(f"{t}: {s:.17g} reference {sc[t]:.17g} recorded discrepancy {lp[t]:.3g}")
            assert abs(s - sc[t]) <= max(4 * lp[t], TOL), (t, s, sc[t])


def case_unsupported(lib, dev):
    z, _ = e1()
    adj = torch.from_numpy(z["graphs/eval_ref/adj"])
    kw = dict(device=dev, lib=lib)
    for m in ("orbit", "spectral", "nspdk"):
        with pytest.raises(NotImplementedError, match=m):
            ev.eval_torch_batch(adj, adj, ["degree", m], **kw)
    d = cc_descriptors(dev, "ref")
    for m in ("hodge_laplacian_spectrum", "rank0_distrib"):
        with pytest.raises(NotImplementedError, match=m):
            ev.eval_CC_batch(d, d, {"min_edge_val": 1, "max_edge_val": 3}, [m], **kw)
    with pytest.raises(TypeError):
        ev.gaussian_emd(np.ones(3), np.ones(3))
    with pytest.raises(TypeError):
        ev.compute_mmd([np.ones(3)], [np.ones(3)], lambda x, y: 0.0, **kw)
