"""Evaluation of finished samples on the GPU: the reference's MMD scores against a held-out set.

Mirrors, under the reference's names, the part of ccsd/src/evaluation/{mmd,stats}.py and ccsd/src/utils/cc_utils.py:1208-1474 that
needs no external program:

  compute_mmd with gaussian_emd / gaussian_tv / gaussian          (mmd.py:27-257)       -> SampleOps.mmd (ccsd_mmd)
  degree_stats, clustering_stats, eval_torch_batch                (stats.py:60-310, 547-570)
  rank1_distrib_stats, rank2_distrib_stats, eval_CC_batch         (cc_utils.py:1208-1474, eval_CC_list)
  spectral_stats                                                  (stats.py:125-203)    -> SampleOps.spectral_hist (ccsd_spectral_hist)
  hodge_laplacian_spectrum_stats                                  (cc_utils.py:994-1098) -> SampleOps.hodge_spectrum (ccsd_hodge_spectrum)
  orbit_stats_all                                                 (stats.py:343-435)    -> SampleOps.orbit_counts (ccsd_orbit_counts)
  nspdk_stats, compute_nspdk_mmd with eden.py's vectorize         (stats.py:438-467, mmd.py:309-377, eden.py)
                                                                                        -> SampleOps.nspdk_features / nspdk_mmd
  convert_graphs_to_CCs with path_based (path_length 3) / cycles  (cc_utils.py:816-880, 1644-1754) -> SampleOps.lift (ccsd_lift); opt-in:
                                                                  describe(lift=), eval_CC_batch(lift=), lift_settings
  gen_mol: construct_mol, correct_mol, the largest fragment       (utils/mol_utils.py:144-326)   -> SampleOps.mol_correct (ccsd_mol_correct)
                                                                  with MOL_TABLES; opt-in: Sampler.molecules, Sampler.evaluate(correct=True)

The reference builds networkx graphs / toponetx complexes on the host and solves one pyemd linear program per pair of histograms.
Here a sample set is a dict of per-sample integer DESCRIPTORS on the device -- `describe()`: the descriptor outputs of
SampleOps.finish plus `cluster_hist` -- and every score is one ccsd_mmd call on them (ccsd_amd/samples.py: the plan-free calls; no
network plan is built here).  The two spectral scores need an eigenvalue
solver (ccsd_eigvalsh, a batched Jacobi iteration on the device) and cost O(N^3) per sample where the others cost O(N^2): they are
opt-in, `spectra=True`.  The orbit score counts 4-node graphlets per graph on the device where the reference starts the orca program
once per graph; its cost grows with the triangles of a graph, so it is opt-in as well, `orbits=True`.  The NSPDK score -- the one
graph score the reference prints for molecule runs -- hashes neighbourhood pairs per graph on the device and is opt-in, `nspdk=True`;
it takes INTEGER node labels (mol_labels) where the reference labels atoms with symbol strings, whose Python hash differs from process
to process.  The reference scores molecules after valency correction and largest-fragment selection (gen_mol): SampleOps.mol_correct
does that on the device with the valence data of MOL_TABLES, Sampler.evaluate(correct=True) scores its result.  There is no CPU fallback:
methods that need an external program raise NotImplementedError (UNSUPPORTED); their histograms, computed elsewhere, can still be
scored through compute_mmd.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .samples import SampleOps


class KernelSelector:
    """Names one of the reference's kernels (mmd.py:69-131) for compute_mmd.  The kernel values are computed on the device inside
    ccsd_mmd, pair tile by pair tile; the selector itself computes nothing."""

    def __init__(self, name: str, kind: str):
        self.__name__, self.kind = name, kind

    def __repr__(self) -> str:
        return f"<kernel selector {self.__name__}>"

    def __call__(self, *a, **k):
        raise TypeError(f"{self.__name__} selects a kernel of compute_mmd; it is evaluated on the device, not called per pair")


gaussian_emd = KernelSelector("gaussian_emd", "emd")
gaussian_tv = KernelSelector("gaussian_tv", "tv")
gaussian = KernelSelector("gaussian", "l2")

UNSUPPORTED = {
    "orbit": "counts the 4-node graphlet orbits of every graph (evaluation/stats.py:343-435) and is opt-in: pass orbits=True",
    "spectral": "runs a symmetric eigenvalue solver per graph (evaluation/stats.py:125-137) and is opt-in: pass spectra=True",
    "hodge_laplacian_spectrum": "runs a symmetric eigenvalue solver per complex (cc_utils.py:994-1060) and is opt-in: pass spectra=True",
    "nspdk": "hashes the neighbourhood pairs of every graph (evaluation/eden.py, mmd.py:331-377) and is opt-in: pass nspdk=True",
    "rank0_distrib": "the node label it histograms is data-set specific (cc_utils.py:1098-1205)",
}

_sample_ops: dict = {}


def _ops(device=None, lib=None) -> SampleOps:
    """One SampleOps (it keeps the uploaded bin edges) per (device, library)."""
    device = torch.device(device if device is not None else "cuda")
    key = (str(device), id(lib))
    if key not in _sample_ops:
        _sample_ops[key] = SampleOps(device, lib)
    return _sample_ops[key]


def _as_rows(samples, device):
    """A sample set -> (rows (n, L) int32 / float64 tensor on `device`, lens (n,) numpy, the set's numpy dtype kind).  Accepts a 2-D array /
    tensor or a sequence of 1-D arrays / tensors of differing lengths (zero padded, as process_tensor does, mmd.py:380-395)."""
    if isinstance(samples, torch.Tensor) and samples.dim() == 2:
        f32 = samples.dtype == torch.float32
        t = samples if samples.dtype == torch.int32 else samples.to(torch.int32 if not samples.dtype.is_floating_point else torch.float64)
        if not samples.dtype.is_floating_point and samples.dtype != torch.int32 and samples.numel() and int(samples.abs().max()) >= 2 ** 31:
            raise ValueError("compute_mmd: integer histograms must fit int32")
        return t.to(device), np.full(t.shape[0], t.shape[1], np.int32), ("f32" if f32 else "f" if t.dtype == torch.float64 else "i")
    rows = [np.asarray(s.detach().cpu() if isinstance(s, torch.Tensor) else s) for s in samples]
    if any(r.ndim != 1 for r in rows):
        raise ValueError("compute_mmd: a sample set is a 2-D array or a sequence of 1-D arrays")
    n = len(rows)
    lens = np.array([len(r) for r in rows], np.int32)
    floating = any(r.dtype.kind == "f" for r in rows)
    f32 = n > 0 and all(r.dtype == np.float32 for r in rows)
    out = np.zeros((n, int(lens.max()) if n else 0), np.float64 if floating else np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    if not floating:
        if out.size and np.abs(out).max() >= 2 ** 31:
            raise ValueError("compute_mmd: integer histograms must fit int32")
        out = out.astype(np.int32)
    return torch.from_numpy(out).to(device), lens, ("f32" if f32 else "f" if floating else "i")


def _pad(t: torch.Tensor, L: int) -> torch.Tensor:
    return t if t.shape[1] == L else torch.nn.functional.pad(t, (0, L - t.shape[1]))


def mmd_terms(samples1, samples2, kernel: KernelSelector = gaussian_emd, is_hist: bool = True, sigma: float = 1.0,
              distance_scaling: float = 1.0, *, degree: bool = False, f32_pmf: Optional[bool] = None, device=None, lib=None) -> torch.Tensor:
    """[disc(1,1), disc(2,2), disc(1,2), mmd] as a float64 device tensor; nothing is synchronised.  f32_pmf=None: taken from the
    inputs (float32 histograms are normalised in float32 by numpy, so by compute_mmd of the reference)."""
    if not isinstance(kernel, KernelSelector):
        raise TypeError("compute_mmd: kernel must be gaussian_emd, gaussian_tv or gaussian of ccsd_amd.evaluation")
    eng = _ops(device, lib)
    s1, l1, k1 = _as_rows(samples1, eng.device)
    s2, l2, k2 = _as_rows(samples2, eng.device)
    if s1.dtype != s2.dtype:
        s1, s2 = s1.to(torch.float64), s2.to(torch.float64)
    L = max(s1.shape[1], s2.shape[1])
    s1, s2 = _pad(s1, L), _pad(s2, L)
    ragged = bool((l1 != L).any() or (l2 != L).any()) and not degree
    lens = [torch.from_numpy(l).to(eng.device) if ragged else None for l in (l1, l2)]
    if f32_pmf is None:
        f32_pmf = k1 == "f32" and k2 == "f32"
    return eng.mmd(s1, s2, kernel.kind, is_hist=is_hist, degree=degree, f32_pmf=bool(f32_pmf and is_hist), sigma=sigma,
                   distance_scaling=distance_scaling, lens1=lens[0], lens2=lens[1])


def compute_mmd(samples1, samples2, kernel: KernelSelector = gaussian_emd, is_hist: bool = True, sigma: float = 1.0,
                distance_scaling: float = 1.0, **kw) -> float:
    """compute_mmd of the reference (mmd.py:230-257).  samples1 / samples2: 2-D arrays or lists of 1-D arrays of differing lengths,
    numpy or torch, integer or floating point."""
    return float(mmd_terms(samples1, samples2, kernel, is_hist, sigma, distance_scaling, **kw)[3].item())


# ---------------------------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------------------------
def describe(adj: torch.Tensor, x: Optional[torch.Tensor] = None, rank2: Optional[torch.Tensor] = None, *, mol: bool = False,
             thr: float = 0.5, bins: int = 100, d_min: int = 0, d_max: int = 0, spectra: bool = False, orbits: bool = False,
             nspdk: bool = False, nspdk_labels: Optional[torch.Tensor] = None, lift: Optional[dict] = None, device=None,
             lib=None) -> Dict[str, torch.Tensor]:
    """The descriptor dict of a batch: SampleOps.finish's descriptors (degree, degree_hist, edge_hist; n_nodes, x_hist with x;
    rank2_cell_bits / _count / _hist, rank2_nnz with rank2) plus cluster_hist (B, bins) and tri2 (B, N).  adj: (B, N, N), raw samples,
    quantised samples or a 0/1 data set (any real or integer dtype).  spectra=True adds spectral_hist (B, 200) int32 and, with rank2,
    hodge_spectrum (B, E) float32 (SampleOps.spectral_hist / hodge_spectrum: an eigenvalue solve per sample).  orbits=True adds
    orbit_counts (B, 15) int64 and orbit_nodes (B,) int32 (SampleOps.orbit_counts).  nspdk=True adds the NSPDK feature rows
    nspdk_indptr, nspdk_indices, nspdk_values (SampleOps.nspdk_features, N <= 64) with the node labels nspdk_labels (B, N), or
    mol_labels(x) when `mol` and x is given, or label 0 in every slot.  lift=dict(procedure=..., d_min=..., d_max=..., and optionally
    path_length, sources: the keywords of SampleOps.lift; lift_settings reads them from a config) without rank2 LIFTS the graphs to
    complexes (N <= 64): it adds rank2_cell_bits / _count / _hist, rank2_nnz and lift_dropped, and with spectra=True hodge_spectrum from
    them.  The cycles rule is networkx's cycle basis of the adjacency, not the reference's set-order-dependent one (SampleOps.lift)."""
    if lift is not None and rank2 is not None:
        raise ValueError("describe: lift= builds the rank-2 cells of a graph; a batch that brings its own rank2 is not lifted")
    eng = _ops(device if device is not None else (adj.device if adj.device.type == "cuda" else None), lib)
    mv = lambda t: None if t is None else t.to(device=eng.device, dtype=torch.float32).contiguous()
    adj, x, rank2 = mv(adj), mv(x), mv(rank2)
    out = eng.finish(x, adj, rank2, None, mol=mol, thr=thr, d_min=d_min, d_max=d_max, dense_rank2=False, dense_adj=False)
    out.update(eng.cluster_hist(adj, mol=mol, thr=thr, bins=bins))
    if lift is not None:
        out.update(eng.lift(adj, mol=mol, thr=thr, **lift))
        d_min, d_max = int(lift["d_min"]), int(lift["d_max"])
    if orbits:
        out.update(eng.orbit_counts(adj, mol=mol, thr=thr))
    if nspdk:
        if nspdk_labels is None and mol and x is not None:
            nspdk_labels = mol_labels(x)
        out.update(eng.nspdk_features(adj, None if nspdk_labels is None else torch.as_tensor(nspdk_labels).to(eng.device), mol=mol, thr=thr))
    if spectra:
        out.update(eng.spectral_hist(adj, mol=mol, thr=thr))
        if rank2 is not None or lift is not None:
            out["hodge_spectrum"] = eng.hodge_spectrum(adj, out["rank2_cell_bits"], d_min=d_min, d_max=d_max, mol=mol, thr=thr)
    return out


def lift_settings(data_cfg, N: Optional[int] = None) -> Optional[dict]:
    """The lifting rule of a config's `data` section as keywords of SampleOps.lift (procedure, and for path_based path_length and
    sources), read as convert_graphs_to_CCs reads lifting_procedure / lifting_procedure_kwargs (cc_utils.py:851-878); None when the
    config names no procedure.  "basic" means every one of the N = max_node_num node slots is a source and path_length 3; a dict
    passes sources_nodes / path_length through, its sources at or past N dropped (they are no node of any graph of the batch).  A string other than "basic", a string for cycles and an unknown procedure raise
    NotImplementedError with the reference's message."""
    get = lambda k: data_cfg.get(k) if isinstance(data_cfg, dict) else getattr(data_cfg, k, None)
    proc, kwargs = get("lifting_procedure"), get("lifting_procedure_kwargs")
    if proc is None:
        return None
    if kwargs is None:
        kwargs = {}
    if proc == "path_based":
        if isinstance(kwargs, str):
            if kwargs != "basic":
                raise NotImplementedError(f"Lifting procedure kwargs {kwargs} not implemented")
            kwargs = {"sources_nodes": None, "path_length": 3}        # (range(max_node_num): every slot, which SampleOps.lift spells None)
        src = kwargs.get("sources_nodes")
        return {"procedure": "path_based", "path_length": int(kwargs.get("path_length", 3)), "sources": None if src is None else [int(n) for n in src if N is None or int(n) < N]}
    if proc == "cycles":
        if isinstance(kwargs, str):
            raise NotImplementedError(f"Lifting procedure kwargs {kwargs} not implemented")
        return {"procedure": "cycles"}
    raise NotImplementedError(f"Lifting procedure {proc} not implemented")


def _descriptors(obj, need: Sequence[str], **kw) -> Dict[str, torch.Tensor]:
    if isinstance(obj, dict):
        missing = [k for k in need if k not in obj]
        if missing:
            raise KeyError(f"descriptor dict lacks {missing}; describe() produces them")
        return obj
    return describe(torch.as_tensor(obj), **kw)


def _dev_kw(kw):
    return {k: kw[k] for k in ("device", "lib") if k in kw}


def degree_stats(ref, pred, kernel: KernelSelector = gaussian_emd, **kw) -> float:
    """degree_stats (stats.py:60-122): MMD of the degree histograms.  ref / pred: adjacency batches or descriptor dicts.  The graphs
    of adjs_to_graphs hold no isolated node and at least one node, so no predicted graph is ever dropped as empty."""
    a, b = _descriptors(ref, ["degree_hist"], **kw), _descriptors(pred, ["degree_hist"], **kw)
    return compute_mmd(a["degree_hist"], b["degree_hist"], kernel, degree=True, **_dev_kw(kw))


def clustering_stats(ref, pred, kernel: KernelSelector = gaussian_emd, bins: int = 100, **kw) -> float:
    """clustering_stats (stats.py:223-310): sigma = 0.1 and, for the kernel that takes it, distance_scaling = bins."""
    a, b = _descriptors(ref, ["cluster_hist"], bins=bins, **kw), _descriptors(pred, ["cluster_hist"], bins=bins, **kw)
    for d in (a, b):
        if d["cluster_hist"].shape[1] != bins:
            raise ValueError(f"clustering_stats: cluster_hist has {d['cluster_hist'].shape[1]} bins, not {bins}")
    return compute_mmd(a["cluster_hist"], b["cluster_hist"], kernel, sigma=1.0 / 10,
                       distance_scaling=bins if kernel is gaussian_emd else 1.0, **_dev_kw(kw))


SPECTRAL_BINS = 200          # spectral_worker's np.histogram(eigs, bins=200, range=(-1e-5, 2)) (stats.py:135)


def _spectral_rows(obj, kw) -> torch.Tensor:
    """spectral_hist of a side: taken from a descriptor dict that has it, computed from its `adj` (or from a raw batch) otherwise."""
    if isinstance(obj, dict) and "spectral_hist" in obj:
        return obj["spectral_hist"]
    if isinstance(obj, dict) and "adj" not in obj:
        raise KeyError("descriptor dict lacks spectral_hist and the adj to compute it from; describe(..., spectra=True) produces it")
    adj = obj["adj"] if isinstance(obj, dict) else torch.as_tensor(obj)
    eng = _ops(kw.get("device") if kw.get("device") is not None else (adj.device if adj.device.type == "cuda" else None), kw.get("lib"))
    adj = adj.to(device=eng.device, dtype=torch.float32).contiguous()
    return eng.spectral_hist(adj, mol=kw.get("mol", False), thr=kw.get("thr", 0.5))["spectral_hist"]


def spectral_stats(ref, pred, kernel: KernelSelector = gaussian_emd, **kw) -> float:
    """spectral_stats (stats.py:140-203): MMD of the 200-bin histograms of the normalised Laplacian's eigenvalues, sigma = 1 and no
    distance scaling.  ref / pred: adjacency batches or descriptor dicts (spectral_hist, or adj to compute it from).  The graphs of
    adjs_to_graphs hold at least one node, so no predicted graph is dropped.  Eigenvalues are clamped to [0, 2] before binning
    (SampleOps.spectral_hist): the one deliberate difference from the reference."""
    a, b = _spectral_rows(ref, kw), _spectral_rows(pred, kw)
    for h in (a, b):
        if h.shape[1] != SPECTRAL_BINS:
            raise ValueError(f"spectral_stats: spectral_hist has {h.shape[1]} bins, not {SPECTRAL_BINS}")
    return compute_mmd(a, b, kernel, **_dev_kw(kw))


def orbit_rows(obj, kw) -> torch.Tensor:
    """The rows orbit_stats_all scores, (B, 15) float64: a graph's orbit counts divided by its node count -- the IEEE division the
    reference performs on its int64 sums (stats.py:414).  Taken from a descriptor dict that holds orbit_counts and orbit_nodes,
    computed from its `adj` (or from a raw batch) otherwise."""
    if not (isinstance(obj, dict) and "orbit_counts" in obj and "orbit_nodes" in obj):
        if isinstance(obj, dict) and "adj" not in obj:
            raise KeyError("descriptor dict lacks orbit_counts / orbit_nodes and the adj to compute them from; describe(..., orbits=True) produces them")
        adj = obj["adj"] if isinstance(obj, dict) else torch.as_tensor(obj)
        eng = _ops(kw.get("device") if kw.get("device") is not None else (adj.device if adj.device.type == "cuda" else None), kw.get("lib"))
        adj = adj.to(device=eng.device, dtype=torch.float32).contiguous()
        obj = eng.orbit_counts(adj, mol=kw.get("mol", False), thr=kw.get("thr", 0.5))
    return obj["orbit_counts"].double() / obj["orbit_nodes"].double()[:, None]


def orbit_stats_all(ref, pred, kernel: KernelSelector = gaussian, **kw) -> float:
    """orbit_stats_all (stats.py:382-435): MMD of the per-graph orbit counts over the node count, raw vectors (is_hist=False) with
    sigma = 30.  ref / pred: adjacency batches or descriptor dicts (orbit_counts and orbit_nodes, or adj to compute them from).
    gaussian_emd has no meaning on raw vectors: ccsd_mmd refuses it."""
    a, b = orbit_rows(ref, kw), orbit_rows(pred, kw)
    return compute_mmd(a, b, kernel, is_hist=False, sigma=30.0, **_dev_kw(kw))


NSPDK_KEYS = ("nspdk_indptr", "nspdk_indices", "nspdk_values")


def mol_labels(x) -> torch.Tensor:
    """Integer node labels of a molecule batch from its raw or one-hot node features x (B, N, F): the index of the first channel
    above 0.5, or -1 where there is none (the "no atom" column of x_onehot, sampler.py:1222-1224) -- such a slot holds no node."""
    x = torch.as_tensor(x)
    on = x > 0.5
    first = on.to(torch.int8).argmax(-1)
    return torch.where(on.any(-1), first, torch.full_like(first, -1)).to(torch.int32)


def _mol_table(atomic_num_list):
    # element -> (largest permitted valence when neutral, with charge +1, the reference's ATOM_VALENCY entry if it may take the charge)
    elements = {6: (4, 4, 0), 7: (3, 4, 3), 8: (2, 3, 2), 9: (1, 1, 0), 15: (7, 7, 0), 16: (6, 6, 2), 17: (1, 1, 0), 35: (1, 1, 0), 53: (5, 5, 0)}
    return {"atomic_num_list": list(atomic_num_list), "max_valence": [list(elements[z][:2]) for z in atomic_num_list],
            "charge_base": [elements[z][2] for z in atomic_num_list]}


MOL_TABLES = {"QM9": _mol_table([6, 7, 8, 9]), "ZINC250k": _mol_table([6, 7, 8, 9, 15, 16, 17, 35, 53])}
"""The valence data of SampleOps.mol_correct per molecule data set -- the one place it lives.  A row per node label, in the order of the
reference's atomic_num_list (gen_mol, utils/mol_utils.py:212-215; the label is mol_labels' channel index):
  atomic_num_list   QM9 [6, 7, 8, 9] = C N O F; ZINC250k [6, 7, 8, 9, 15, 16, 17, 35, 53] = C N O F P S Cl Br I
  max_valence       [neutral, charge +1]: the bond-order sum above which rdkit's SanitizeMol(SANITIZE_PROPERTIES) refuses the atom, i.e. the
                    largest entry of rdkit's permitted-valence list.  Neutral: C 4, N 3, O 2, F 1, P 7, S 6, Cl 1, Br 1, I 5.  With
                    charge +1 rdkit takes the list of the isoelectronic element: N 4, O 3.  Only N and O are ever charged with these
                    tables (S at 3 is not over-valent, so construct_mol never charges it); the other labels repeat their neutral entry,
                    which is never read.
  charge_base       the reference's ATOM_VALENCY entry (mol_utils.py:24) of the labels construct_mol may charge (mol_utils.py:186): N 3,
                    O 2, S 2; 0 for every other label.
rdkit is not installed where this project is built and tested, so NOBODY HAS CHECKED THESE MAXIMA AGAINST RDKIT: they are restated from
rdkit's element table.  That is why they are data and an argument of mol_correct (max_valence=, charge_base=), not constants of the
kernel."""


def nspdk_rows(obj, kw) -> Dict[str, torch.Tensor]:
    """The NSPDK feature rows of a side (CSR: NSPDK_KEYS): taken from a dict that holds them, computed from its `adj` with the labels
    `nspdk_labels`, or mol_labels(x) of its `x` in mol mode, or label 0 (a raw batch has label 0 in every slot)."""
    if isinstance(obj, dict) and all(k in obj for k in NSPDK_KEYS):
        return obj
    if isinstance(obj, dict) and "adj" not in obj:
        raise KeyError("descriptor dict lacks nspdk_indptr / nspdk_indices / nspdk_values and the adj to compute them from; describe(..., nspdk=True) produces them")
    adj = obj["adj"] if isinstance(obj, dict) else torch.as_tensor(obj)
    eng = _ops(kw.get("device") if kw.get("device") is not None else (adj.device if adj.device.type == "cuda" else None), kw.get("lib"))
    adj = adj.to(device=eng.device, dtype=torch.float32).contiguous()
    labels = None
    if isinstance(obj, dict):
        labels = obj.get("nspdk_labels")
        if labels is None and kw.get("mol", False) and obj.get("x") is not None:
            labels = mol_labels(obj["x"])
    return eng.nspdk_features(adj, None if labels is None else torch.as_tensor(labels).to(eng.device), mol=kw.get("mol", False), thr=kw.get("thr", 0.5))


def nspdk_stats(ref, pred, **kw) -> float:
    """nspdk_stats (stats.py:438-467): the MMD of the two sets' NSPDK feature rows under the linear kernel -- it takes no kernel
    argument.  ref / pred: adjacency batches (label 0 in every slot) or dicts (the three nspdk_* keys, or adj plus nspdk_labels or x).
    Predicted graphs without a node are left out, as in the reference.  The score is of the sets as given, with integer labels: for
    molecules the reference corrects the predicted set first (SampleOps.mol_correct; see the module docstring)."""
    a, b = nspdk_rows(ref, kw), nspdk_rows(pred, kw)
    eng = _ops(kw.get("device") if kw.get("device") is not None else (a["nspdk_indptr"].device if a["nspdk_indptr"].device.type == "cuda" else None), kw.get("lib"))
    return float(eng.nspdk_mmd(a, b)[3].item())


def _cc_keep(desc: Dict[str, torch.Tensor], n: Optional[int], drop_empty: bool) -> torch.Tensor:
    """Row indices eval_CC_list scores: the first n complexes (cc_nb_eval slices first), minus -- predictions only -- the complexes
    with no node, edge or cell (is_empty_cc, cc_utils.py:982-991)."""
    cells = desc["edge_hist"][:, 1:].sum(-1)
    if "n_nodes" in desc:
        cells = cells + desc["n_nodes"]
    if "rank2_cell_hist" in desc:
        cells = cells + desc["rank2_cell_hist"].sum(-1)
    idx = torch.arange(cells.shape[0], device=cells.device)[:n]
    return idx[cells[:n] > 0] if drop_empty else idx


def rank1_distrib_stats(ref_desc, pred_desc, worker_kwargs, kernel: KernelSelector = gaussian_emd, cc_nb_eval: Optional[int] = None, **kw) -> float:
    """rank1_distrib_stats (cc_utils.py:1235-1312): histogram of the rank-1 cells' integer values over min_edge_val..max_edge_val,
    from edge_hist (pairs by quantised value; value 0 is no cell and never counts)."""
    lo, hi = int(worker_kwargs["min_edge_val"]), int(worker_kwargs["max_edge_val"])
    sets = []
    for desc, drop in ((ref_desc, False), (pred_desc, True)):
        eh = desc["edge_hist"].index_select(0, _cc_keep(desc, cc_nb_eval, drop))
        h = torch.zeros((eh.shape[0], hi - lo + 1), dtype=torch.int32, device=eh.device)
        for v in range(max(lo, 1), min(hi, eh.shape[1] - 1) + 1):
            h[:, v - lo] = eh[:, v]
        sets.append(h)
    return compute_mmd(sets[0], sets[1], kernel, f32_pmf=True, **_dev_kw(kw))        # (the worker's histograms are float32)


def rank2_distrib_stats(ref_desc, pred_desc, worker_kwargs=None, kernel: KernelSelector = gaussian_emd, cc_nb_eval: Optional[int] = None, **kw) -> float:
    """rank2_distrib_stats (cc_utils.py:1337-1406): histogram of the rank-2 cells by size d_min..d_max = rank2_cell_hist."""
    sets = [desc["rank2_cell_hist"].index_select(0, _cc_keep(desc, cc_nb_eval, drop)) for desc, drop in ((ref_desc, False), (pred_desc, True))]
    if worker_kwargs is not None and "d_min" in worker_kwargs:
        nb = int(worker_kwargs["d_max"]) - int(worker_kwargs["d_min"]) + 1
        if any(s.shape[1] != nb for s in sets):
            raise ValueError(f"rank2_distrib_stats: rank2_cell_hist does not have d_max - d_min + 1 = {nb} bins")
    return compute_mmd(sets[0], sets[1], kernel, f32_pmf=True, **_dev_kw(kw))        # (the worker's histograms are float32)


def _hodge_rows(desc, worker_kwargs, kw) -> torch.Tensor:
    """hodge_spectrum of a descriptor dict: taken from it, or computed from its `adj` and `rank2_cell_bits` (the cell sizes
    d_min..d_max come from worker_kwargs, as in the reference)."""
    if "hodge_spectrum" in desc:
        return desc["hodge_spectrum"]
    missing = [k for k in ("adj", "rank2_cell_bits") if k not in desc]
    if missing:
        raise KeyError(f"descriptor dict lacks hodge_spectrum and {missing} to compute it from; describe(..., spectra=True) produces it")
    adj = desc["adj"]
    eng = _ops(kw.get("device") if kw.get("device") is not None else (adj.device if adj.device.type == "cuda" else None), kw.get("lib"))
    adj = adj.to(device=eng.device, dtype=torch.float32).contiguous()
    if "N" in worker_kwargs and int(worker_kwargs["N"]) != adj.shape[1]:
        raise ValueError(f"hodge_laplacian_spectrum_stats: worker_kwargs N = {worker_kwargs['N']} but adj has {adj.shape[1]} nodes")
    return eng.hodge_spectrum(adj, desc["rank2_cell_bits"].to(eng.device), d_min=int(worker_kwargs["d_min"]), d_max=int(worker_kwargs["d_max"]),
                              mol=kw.get("mol", False), thr=kw.get("thr", 0.5))


def hodge_laplacian_spectrum_stats(ref_desc, pred_desc, worker_kwargs, kernel: KernelSelector = gaussian_emd,
                                   cc_nb_eval: Optional[int] = None, **kw) -> float:
    """hodge_laplacian_spectrum_stats (cc_utils.py:1025-1098): MMD of the float32 eigenvalue vectors of F F^T (length E; zeros for a
    complex without rank-2 cells), each normalised by its sum like a histogram (compute_mmd's is_hist default).  The descriptor dicts
    hold hodge_spectrum, or adj and rank2_cell_bits to compute it from (worker_kwargs: d_min, d_max)."""
    sets = [_hodge_rows(desc, worker_kwargs, kw).index_select(0, _cc_keep(desc, cc_nb_eval, drop))
            for desc, drop in ((ref_desc, False), (pred_desc, True))]
    return compute_mmd(sets[0], sets[1], kernel, **_dev_kw(kw))                      # (float32 rows: the f32_pmf path)


METHOD_NAME_TO_FUNC = {"degree": degree_stats, "cluster": clustering_stats}
CC_METHOD_NAME_TO_FUNC = {"rank1_distrib": rank1_distrib_stats, "rank2_distrib": rank2_distrib_stats}
# the methods that run the eigenvalue solver: accepted only with spectra=True
SPECTRA_METHOD_NAME_TO_FUNC = {"spectral": spectral_stats}
SPECTRA_CC_METHOD_NAME_TO_FUNC = {"hodge_laplacian_spectrum": hodge_laplacian_spectrum_stats}
# the method that counts graphlet orbits: accepted only with orbits=True
ORBIT_METHOD_NAME_TO_FUNC = {"orbit": orbit_stats_all}
# the method that hashes neighbourhood pairs: accepted only with nspdk=True, never a default, and without a kernel argument
NSPDK_METHOD_NAME_TO_FUNC = {"nspdk": nspdk_stats}
# the kernel a method gets when `kernels` does not name one: load_eval_settings' choice for "orbit" (utils/loader.py:660-684)
DEFAULT_KERNEL = {"orbit": gaussian}


def _check_methods(methods, table, spectra=False):
    for m in methods:
        if m in table:
            continue
        opted_in = spectra and (m in SPECTRA_METHOD_NAME_TO_FUNC or m in SPECTRA_CC_METHOD_NAME_TO_FUNC)      # (the other evaluator's method)
        if m in UNSUPPORTED and not opted_in:
            raise NotImplementedError(f"evaluation method {m!r}: {UNSUPPORTED[m]}")
        raise KeyError(f"unknown evaluation method {m!r}; available: {sorted(table)}")


def eval_torch_batch(ref_batch, pred_batch, methods: Optional[Sequence[str]] = None, kernels: Optional[dict] = None, *,
                     mol: bool = False, thr: float = 0.5, bins: int = 100, spectra: bool = False, orbits: bool = False,
                     nspdk: bool = False, **kw) -> Dict[str, float]:
    """eval_torch_batch / eval_graph_list (stats.py:480-570): {method: round(score, 6)}.  ref_batch / pred_batch: adjacency batches
    (B, N, N) or descriptor dicts.  Default methods: "degree", "cluster"; default kernel: gaussian_emd for both.
    orbits=True also accepts "orbit" (default kernel: gaussian, as load_eval_settings sets it) and, with methods=None, scores the
    reference's own default list "degree", "cluster", "orbit"; the counts of a side that does not hold them are computed from its
    adjacency.  spectra=True also accepts "spectral" and computes spectral_hist for a side given as a raw batch; with methods=None
    it is appended when orbits=True as well, which gives load_eval_settings' list "degree", "cluster", "orbit", "spectral", and is
    left out otherwise.  nspdk=True also accepts "nspdk" in `methods` (it is never a default; nspdk_stats: the linear-kernel MMD of
    the NSPDK feature rows, no kernel argument; like the reference's, its result is not rounded).  Without its keyword each of the
    three names raises NotImplementedError."""
    if methods is None:
        methods = ["degree", "cluster"] + (["orbit"] + (["spectral"] if spectra else []) if orbits else [])
    methods = list(methods)
    table = dict(METHOD_NAME_TO_FUNC, **(SPECTRA_METHOD_NAME_TO_FUNC if spectra else {}), **(ORBIT_METHOD_NAME_TO_FUNC if orbits else {}),
                 **(NSPDK_METHOD_NAME_TO_FUNC if nspdk else {}))
    _check_methods(methods, table, spectra)
    kernels = kernels or {}
    want_spec = "spectral" in methods
    dkw = dict(mol=mol, thr=thr, bins=bins, **_dev_kw(kw))
    # what a dict side must hold: the histograms of the methods asked for (orbit counts and NSPDK rows may be computed from its adj)
    need = (["degree_hist"] if "degree" in methods else []) + (["cluster_hist"] if "cluster" in methods else []) + (["spectral_hist"] if want_spec else [])
    sides = []
    for obj in (ref_batch, pred_batch):
        if isinstance(obj, dict) and want_spec and "spectral_hist" not in obj and "adj" in obj:
            obj = dict(obj, spectral_hist=_spectral_rows(obj, dict(mol=mol, thr=thr, **_dev_kw(kw))))
        # (a raw batch is described once, with everything the methods read; a dict side that lacks the orbit counts has them computed
        # from its adj inside orbit_stats_all; likewise the NSPDK rows -- a raw batch has label 0 in every slot)
        sides.append(_descriptors(obj, need, **dkw, **({"spectra": True} if want_spec else {}), **({"orbits": True} if "orbit" in methods else {}),
                                  **({"nspdk": True} if "nspdk" in methods else {})))
    ref, pred = sides
    out = {}
    for m in methods:
        if m == "nspdk":
            out[m] = nspdk_stats(ref, pred, mol=mol, thr=thr, **_dev_kw(kw))
            continue
        extra = {"bins": bins} if m == "cluster" else dict(mol=mol, thr=thr) if m == "orbit" else {}
        out[m] = round(table[m](ref, pred, kernels.get(m, DEFAULT_KERNEL.get(m, gaussian_emd)), **extra, **_dev_kw(kw)), 6)
    return out


def eval_CC_batch(ref_desc, pred_desc, worker_kwargs, methods: Optional[Sequence[str]] = None, kernels: Optional[dict] = None,
                  cc_nb_eval: Optional[int] = 1000, *, spectra: bool = False, mol: bool = False, thr: float = 0.5, lift: Optional[dict] = None,
                  **kw) -> Dict[str, float]:
    """eval_CC_list (cc_utils.py:1418-1474) on descriptor dicts: {method: round(score, 6)}.  Default methods: "rank1_distrib",
    "rank2_distrib" (the reference's other two defaults raise NotImplementedError when asked for, see UNSUPPORTED).
    spectra=True also accepts "hodge_laplacian_spectrum" in `methods` (it is never a default): a side without hodge_spectrum has it
    computed from its adj and rank2_cell_bits with the quantiser `mol`, `thr` and worker_kwargs' d_min, d_max.  Without spectra=True
    the name raises NotImplementedError.  lift=dict(procedure=..., d_min=..., d_max=..., ...) (describe's keyword) lifts a side that
    holds `adj` and edge_hist but no rank2_cell_hist -- a set of graphs -- to complexes first; the dicts passed in are not written to."""
    if lift is not None:
        sides = []
        for desc in (ref_desc, pred_desc):
            if "rank2_cell_hist" not in desc:
                if "adj" not in desc:
                    raise KeyError("eval_CC_batch: lift= needs adj on a side without rank2_cell_hist")
                adj = desc["adj"]
                eng = _ops(kw.get("device") if kw.get("device") is not None else (adj.device if adj.device.type == "cuda" else None), kw.get("lib"))
                desc = dict(desc, **eng.lift(adj.to(device=eng.device, dtype=torch.float32), mol=mol, thr=thr, **lift))
            sides.append(desc)
        ref_desc, pred_desc = sides
    methods = ["rank1_distrib", "rank2_distrib"] if methods is None else list(methods)
    table = dict(CC_METHOD_NAME_TO_FUNC, **SPECTRA_CC_METHOD_NAME_TO_FUNC) if spectra else CC_METHOD_NAME_TO_FUNC
    _check_methods(methods, table, spectra)
    kernels = kernels or {}
    out = {}
    for m in methods:
        extra = dict(mol=mol, thr=thr) if m in SPECTRA_CC_METHOD_NAME_TO_FUNC else {}
        out[m] = round(table[m](ref_desc, pred_desc, worker_kwargs, kernels.get(m, gaussian_emd), cc_nb_eval=cc_nb_eval, **extra,
                                **_dev_kw(kw)), 6)
    return out
