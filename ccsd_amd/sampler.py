"""Sampler harness: the reference's Sampler_{Graph,CC,mol_Graph,mol_CC}.sample() up to quantisation.

Mirrors ccsd/src/sampler.py:92-1235 for the part that is on, or directly around, the reverse-SDE path:

  load_ckpt -> load_seed(config.seed) -> load_model_from_ckpt x3 (EMA weights if sample.use_ema)
  -> load_sampling_fn(configt, config.sampler, config.sample, device, is_cc, d_min, d_max, divide_batch)
  -> load_seed(config.sample.seed) -> [init_flags -> sampling_fn] x divide_batch (x sampling rounds for the generic
  datasets) -> torch.cat -> quantize / quantize_mol (+ the molecule relabelling and one-hot of sampler.py:1216-1225)

What follows in the reference -- rdkit molecule construction, toponetx complexes, MMD / NSPDK / FCD metrics, pickles,
plots, wandb -- is out of scope; `sample()` returns the tensors those steps consume and, when
`save=True`, writes them to <folder>/samples/<log name>.npz.

init_flags (cc_utils.py:883-914): the reference draws `np.random.randint(0, len(train_list), batch)` and takes the node
flags of those training objects.  Only the node COUNT of each training object matters, so this build ships the counts
(ccsd_amd/data/node_counts.json: per-graph node counts of the pickled datasets in file order -> the same indices pick
the same flags for the same numpy seed).  QM9 / ZINC250k: the reference draws from its training molecules (sampler.py:1162-1194),
whose files the reference repository does not ship (.MISSING_LARGE_BLOBS).  When the user's dataset copy is present under
<folder>/data (<dataset>_kekulized.npz or <dataset>.csv, with valid_idx_<dataset>.json) the node counts of the training molecules
are read from it in the reference's order (mol_train_node_counts: same indices, same flags for the same numpy seed); otherwise
the flags come from a shipped histogram -- QM9: the node counts of the shipped test graphs (data/qm9_test_nx.pkl), ZINC250k: a
discretised normal fit of the dataset's published heavy-atom statistics (node_counts.json notes) -- and the run says so.
Generic datasets without shipped counts (ENZYMES, grid): the training graphs of the user's <folder>/<data.dir>/<data>.pkl, the file
the reference loads (graph_train_node_counts, reference order; its test split sets the number of sampling rounds); without it,
sample(node_counts=...) supplies them.
"""
from __future__ import annotations

import json
import math
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import loader
from .samples import SampleOps
from .loader import AttrDict, _get

_COUNTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "node_counts.json")


def _dataset_key(name: str) -> str:
    return name[:-3] if name.endswith("_CC") else name


def train_node_counts(configt, with_test_size: bool = False):
    """Node counts of the training split, in the order the reference's load_data(get_list=True) returns it
    (and, on request, the size of the test split, which sets the number of sampling rounds)."""
    with open(_COUNTS) as f:
        table = json.load(f)
    data = _get(configt, "data")
    entry = table.get(_dataset_key(_get(data, "data")))
    if entry is None or "node_counts" not in entry:
        return (None, 0) if with_test_size else None
    counts = np.asarray(entry["node_counts"], dtype=np.int64)
    test_size = int(_get(data, "test_split", 0.2) * len(counts))          # data_loader.py:80-81, 109-110
    return (counts[test_size:], test_size) if with_test_size else counts[test_size:]


def init_flags(obj_counts, config, batch_size: Optional[int] = None, is_cc: bool = False) -> torch.Tensor:
    """cc_utils.py:883-914 on node counts: flags[b, :n_b] = 1 with n_b the node count of a uniformly drawn training
    object (np.random.randint on the global numpy stream, like the reference).  `obj_counts` may also be a
    {node count: frequency} histogram (QM9 / ZINC250k, see the module docstring)."""
    data = _get(config, "data")
    if batch_size is None:
        batch_size = _get(data, "batch_size")
    N = _get(data, "max_node_num")
    if isinstance(obj_counts, dict):
        ks = np.array([int(k) for k in obj_counts], dtype=np.int64)
        p = np.array([float(v) for v in obj_counts.values()], dtype=np.float64)
        counts = np.random.choice(ks, size=batch_size, p=p / p.sum())
    else:
        counts = np.asarray(obj_counts, dtype=np.int64)
        counts = counts[np.random.randint(0, len(counts), batch_size)]
    flags = torch.zeros(batch_size, N)
    for b, c in enumerate(counts):
        flags[b, : int(min(c, N))] = 1.0
    return flags


_TWO_LETTER = ("Cl", "Br", "Si", "Se", "Na", "Li", "Mg", "Ca", "Al", "Sn", "Zn", "Cu", "Fe", "As", "Te")


def smiles_heavy_atoms(smiles: str) -> int:
    """Number of non-hydrogen atoms of a SMILES string, without rdkit: one per bracket atom (other than [H] / isotopes of H), per
    two-letter element, per organic-subset letter (B C N O P S F I) and per aromatic letter (b c n o p s).  That is the node count
    of the molecule's graph in the reference (mol.GetNumAtoms() of the kekulised molecule, data_loader_mol.py / mol_utils.py)."""
    n, i, L = 0, 0, len(smiles)
    while i < L:
        ch = smiles[i]
        if ch == "[":
            j = smiles.index("]", i)
            body = smiles[i + 1:j].lstrip("0123456789")
            sym = body[:2] if body[:2] in _TWO_LETTER else body[:1]
            if sym not in ("H",):
                n += 1
            i = j + 1
        elif smiles[i:i + 2] in _TWO_LETTER:
            n += 1
            i += 2
        elif ch in "BCNOPSFI" or ch in "bcnops":
            n += 1
            i += 1
        else:
            i += 1
    return n


def mol_train_node_counts(config, configt):
    """Node counts of the TRAINING molecules of QM9 / ZINC250k in the reference's order (data_loader_mol.py:352-379: the molecules of
    <dataset>_kekulized.npz in file order minus the indices of valid_idx_<dataset>.json), from the user's own copy of the dataset --
    the reference repository does not ship these blobs (.MISSING_LARGE_BLOBS).  Looked up under <folder>/<data.dir>/:
      <dataset>_kekulized.npz   arr_0 = atomic numbers per molecule, zero padded -> count of non-zeros (what the reference itself loads), else
      <dataset>.csv             column SMILES1 (QM9) / smiles (ZINC250k) -> heavy atoms per SMILES (smiles_heavy_atoms)
    with valid_idx_<dataset>.json beside it.  Returns None when neither file (or the index file) is there."""
    data = _get(configt, "data")
    name = str(_get(data, "data")).lower()
    folder = _get(config, "folder", "./")
    ddir = _get(_get(config, "data"), "dir", None) or _get(data, "dir", "./data")
    for base in dict.fromkeys([os.path.join(folder, ddir), os.path.join(folder, "data")]):
        idx_path = os.path.join(base, f"valid_idx_{name}.json")
        npz, csv_path = os.path.join(base, f"{name}_kekulized.npz"), os.path.join(base, f"{name}.csv")
        if not os.path.exists(idx_path) or not (os.path.exists(npz) or os.path.exists(csv_path)):
            continue
        with open(idx_path) as f:
            test_idx = json.load(f)
        if isinstance(test_idx, dict):                       # QM9: {"valid_idxs": ["123", ...]}
            test_idx = test_idx["valid_idxs"]
        test_idx = {int(i) for i in test_idx}
        if os.path.exists(npz):
            with np.load(npz, allow_pickle=True) as z:
                counts = np.array([int(np.count_nonzero(np.asarray(x))) for x in z["arr_0"]], dtype=np.int64)
        else:
            import csv

            col = "SMILES1" if name == "qm9" else "smiles"
            with open(csv_path, newline="") as f:
                counts = np.array([smiles_heavy_atoms(row[col]) for row in csv.DictReader(f)], dtype=np.int64)
        keep = np.ones(len(counts), dtype=bool)
        keep[[i for i in test_idx if i < len(counts)]] = False
        return counts[keep]
    return None


def graph_train_node_counts(config, configt):
    """Node counts of the TRAINING graphs of a generic dataset that node_counts.json does not cover (ENZYMES, grid), from the user's own
    copy of the dataset -- the file the reference itself loads (data_loader.py:76-81): <folder>/<data.dir>/<data>.pkl, a pickled list of
    networkx graphs; test_size = int(test_split * len(graph_list)), training split = graph_list[test_size:] in file order.  Returns
    (counts, test_size), or (None, 0) when the file is not there.  networkx is imported only here (the pickled graphs are its objects)."""
    data = _get(configt, "data")
    name = str(_get(data, "data"))
    folder = _get(configt, "folder", None) or _get(config, "folder", "./")
    dirs = [_get(data, "dir", "./data"), _get(_get(config, "data"), "dir", None), "data"]
    for base in dict.fromkeys(os.path.join(folder, d) for d in dirs if d):
        path = os.path.join(base, f"{name}.pkl")
        if not os.path.exists(path):
            continue
        import pickle

        import networkx  # noqa: F401

        with open(path, "rb") as f:
            graphs = pickle.load(f)
        test_size = int(_get(data, "test_split", 0.2) * len(graphs))
        return np.array([g.number_of_nodes() for g in graphs[test_size:]], dtype=np.int64), test_size
    return None, 0


class Sampler:
    """Common body of the four reference samplers.  The subclasses below carry the reference's per-class differences:
    `IS_MOL` (molecule datasets: one sampling round of sample.n_samples, quantize_mol + relabelling) and `APPLIES_EMA`
    (Sampler_Graph / Sampler_CC copy the EMA weights into the models when sample.use_ema is set, sampler.py:177-186, 458-471;
    Sampler_mol_Graph / Sampler_mol_CC never look at the switch, sampler.py:684-1240).  Instantiated directly, the class
    picks both from the dataset name."""

    IS_MOL: Optional[bool] = None
    APPLIES_EMA: Optional[bool] = None

    def __init__(self, config) -> None:
        self.config = config if isinstance(config, AttrDict) else AttrDict(config)
        self.is_cc = bool(_get(self.config, "is_cc", False))
        self.is_mol = self.IS_MOL if self.IS_MOL is not None else _get(_get(self.config, "data"), "data") in ("QM9", "ZINC250k")
        self.applies_ema = self.APPLIES_EMA if self.APPLIES_EMA is not None else not self.is_mol
        # Several GPUs (reference: load_device() returns every GPU and each network is wrapped in DataParallel, loader.py:58-68,
        # 134-135, 649-650).  Here: one process per GPU, each sampling a shard of every chunk (ccsd_amd/distributed.py).  A process
        # that belongs to a torch.distributed group -- started by torch.distributed.run, or by CCSD.run(gpus=N) -- takes the
        # sharded seam in load(); a lone process is the single-GPU harness.
        self.rank, self.world = 0, 1
        if (torch.distributed.is_available() and torch.distributed.is_initialized()) or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            from . import distributed

            self.rank, self.world, dev = distributed.init()
            self.device = dev if dev == "cpu" else [dev]
            self.device0 = dev
        else:
            self.device = loader.load_device()
            self.device0 = loader._device_id(self.device)
        sample = _get(self.config, "sample")
        # sharded runs: True (default) = the Langevin norm sums are all-reduced and Philox is keyed by the global sample index, i.e. the
        # statistics of the reference's DataParallel run (norms over the whole chunk); False = per-shard norms, no per-step traffic
        self.shard_exact = bool(_get(sample, "shard_exact", True))
        # every class: sample.n_samples, else the SAMPLING config's data.batch_size, else None (sampler.py:116-118, 393-395, 705-707)
        self.n_samples = _get(sample, "n_samples", _get(_get(self.config, "data"), "batch_size", None))
        self.divide_batch = _get(sample, "divide_batch", 1) or 1
        # diff_traj has one consumer, the plotting code behind general_config.plotly_fig (sampler.py:329, 644, 983, 1402): it is
        # recorded exactly when that switch is on; `extra["keep_traj"]` overrides
        self.keep_traj = bool(_get(_get(self.config, "general_config", {}), "plotly_fig", False))
        self.extra = {}          # forwarded to get_pc_sampler / S4_solver (rng, seed, keep_traj, group, lib, ...)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(is_cc={self.is_cc}, data={_get(_get(self.config, 'data'), 'data')})"

    # -- pieces of sample(), reusable on their own
    def load(self, node_counts=None):
        """`node_counts`: the caller's node counts (sample(node_counts=...)); they stand in when no dataset source is found."""
        cfg = self.config
        self.ckpt_dict = loader.load_ckpt(cfg, self.device, is_cc=self.is_cc)
        self.configt = self.ckpt_dict["config"]
        loader.load_seed(_get(cfg, "seed", 42))
        parts = ["x", "adj"] + (["rank2"] if self.is_cc else [])
        use_ema = self.applies_ema and bool(_get(_get(cfg, "sample"), "use_ema", False))
        self.models = []
        for p in parts:
            sd = dict(self.ckpt_dict[f"{p}_state_dict"])
            if use_ema:
                ema = self.ckpt_dict.get(f"ema_{p}")
                if ema is None:
                    raise KeyError(f"sample.use_ema is set but the checkpoint holds no EMA weights for {p}")
                sd.update(ema)                                            # ema.copy_to(model.parameters()), sampler.py:469-471
            self.models.append(loader.load_model_from_ckpt(self.ckpt_dict[f"params_{p}"], sd, self.device))
        data = _get(cfg, "data")
        extra = dict({"keep_traj": self.keep_traj}, **self.extra)
        if self.world > 1:
            # full-chunk flags in, all-gathered full chunk out on every rank: the contract of the reference's DataParallel call
            from . import distributed

            self.sampling_fn = distributed.load_sampling_fn_sharded(self.configt, _get(cfg, "sampler"), _get(cfg, "sample"), self.device,
                                                                    is_cc=self.is_cc, d_min=_get(data, "d_min"), d_max=_get(data, "d_max"),
                                                                    divide_batch=self.divide_batch, exact=self.shard_exact, **extra)
        else:
            self.sampling_fn = loader.load_sampling_fn(self.configt, _get(cfg, "sampler"), _get(cfg, "sample"), self.device,
                                                       is_cc=self.is_cc, d_min=_get(data, "d_min"), d_max=_get(data, "d_max"),
                                                       divide_batch=self.divide_batch, **extra)
        counts, self.n_test = train_node_counts(self.configt, with_test_size=True)
        self.node_counts_source = "shipped per-graph node counts of the training split (ccsd_amd/data/node_counts.json)"
        if counts is None and not self.is_mol:
            # generic datasets without shipped counts (ENZYMES, grid): the training graphs of the user's dataset copy, reference order
            counts, n_test = graph_train_node_counts(cfg, self.configt)
            if counts is not None:
                self.n_test = n_test
                self.node_counts_source = "training graphs of the dataset under <folder>/<data.dir> (reference order)"
        if counts is None and self.is_mol:
            # molecule datasets: the training molecules of the user's own dataset copy, as the reference draws them (sampler.py:1162-1194)
            counts = mol_train_node_counts(cfg, self.configt)
            self.node_counts_source = "training molecules of the dataset under <folder>/data (reference order)"
        if counts is None:
            with open(_COUNTS) as f:
                entry = json.load(f).get(_dataset_key(_get(_get(self.configt, "data"), "data")), {})
            counts = entry.get("test_histogram") or entry.get("fallback_histogram")
            if counts is None and node_counts is None:
                name = _get(_get(self.configt, "data"), "data")
                raise FileNotFoundError(f"no node counts for dataset {name}: put the dataset's {name}.pkl under <folder>/<data.dir> or pass "
                                        "`node_counts=` to sample()")
            if counts is None:
                counts = node_counts
                self.node_counts_source = "node_counts= of the caller"
            else:
                self.node_counts_source = entry.get("note", "shipped node-count histogram")
            if self.rank == 0 and counts is not node_counts:
                print(f"init_flags: dataset files not found under {_get(cfg, 'folder', './')}/data -- node counts are drawn from the shipped "
                      f"histogram ({self.node_counts_source})")
        self.node_counts = counts

    def sample(self, save: bool = False, node_counts=None, rounds: Optional[int] = None, dense_rank2: bool = True) -> Dict[str, torch.Tensor]:
        """`dense_rank2=False` leaves the dense incidence tensors `rank2` and `rank2_int` out of the result and the saved file (the cell
        bitmask and the descriptors describe the rank-2 cells); everything else is unchanged."""
        cfg = self.config
        self.load(node_counts)
        if node_counts is not None:
            self.node_counts = node_counts
        loader.load_seed(_get(_get(cfg, "sample"), "seed", 42))
        datat = _get(self.configt, "data")
        # flags per chunk: n_samples // divide_batch, or the training batch size when no n_samples is configured
        # (sampler.py:210-214, 498-502, 794-796, 1185-1187; init_flags' default, cc_utils.py:901-902)
        qty = self.n_samples // self.divide_batch if self.n_samples is not None else None
        if self.is_mol:
            n_rounds = 1
        else:
            bs = _get(datat, "batch_size")
            n_rounds = rounds if rounds is not None else max(1, math.ceil(self.n_test / bs))   # sampler.py:200-202, 488-490
        t0 = time.perf_counter()
        outs: List[List[torch.Tensor]] = []
        flags_all = []
        diff_traj = []
        for _ in range(n_rounds):
            parts = None
            for _d in range(self.divide_batch):
                # (sharded runs: every rank draws the same full-chunk flags from its identically seeded numpy stream)
                fl = init_flags(self.node_counts, self.configt, qty, is_cc=self.is_cc).to(self.device0)
                res = self.sampling_fn(*self.models, fl)
                nt = 3 if self.is_cc else 2
                if parts is None:
                    diff_traj = res[-1]        # the first chunk's trajectory of the (last) round is the one kept (sampler.py:220, 511)
                parts = list(res[:nt]) if parts is None else [torch.cat((a, b), dim=0) for a, b in zip(parts, res[:nt])]
                flags_all.append(fl)
            outs.append(parts)
        self.diff_traj = diff_traj
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        sampling_time = time.perf_counter() - t0
        x, adj = (torch.cat([o[k] for o in outs], dim=0) for k in (0, 1))
        rank2 = torch.cat([o[2] for o in outs], dim=0) if self.is_cc else None
        out: Dict[str, torch.Tensor] = {"x": x, "adj": adj, "flags": torch.cat(flags_all, dim=0)}
        quant = SampleOps(self.device0, self.extra.get("lib"))
        # one call: quantize / quantize_mol (graph_utils.py:181-213), the sparse form of the rank-2 incidence matrix for cc_from_incidence
        # (cc_utils.py:243-262) and the per-complex descriptors the evaluators histogram (stats.py:36, cc_utils.py:1208-1334)
        datac = _get(cfg, "data")
        fin = quant.finish(x, adj, rank2, out["flags"], mol=self.is_mol, thr=0.5, dense_rank2=dense_rank2,
                           d_min=(_get(datac, "d_min") or _get(datat, "d_min") or 0) if self.is_cc else 0,
                           d_max=(_get(datac, "d_max") or _get(datat, "d_max") or 0) if self.is_cc else 0)
        if self.is_mol:
            samples_int = fin["adj_int"]                                     # quantize_mol, graph_utils.py:195-213
            samples_int = samples_int - 1
            samples_int[samples_int == -1] = 3                               # 0,1,2,3 (no,S,D,T) -> 3,0,1,2 (sampler.py:1219-1220)
            out["adj_int"] = samples_int
            out["adj_onehot"] = torch.nn.functional.one_hot(samples_int, num_classes=4).permute(0, 3, 1, 2)
            xi = torch.where(x > 0.5, 1, 0)
            out["x_onehot"] = torch.concat([xi, 1 - xi.sum(dim=-1, keepdim=True)], dim=-1)
        else:
            out["adj_int"] = fin["adj_int"]                                  # quantize, graph_utils.py:181-192
        for k in ("n_nodes", "degree", "degree_hist", "edge_hist", "x_hist"):
            out[k] = fin[k]
        if self.is_cc:
            if dense_rank2:
                out["rank2"] = rank2
                out["rank2_int"] = fin["rank2_int"]
            # sparse form for cc_from_incidence (cc_utils.py:243-262): which of the K candidate cells exist, per complex
            for k in ("rank2_cell_bits", "rank2_cell_count", "rank2_cell_hist", "rank2_nnz"):
                out[k] = fin[k]
        out["sampling_time"] = torch.tensor(sampling_time)
        self.result = out
        if save and self.rank == 0:          # every rank holds the gathered samples; rank 0 writes them
            folder = os.path.join(_get(cfg, "folder", "./"), "samples")
            os.makedirs(folder, exist_ok=True)
            name = f"{_get(cfg, 'config_name', 'sample')}_{_get(cfg, 'ckpt')}-sample_{_get(cfg, 'current_time', 'now')}"
            np.savez_compressed(os.path.join(folder, name + ".npz"), **{k: v.detach().cpu().numpy() for k, v in out.items()})
        if self.rank == 0:
            print("Sampling done.")
        return out

    def molecules(self, result, largest_fragment: bool = True) -> Dict[str, torch.Tensor]:
        """The molecules the reference scores (gen_mol, utils/mol_utils.py:191-229; Sampler_mol_*.sample calls it on every sample):
        SampleOps.mol_correct -- formal charges, valency correction, the largest fragment, with the data set's row of
        evaluation.MOL_TABLES -- of `result["adj"]` and evaluation.mol_labels(result["x"]).  `result`: what sample() returned (or any
        dict with raw `adj` (B,N,N) and `x` (B,N,F)).  Returns mol_correct's outputs plus "validity_wo_correction" = mol_no_correct.sum()
        / B, the first figure the reference prints for a molecule run.  Molecule samplers only: ValueError otherwise."""
        from . import evaluation as ev

        if not self.is_mol:
            raise ValueError("molecules: valency correction applies to molecule samplers (data.data QM9 or ZINC250k) only")
        name = _get(_get(self.config, "data"), "data")
        if name not in ev.MOL_TABLES:
            raise ValueError(f"molecules: no valence table for data.data = {name!r}; evaluation.MOL_TABLES has {sorted(ev.MOL_TABLES)}")
        missing = [k for k in ("adj", "x") if k not in result]
        if missing:
            raise KeyError(f"molecules: the result lacks {missing}")
        adj = torch.as_tensor(result["adj"]).to(device=self.device0, dtype=torch.float32)
        labels = ev.mol_labels(torch.as_tensor(result["x"])).to(self.device0)
        out = SampleOps(self.device0, self.extra.get("lib")).mol_correct(adj, labels, dataset=name, largest_fragment=largest_fragment)
        out["validity_wo_correction"] = float(out["mol_no_correct"].sum().item()) / max(adj.shape[0], 1)
        return out

    def evaluate(self, result, ref, methods: Optional[List[str]] = None, cc_methods: Optional[List[str]] = None, bins: int = 100,
                 cc_nb_eval: Optional[int] = 1000, spectra: bool = False, orbits: bool = False, nspdk: bool = False,
                 lift: bool = False, correct: bool = False) -> Dict[str, float]:
        """Score a finished run against a held-out set on the GPU (ccsd_amd/evaluation.py): what the reference prints after
        sampling from eval_graph_list and eval_CC_list (sampler.py:253-262, 565-583), for the methods this build computes.
        `result`: what sample() returned.  `ref`: an adjacency batch (B, N, N) of the held-out graphs, a descriptor dict
        (evaluation.describe), or the path of an .npz that sample(save=True) wrote.  Returns {method: round(score, 6)}: "degree" and
        "cluster" and, for combinatorial complexes whose two sides hold the descriptors, "rank1_distrib" and "rank2_distrib"
        (data.min_edge_val / data.max_edge_val of the config; default 1..3 for molecules, 1..1 otherwise).  sample() itself is
        untouched: nothing here runs unless it is called.  spectra=True adds the two scores that run an eigenvalue solver per
        sample: "spectral" and, for combinatorial complexes, "hodge_laplacian_spectrum" -- both computed from `adj` and
        `rank2_cell_bits`, so results of sample(dense_rank2=False) and saved .npz files serve as well.  orbits=True adds "orbit", the
        reference's third default score for generic graphs (orbit_stats_all: 4-node graphlet orbit counts per graph, which the
        reference gets from the external orca program), computed from `adj` of each side.  nspdk=True adds "nspdk", the graph score the
        reference prints for molecule runs (nspdk_stats; not rounded, as in the reference), computed from `adj` of each side (at most 64
        nodes) and integer node labels: for molecule samplers evaluation.mol_labels of the side's `x`, or its `nspdk_labels`
        (KeyError when a side has neither), label 0 otherwise.  Without `correct` it scores the quantised samples AS SAMPLED.
        correct=True (molecule samplers only, ValueError otherwise) first passes the PREDICTED side through molecules() -- the
        reference's gen_mol: formal charges, valency correction, largest fragment -- and computes every score from its mol_adj /
        mol_labels: "degree", "cluster", "nspdk" and, for complexes, "rank1_distrib" (the sampled rank-2 cells belong to the uncorrected
        molecule and are not scored).  Predicted molecules left without an atom are left out; the held-out side holds real molecules and
        is left as given, as in the reference.  The result gains "validity_wo_correction".
        lift=True LIFTS graphs to complexes by the config's rule (data.lifting_procedure /
        lifting_procedure_kwargs with data.d_min / d_max; evaluation.lift_settings, SampleOps.lift, at most 64 nodes), as the reference's
        data generators and Sampler_Graph do (sampler.py:259-287): on a sampler of complexes a side that has `adj` but no rank-2
        descriptors -- normally the held-out graphs -- is lifted, so that "rank2_distrib" and, with spectra=True,
        "hodge_laplacian_spectrum" are scored; on a graph sampler both sides are lifted and the eval_CC_batch scores are added (the
        reference's "CCs eval" line).  The cycles rule is networkx's cycle basis of the adjacency, not the reference's
        set-order-dependent one; both sides go through the same rule.  A config without lifting_procedure raises ValueError, a
        molecule sampler NotImplementedError (its cells are rdkit's rings, which this build does not have).  In a sharded run every
        rank holds the gathered samples and rank 0 alone evaluates; the other ranks return {}."""
        from . import evaluation as ev

        if correct and not self.is_mol:
            raise ValueError("evaluate: correct=True applies to molecule samplers (data.data QM9 or ZINC250k) only")
        if self.rank != 0:
            return {}
        validity = None
        if correct:
            if isinstance(result, (str, os.PathLike)):
                with np.load(result) as z:
                    result = {k: torch.from_numpy(z[k]) for k in ("adj", "x") if k in z.files}
            mols = self.molecules(result)
            validity = mols["validity_wo_correction"]
            kept = mols["mol_atoms"] > 0
            result = {"adj": mols["mol_adj"][kept].to(torch.float32), "nspdk_labels": mols["mol_labels"][kept], "n_nodes": mols["mol_atoms"][kept]}
        lib = self.extra.get("lib")
        kw = dict(device=self.device0, lib=lib)
        data = _get(self.config, "data")
        datat = _get(getattr(self, "configt", None), "data")     # (the cell sizes sample() hands to finish(); no checkpoint loaded yet: none)
        cell_sizes = dict(d_min=_get(data, "d_min") or _get(datat, "d_min") or 0, d_max=_get(data, "d_max") or _get(datat, "d_max") or 0)
        lift_kw = None
        if lift:
            if self.is_mol:
                raise NotImplementedError("evaluate: lift=True on a molecule sampler: the reference's cells of a molecule are rdkit's rings, which this build does not have")
            lift_kw = ev.lift_settings(data, _get(data, "max_node_num") or _get(datat, "max_node_num"))
            if lift_kw is None:
                raise ValueError("evaluate: lift=True needs data.lifting_procedure in the config")
            if not cell_sizes["d_min"] or not cell_sizes["d_max"]:
                raise ValueError("evaluate: lift=True needs data.d_min and data.d_max in the config")
            lift_kw.update(cell_sizes)

        keep = ("adj", "degree_hist", "edge_hist", "n_nodes", "rank2_cell_hist", "cluster_hist") + (
            ("rank2_cell_bits", "spectral_hist", "hodge_spectrum") if spectra else ()) + (("orbit_counts", "orbit_nodes") if orbits else ()) + (
            ("x", "nspdk_labels") + ev.NSPDK_KEYS if nspdk else ())

        def side(obj):
            if isinstance(obj, (str, os.PathLike)):
                with np.load(obj) as z:           # (only the kept keys are decompressed: the dense rank2 of a saved run is never read)
                    obj = {k: torch.from_numpy(z[k]) for k in keep if k in z.files}
            if isinstance(obj, dict):
                desc = {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)).to(self.device0) for k, v in obj.items() if k in keep}
                if "cluster_hist" not in desc or desc["cluster_hist"].shape[1] != bins or "degree_hist" not in desc or "edge_hist" not in desc:
                    if "adj" not in desc:
                        raise KeyError("evaluate: a descriptor dict needs degree_hist, edge_hist and cluster_hist, or adj to compute them from")
                    desc.update(ev.describe(desc["adj"], mol=self.is_mol, bins=bins, **kw))
                if nspdk and self.is_mol and not all(k in desc for k in ev.NSPDK_KEYS) and "x" not in desc and "nspdk_labels" not in desc:
                    raise KeyError("evaluate: nspdk=True on a molecule run needs x or nspdk_labels (or the nspdk_* rows) on each side")
                if lift_kw is not None and "rank2_cell_hist" not in desc:
                    if "adj" not in desc:
                        raise KeyError("evaluate: lift=True needs adj on a side without rank-2 descriptors")
                    desc.update(SampleOps(self.device0, lib).lift(desc["adj"].to(torch.float32), mol=self.is_mol, **lift_kw))
                return desc
            if nspdk and self.is_mol:
                raise KeyError("evaluate: nspdk=True on a molecule run needs x or nspdk_labels beside the adjacency batch: pass a dict")
            desc = ev.describe(torch.as_tensor(obj), mol=self.is_mol, bins=bins, orbits=orbits, nspdk=nspdk, lift=lift_kw, **kw)
            if lift_kw is not None:
                desc["adj"] = torch.as_tensor(obj).to(self.device0)          # (what hodge_laplacian_spectrum reads beside the lifted cells)
            return desc

        pred, held = side(result), side(ref)
        if methods is None:
            methods = ["degree", "cluster"] + (["orbit"] if orbits else []) + (["spectral"] if spectra else []) + (["nspdk"] if nspdk else [])
        out = ev.eval_torch_batch(held, pred, methods, bins=bins, mol=self.is_mol, spectra=spectra, orbits=orbits, nspdk=nspdk, **kw)
        if self.is_cc or lift_kw is not None:
            wk = {"min_edge_val": _get(data, "min_edge_val", 1), "max_edge_val": _get(data, "max_edge_val", 3 if self.is_mol else 1)}
            have = ["rank1_distrib"] + (["rank2_distrib"] if "rank2_cell_hist" in pred and "rank2_cell_hist" in held else [])
            if spectra:
                wk.update(cell_sizes)
                if all("hodge_spectrum" in d or ("adj" in d and "rank2_cell_bits" in d) for d in (pred, held)):
                    have.append("hodge_laplacian_spectrum")
            out.update(ev.eval_CC_batch(held, pred, wk, have if cc_methods is None else cc_methods, cc_nb_eval=cc_nb_eval, spectra=spectra,
                                        mol=self.is_mol, **kw))
        if validity is not None:
            out["validity_wo_correction"] = validity
        return out


# the reference's four class names (sampler.py:92, 369, 684, 1061) and its factory (sampler.py:1438-1468)
class Sampler_Graph(Sampler):
    IS_MOL, APPLIES_EMA = False, True


class Sampler_CC(Sampler):
    IS_MOL, APPLIES_EMA = False, True


class Sampler_mol_Graph(Sampler):
    IS_MOL, APPLIES_EMA = True, False


class Sampler_mol_CC(Sampler):
    IS_MOL, APPLIES_EMA = True, False


def get_sampler_from_config(config) -> Sampler:
    config = config if isinstance(config, AttrDict) else AttrDict(config)
    is_cc = bool(_get(config, "is_cc", False))
    is_mol = _get(_get(config, "data"), "data") in ("QM9", "ZINC250k")
    cls = (Sampler_mol_CC if is_cc else Sampler_mol_Graph) if is_mol else (Sampler_CC if is_cc else Sampler_Graph)
    return cls(config)
