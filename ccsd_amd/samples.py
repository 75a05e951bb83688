"""SampleOps: the plan-free half of the C ABI -- operations on FINISHED samples (quantise, describe, score), which take tensors
and sizes and never a ccsd_plan_t.  Constructing one builds no network plan; PCEngine inherits the same methods.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _adj_mode(mol: bool) -> int:
    return _lib.FINISH_ADJ_MOL if mol else _lib.FINISH_ADJ_QUANTIZE


class SampleOps:
    def __init__(self, device="cuda", lib: Optional[_lib.Library] = None):
        self.lib = lib if lib is not None else _lib.get_library()
        self.device = torch.device(device)
        if self.lib.is_hip:
            if self.device.type != "cuda":
                raise _lib.CcsdError("the HIP library needs a cuda (ROCm) device; ccsd_amd has no CPU path")
            if not torch.cuda.is_available():
                raise _lib.CcsdError("no MI355X visible: ccsd_amd has no CPU fallback")
        self._edges: dict = {}          # (lo, hi, bins, device) -> np.linspace(lo, hi, bins + 1) on the device

    # -- helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.lib.is_hip else None

    def _scratch(self, nbytes: int, device) -> torch.Tensor:
        return torch.empty(max(int(nbytes), 8) // 8 + 1, dtype=torch.float64, device=device)        # (8-byte aligned)

    def _adj(self, who: str, adj: torch.Tensor) -> torch.Tensor:
        """The (B, N, N) float32 adjacency argument of `who`, contiguous."""
        if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
            raise ValueError(f"{who}: adj must be (B, N, N), got {tuple(adj.shape)}")
        if adj.dtype != torch.float32 or adj.device.type != self.device.type:
            raise ValueError(f"{who}: adj must be float32 on {self.device}, got {adj.dtype} {adj.device}")
        return adj.contiguous()

    def _hist_edges(self, who: str, lo: float, hi: float, bins: int, device) -> torch.Tensor:
        """numpy's own bin edges np.linspace(lo, hi, bins + 1) as a device tensor, uploaded once per (lo, hi, bins, device)."""
        if not 1 <= bins <= _lib.CLUSTER_MAX_BINS:
            raise ValueError(f"{who}: bins = {bins} outside 1..{_lib.CLUSTER_MAX_BINS}")
        key = (lo, hi, bins, device)
        if key not in self._edges:
            self._edges[key] = torch.from_numpy(np.linspace(lo, hi, bins + 1)).to(device)
        return self._edges[key]

    # -- API
    def quantize(self, t: torch.Tensor, thr: float = 0.5) -> torch.Tensor:
        """thr < 0 selects quantize_mol's 0/1/2/3 bins."""
        t = t.contiguous()
        out = torch.empty(t.shape, dtype=torch.int64, device=t.device)
        self.lib.check(self.lib.ccsd_quantize(_ptr(t), t.numel(), float(thr), _ptr(out), self._stream()))
        return out

    def rank2_cells(self, rank2: torch.Tensor, thr: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
        """Sparse form of quantize(rank2): (bits (B, ceil(K/64)) int64 -- bit k%64 of word k//64 set iff column k holds a
        rank-2 cell --, counts (B,) int32).  cells_from_bits turns a row into the cell tuples cc_from_incidence adds."""
        rank2 = rank2.contiguous()
        B, E, K = rank2.shape
        bits = torch.zeros(B, (K + 63) // 64, dtype=torch.int64, device=rank2.device)
        counts = torch.zeros(B, dtype=torch.int32, device=rank2.device)
        self.lib.check(self.lib.ccsd_rank2_cells(_ptr(rank2), B, E, K, float(thr), _ptr(bits), _ptr(counts), self._stream()))
        return bits, counts

    def finish(self, x: Optional[torch.Tensor], adj: Optional[torch.Tensor], rank2: Optional[torch.Tensor] = None,
               flags: Optional[torch.Tensor] = None, *, mol: bool = False, thr: float = 0.5, d_min: int = 0, d_max: int = 0,
               dense_rank2: bool = True, descriptors: bool = True, dense_adj: bool = True) -> dict:
        """The finish of a sampling run in one C call (ccsd_finish): one pass over (x, adj) and one over rank2.
          adj_int (B,N,N) int64         quantize_mol(adj) if `mol` else quantize(adj, thr), as quantize()        [dense_adj]
          degree, degree_hist (B,N), edge_hist (B,4), n_nodes (B,), x_hist (B,F) int32                            [descriptors]
        and, with rank2 (B,E,K) and its cell sizes d_min..d_max,
          rank2_int (B,E,K) uint8       quantize(rank2, thr)                                                       [dense_rank2]
          rank2_cell_bits (B,ceil(K/64)) int64, rank2_cell_count (B,) int32      as rank2_cells()
          rank2_cell_hist (B,d_max-d_min+1), rank2_nnz (B,) int32                                                  [descriptors]
        A switched-off group is left out of the result and never computed.  No tensor of rank2's shape other than the uint8 output is
        allocated.  x or adj may be None (their outputs are then left out)."""
        ref = adj if adj is not None else x
        if ref is None:
            raise ValueError("finish: x or adj is required")
        B, N = ref.shape[0], ref.shape[1]
        dev = ref.device
        x = None if x is None else x.contiguous()
        adj = None if adj is None else adj.contiguous()
        if adj is not None and (adj.dim() != 3 or tuple(adj.shape) != (B, N, N)):
            raise ValueError(f"finish: adj must be (B, N, N), got {tuple(adj.shape)}")
        if x is not None and (x.dim() != 3 or tuple(x.shape[:2]) != (B, N)):
            raise ValueError(f"finish: x must be (B, N, F) with B, N = {B}, {N}, got {tuple(x.shape)}")
        F = x.shape[2] if x is not None else 1
        E, K = N * (N - 1) // 2, 0
        res = {}

        def new(name, shape, dtype):
            res[name] = torch.empty(shape, dtype=dtype, device=dev)

        if adj is not None:
            if dense_adj:
                new("adj_int", (B, N, N), torch.int64)
            if descriptors:
                new("degree", (B, N), torch.int32)
                new("degree_hist", (B, N), torch.int32)
                new("edge_hist", (B, 4), torch.int32)
        if x is not None and descriptors:
            new("n_nodes", (B,), torch.int32)
            new("x_hist", (B, F), torch.int32)
        if rank2 is not None:
            rank2 = rank2.contiguous()
            if rank2.dim() != 3 or rank2.shape[0] != B:
                raise ValueError(f"finish: rank2 must be (B, E, K) with B = {B}, got {tuple(rank2.shape)}")
            E, K = rank2.shape[1], rank2.shape[2]
            if dense_rank2:
                new("rank2_int", (B, E, K), torch.uint8)
            new("rank2_cell_bits", (B, (K + 63) // 64), torch.int64)
            new("rank2_cell_count", (B,), torch.int32)
            if descriptors:
                new("rank2_cell_hist", (B, max(d_max - d_min + 1, 1)), torch.int32)
                new("rank2_nnz", (B,), torch.int32)
        for name, t in (("x", x), ("adj", adj), ("rank2", rank2), ("flags", flags)):
            if t is not None and (t.dtype != torch.float32 or t.device.type != self.device.type):
                raise ValueError(f"finish: {name} must be float32 on {self.device}, got {t.dtype} {t.device}")
        dims = _lib.FinishDims(B, N, F, E, K, int(d_min), int(d_max), _adj_mode(mol), float(thr))
        out = _lib.FinishOut(*[_ptr(res.get("rank2_int" if n == "rank2_u8" else n)) for n in _lib.FINISH_OUTPUTS])
        st = _lib.State(_ptr(x), _ptr(adj), _ptr(rank2))
        self.lib.check(self.lib.ccsd_finish(C.byref(dims), C.byref(st), _ptr(flags), C.byref(out), self._stream()))
        return res

    def cluster_hist(self, adj: torch.Tensor, *, mol: bool = False, thr: float = 0.5, bins: int = 100, tri2: bool = True) -> dict:
        """Clustering-coefficient histogram per graph (ccsd_cluster_hist): clustering_worker of the reference (evaluation/stats.py:206-220)
        on adjs_to_graphs of the quantised adjacency, with finish()'s quantiser (`mol`, `thr`).  adj (B,N,N) float32, SYMMETRIC.
          cluster_hist (B,bins) int32   np.histogram(nx.clustering(G).values(), bins, range=(0, 1))
          tri2 (B,N) int32              twice the triangles through each node                                      [tri2]
        The bin edges are numpy's own: np.linspace(0.0, 1.0, bins + 1), uploaded once per `bins`."""
        adj = self._adj("cluster_hist", adj)
        B, N = adj.shape[0], adj.shape[1]
        bins = int(bins)
        edges = self._hist_edges("cluster_hist", 0.0, 1.0, bins, adj.device)
        res = {"cluster_hist": torch.empty((B, bins), dtype=torch.int32, device=adj.device)}
        if tri2:
            res["tri2"] = torch.empty((B, N), dtype=torch.int32, device=adj.device)
        self.lib.check(self.lib.ccsd_cluster_hist(_ptr(adj), B, N, _adj_mode(mol), float(thr), _ptr(edges), bins, _ptr(res.get("tri2")),
                                                  _ptr(res["cluster_hist"]), self._stream()))
        return res

    def orbit_counts(self, adj: torch.Tensor, *, mol: bool = False, thr: float = 0.5, per_node: bool = False) -> dict:
        """4-node graphlet orbit counts per graph (ccsd_orbit_counts): what orbit_stats_all of the reference (evaluation/stats.py:382-435)
        reads from the external orca program (`orca node 4`) for adjs_to_graphs of the quantised adjacency, with finish()'s quantiser
        (`mol`, `thr`; in mol mode every bond order is a plain edge).  adj (B,N,N) float32, SYMMETRIC.
          orbit_counts (B,15) int64     the column sums of orca's per-node rows (ORCA's orbit numbering, include/ccsd_hip.h)
          orbit_nodes (B,) int32        G.number_of_nodes(): the nodes that have an edge, 1 for a graph without any
          node_orbits (B,N,15) int64    the per-node rows, zeros for nodes without an edge                          [per_node]
        Nothing is synchronised."""
        adj = self._adj("orbit_counts", adj)
        B, N = adj.shape[0], adj.shape[1]
        res = {"orbit_counts": torch.empty((B, _lib.ORBITS), dtype=torch.int64, device=adj.device),
               "orbit_nodes": torch.empty((B,), dtype=torch.int32, device=adj.device)}
        if per_node:
            res["node_orbits"] = torch.empty((B, N, _lib.ORBITS), dtype=torch.int64, device=adj.device)
        self.lib.check(self.lib.ccsd_orbit_counts(_ptr(adj), B, N, _adj_mode(mol), float(thr), _ptr(res.get("node_orbits")),
                                                  _ptr(res["orbit_counts"]), _ptr(res["orbit_nodes"]), self._stream()))
        return res

    def nspdk_features(self, adj: torch.Tensor, labels: Optional[torch.Tensor] = None, *, mol: bool = False, thr: float = 0.5) -> dict:
        """NSPDK feature rows (ccsd_nspdk_features): what vectorize(graphs, complexity=4, discrete=True) of the reference
        (evaluation/eden.py; mmd.py:331-337) gives for the graphs of the quantised adjacency, finish()'s quantiser (`mol`, `thr`; in
        mol mode the bond order 1..3 is the edge label), when nodes carry INTEGER labels.  adj (B,N,N) float32, SYMMETRIC, N <= 64.
        labels (B,N) integer: the label per node slot, negative = the slot holds no node (its edges are ignored); None = every slot is
        a node with label 0.  -> the rows in CSR form, compacted on the device:
          nspdk_indptr (B+1,) int64, nspdk_indices (nnz,) int32 ascending within a row in 1..65536, nspdk_values (nnz,) float64
        Each row has unit L2 norm; a graph without a node has an empty row.  Two calls give identical bits.  The one host round trip
        is the total size.  N > 64 raises NotImplementedError."""
        adj = self._adj("nspdk_features", adj)
        B, N = adj.shape[0], adj.shape[1]
        if labels is not None:
            if tuple(labels.shape) != (B, N) or labels.dtype.is_floating_point or labels.device.type != self.device.type:
                raise ValueError(f"nspdk_features: labels must be integer of shape ({B}, {N}) on {self.device}, got {labels.dtype} {tuple(labels.shape)} {labels.device}")
            labels = labels.to(torch.int32).contiguous()
        cap = self.lib.ccsd_nspdk_row_capacity(N)
        nbytes = self.lib.ccsd_nspdk_workspace_bytes(B, N)
        if cap == 0 or nbytes == 0:
            self.lib.check(_lib.ERR_UNSUPPORTED if N > _lib.NSPDK_MAX_NODES else _lib.ERR_INVALID)
        nnz = torch.empty((B,), dtype=torch.int32, device=adj.device)
        idx = torch.empty((B, cap), dtype=torch.int32, device=adj.device)
        val = torch.empty((B, cap), dtype=torch.float64, device=adj.device)
        ws = self._scratch(nbytes, adj.device)
        self.lib.check(self.lib.ccsd_nspdk_features(_ptr(adj), _ptr(labels), B, N, _adj_mode(mol), float(thr), _ptr(nnz), _ptr(idx), _ptr(val),
                                                    _ptr(ws), ws.numel() * 8, self._stream()))
        indptr = torch.zeros((B + 1,), dtype=torch.int64, device=adj.device)
        torch.cumsum(nnz, 0, out=indptr[1:])
        keep = torch.arange(cap, device=adj.device)[None, :] < nnz[:, None]
        return {"nspdk_indptr": indptr, "nspdk_indices": idx[keep], "nspdk_values": val[keep]}

    def nspdk_mmd(self, a: dict, b: dict) -> torch.Tensor:
        """compute_nspdk_mmd of the reference (evaluation/mmd.py:352-377) on two sets of nspdk_features rows (ccsd_nspdk_mmd) -> a
        float64 device tensor [mean Kxx, mean Kyy, mean Kxy, mmd].  a: the reference set (empty rows count as zero vectors), b: the
        predicted set (empty rows are left out, as nspdk_stats drops graphs without a node).  Nothing is synchronised."""
        sets = []
        for name, d in (("a", a), ("b", b)):
            try:
                ip, ix, vl = d["nspdk_indptr"], d["nspdk_indices"], d["nspdk_values"]
            except KeyError as e:
                raise KeyError(f"nspdk_mmd: set {name} lacks {e.args[0]}; nspdk_features produces it") from None
            if ip.dtype != torch.int64 or ix.dtype != torch.int32 or vl.dtype != torch.float64 or ip.dim() != 1 or ip.numel() < 2 or ix.shape != vl.shape:
                raise ValueError(f"nspdk_mmd: set {name} must hold nspdk_indptr (n+1,) int64, nspdk_indices int32 and nspdk_values float64 of one shape")
            for t in (ip, ix, vl):
                if t.device.type != self.device.type:
                    raise ValueError(f"nspdk_mmd: set {name} must be on {self.device}, got {t.device}")
            if ix.numel() == 0:                                   # (no non-zero at all: the C call still wants addresses)
                ix, vl = ix.new_zeros(1), vl.new_zeros(1)
            sets.append((ip.contiguous(), ix.contiguous(), vl.contiguous(), ip.numel() - 1))
        (p1, i1, v1, n1), (p2, i2, v2, n2) = sets
        out = torch.empty(4, dtype=torch.float64, device=p1.device)
        nbytes = self.lib.ccsd_nspdk_mmd_workspace_bytes(n1, n2)
        if nbytes == 0:
            self.lib.check(_lib.ERR_INVALID)
        ws = self._scratch(nbytes, p1.device)
        self.lib.check(self.lib.ccsd_nspdk_mmd(_ptr(p1), _ptr(i1), _ptr(v1), n1, _ptr(p2), _ptr(i2), _ptr(v2), n2, _ptr(ws), ws.numel() * 8,
                                               _ptr(out), self._stream()))
        return out

    def mmd(self, s1: torch.Tensor, s2: torch.Tensor, kind: str = "emd", *, is_hist: bool = True, degree: bool = False,
            f32_pmf: bool = False, sigma: float = 1.0, distance_scaling: float = 1.0, lens1: Optional[torch.Tensor] = None,
            lens2: Optional[torch.Tensor] = None) -> torch.Tensor:
        """compute_mmd of the reference (evaluation/mmd.py:230-257) on the device (ccsd_mmd): s1 (n1,L), s2 (n2,L) int32 or float64
        histograms with one row per sample -> a float64 device tensor [disc(1,1), disc(2,2), disc(1,2), mmd].  kind: "emd"
        (gaussian_emd), "tv" (gaussian_tv), "l2" (gaussian).  degree: the rows are finish()'s degree_hist (bin 0 is no node of the
        reference's graphs).  f32_pmf: normalise in float32, as numpy does for float32 histograms.  lens1 / lens2 (n,) int32: the
        lengths of the original arrays of a ragged set (they matter only to the EMD of rows without mass).  Nothing is synchronised."""
        kinds = {"emd": _lib.MMD_EMD, "tv": _lib.MMD_TV, "l2": _lib.MMD_L2}
        if kind not in kinds:
            raise ValueError(f"mmd: kind must be one of {sorted(kinds)}, got {kind!r}")
        if s1.dim() != 2 or s2.dim() != 2 or s1.shape[1] != s2.shape[1]:
            raise ValueError(f"mmd: s1 and s2 must be (n1, L) and (n2, L), got {tuple(s1.shape)} and {tuple(s2.shape)}")
        if s1.dtype != s2.dtype or s1.dtype not in (torch.int32, torch.float64):
            raise ValueError(f"mmd: s1 and s2 must both be int32 or both float64, got {s1.dtype} and {s2.dtype}")
        for name, t in (("s1", s1), ("s2", s2), ("lens1", lens1), ("lens2", lens2)):
            if t is not None and t.device.type != self.device.type:
                raise ValueError(f"mmd: {name} must be on {self.device}, got {t.device}")
        for name, t, s in (("lens1", lens1, s1), ("lens2", lens2, s2)):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (s.shape[0],)):
                raise ValueError(f"mmd: {name} must be int32 of shape ({s.shape[0]},), got {t.dtype} {tuple(t.shape)}")
        s1, s2 = s1.contiguous(), s2.contiguous()
        lens1, lens2 = (None if t is None else t.contiguous() for t in (lens1, lens2))
        n1, n2, L = s1.shape[0], s2.shape[0], s1.shape[1]
        out = torch.empty(4, dtype=torch.float64, device=s1.device)
        ws = self._scratch(self.lib.ccsd_mmd_workspace_bytes(n1, n2, L), s1.device)
        flags = (_lib.MMD_IS_HIST if is_hist else 0) | (_lib.MMD_DEGREE if degree else 0) | (_lib.MMD_F32_PMF if f32_pmf else 0)
        self.lib.check(self.lib.ccsd_mmd(_ptr(s1), n1, _ptr(lens1), _ptr(s2), n2, _ptr(lens2), L,
                                         _lib.MMD_FP64 if s1.dtype == torch.float64 else _lib.MMD_INT32, kinds[kind], flags, float(sigma),
                                         float(distance_scaling), _ptr(ws), ws.numel() * 8, _ptr(out), self._stream()))
        return out

    def eigvalsh(self, a: torch.Tensor, *, sweeps: bool = False):
        """Eigenvalues of symmetric matrices, ascending (ccsd_eigvalsh: a batched Jacobi solver; what numpy.linalg.eigvalsh gives, to
        a small multiple of n 2^-53 ||A||_F).  a: (B, n, n) or (n, n) float64 on the device, 1 <= n <= 512; it is not modified.
        sweeps=True also returns the (B,) int32 sweep counts (negative: the sweep cap ended the iteration).  Nothing is synchronised."""
        single = a.dim() == 2
        if single:
            a = a.unsqueeze(0)
        if a.dim() != 3 or a.shape[1] != a.shape[2]:
            raise ValueError(f"eigvalsh: a must be (B, n, n), got {tuple(a.shape)}")
        if a.dtype != torch.float64 or a.device.type != self.device.type:
            raise ValueError(f"eigvalsh: a must be float64 on {self.device}, got {a.dtype} {a.device}")
        a = a.contiguous()
        B, n = a.shape[0], a.shape[1]
        w = torch.empty((B, n), dtype=torch.float64, device=a.device)
        sw = torch.empty((B,), dtype=torch.int32, device=a.device)
        if B and n:
            ws = self._scratch(self.lib.ccsd_eig_workspace_bytes(B, min(n, _lib.EIG_MAXN)), a.device)
            self.lib.check(self.lib.ccsd_eigvalsh(_ptr(a), B, n, _ptr(w), _ptr(sw), _ptr(ws), ws.numel() * 8, self._stream()))
        if single:
            w, sw = w[0], sw[0]
        return (w, sw) if sweeps else w

    def spectral_hist(self, adj: torch.Tensor, *, mol: bool = False, thr: float = 0.5, bins: int = 200, eig: bool = False) -> dict:
        """Histogram of the normalised Laplacian's eigenvalues per graph (ccsd_spectral_hist): spectral_worker of the reference
        (evaluation/stats.py:125-137) on adjs_to_graphs of the quantised adjacency, with finish()'s quantiser (`mol`, `thr`; in mol
        mode the bond orders are the edge weights).  adj (B,N,N) float32, SYMMETRIC.
          spectral_hist (B,bins) int32   np.histogram(eigvalsh(L), bins, range=(-1e-5, 2)) -- counts; compute_mmd normalises them
          spectral_eig (B,N) float64, spectral_n (B,) int32    the n eigenvalues ascending, then zeros                [eig]
        Eigenvalues are clamped to [0, 2] before binning: an eigenvalue 2 of a bipartite component that a solver rounds above 2 still
        counts in the last bin (the reference drops it).  The bin edges are np.linspace(-1e-5, 2, bins + 1), uploaded once per `bins`.
        The call allocates its workspace, which holds every Laplacian: 8 B N^2 bytes (2 GB for 1024 graphs of N = 512) -- split a
        large batch of large graphs into several calls."""
        adj = self._adj("spectral_hist", adj)
        B, N = adj.shape[0], adj.shape[1]
        bins = int(bins)
        edges = self._hist_edges("spectral_hist", -1e-5, 2, bins, adj.device)
        res = {"spectral_hist": torch.empty((B, bins), dtype=torch.int32, device=adj.device)}
        if eig:
            res["spectral_eig"] = torch.empty((B, N), dtype=torch.float64, device=adj.device)
            res["spectral_n"] = torch.empty((B,), dtype=torch.int32, device=adj.device)
        nbytes = self.lib.ccsd_spectral_workspace_bytes(B, N)
        if nbytes == 0:
            self.lib.check(_lib.ERR_INVALID)
        ws = self._scratch(nbytes, adj.device)
        self.lib.check(self.lib.ccsd_spectral_hist(_ptr(adj), B, N, _adj_mode(mol), float(thr), _ptr(edges), bins, _ptr(res["spectral_hist"]),
                                                   _ptr(res.get("spectral_eig")), _ptr(res.get("spectral_n")), _ptr(ws), ws.numel() * 8,
                                                   self._stream()))
        return res

    def hodge_spectrum(self, adj: torch.Tensor, cell_bits: torch.Tensor, *, d_min: int, d_max: int, mol: bool = False, thr: float = 0.5,
                       sweeps: bool = False):
        """Eigenvalues of the hodge Laplacian F F^T per complex (ccsd_hodge_spectrum): hodge_laplacian_spectrum_worker of the reference
        (cc_utils.py:994-1060) on the complex cc_from_incidence builds from the quantised sample.  adj (B,N,N) float32 (finish()'s
        quantiser `mol`, `thr`), cell_bits (B, ceil(K/64)) int64 = finish()'s rank2_cell_bits for the cell sizes d_min..d_max.
        -> (B,E) float32, ascending, E = N (N - 1) / 2; exact zeros for a complex without a cell.  E > 512 raises NotImplementedError.
        sweeps=True also returns the solver's (B,) int32 sweep counts.  The call allocates its workspace, which holds every H:
        8 B E^2 bytes (296 MB for 1024 complexes at E = 190) -- split a large batch into several calls."""
        adj = self._adj("hodge_spectrum", adj)
        B, N = adj.shape[0], adj.shape[1]
        E = N * (N - 1) // 2
        d_min, d_max = int(d_min), int(d_max)
        if not 1 <= d_min <= d_max <= N:
            raise ValueError(f"hodge_spectrum: bad cell sizes d_min = {d_min}, d_max = {d_max} for N = {N}")
        K = sum(math.comb(N, d) for d in range(d_min, d_max + 1))
        if cell_bits.dtype != torch.int64 or cell_bits.device.type != self.device.type or tuple(cell_bits.shape) != (B, (K + 63) // 64):
            raise ValueError(f"hodge_spectrum: cell_bits must be int64 of shape ({B}, {(K + 63) // 64}) on {self.device}, "
                             f"got {cell_bits.dtype} {tuple(cell_bits.shape)} {cell_bits.device}")
        cell_bits = cell_bits.contiguous()
        nbytes = self.lib.ccsd_hodge_workspace_bytes(B, N)
        if nbytes == 0:
            self.lib.check(_lib.ERR_UNSUPPORTED if E > _lib.EIG_MAXN else _lib.ERR_INVALID)
        out = torch.empty((B, E), dtype=torch.float32, device=adj.device)
        sw = torch.empty((B,), dtype=torch.int32, device=adj.device)
        ws = self._scratch(nbytes, adj.device)
        self.lib.check(self.lib.ccsd_hodge_spectrum(_ptr(adj), _ptr(cell_bits), B, N, d_min, d_max, _adj_mode(mol), float(thr), _ptr(out),
                                                    _ptr(sw), _ptr(ws), ws.numel() * 8, self._stream()))
        return (out, sw) if sweeps else out

    def lift(self, adj: torch.Tensor, procedure: str, *, d_min: int, d_max: int, path_length: int = 3, sources=None, mol: bool = False,
             thr: float = 0.5, dense: bool = False) -> dict:
        """Graphs lifted to combinatorial complexes (ccsd_lift): the rank-2 cells convert_graphs_to_CCs of the reference (cc_utils.py:
        816-880) adds to the graphs of the quantised adjacency, finish()'s quantiser (`mol`, `thr`; in mol mode every bond order is a
        plain edge), in the form finish() writes.  adj (B,N,N) float32, N <= 64; pair (i, j), i < j, is read from row i, as
        hodge_spectrum reads it, and the diagonal is ignored.
          procedure "path_based"   path_based_lift_CC with path_length 3: {a, b, c} is a cell iff one of the three nodes is adjacent to
                                   the other two and one of those two is in `sources` (an iterable of node indices; None = every node,
                                   the reference's "basic" setting; empty = no cell).  Another path_length raises NotImplementedError.
          procedure "cycles"       cycles_lift_CC: the node sets of networkx.cycle_basis(networkx.from_numpy_array(A)).  The reference
                                   rebuilds the graph from frozenset edges first, so its walk follows CPython's set-slot order and finds
                                   another basis for about half of all random graphs; the number of cycles, E - V + C, is the same, and
                                   both sides of a score are lifted by the one rule here.
        -> rank2_cell_bits (B, ceil(K/64)) int64, rank2_cell_count (B,), rank2_cell_hist (B, d_max-d_min+1), rank2_nnz (B,) int32 as
        finish() gives them for the lifted complex's incidence tensor; lift_dropped (B,) int32: the basis cycles whose size lies outside
        d_min..d_max, which have no column (0 for paths); and rank2 (B, E, K) float32, the incidence tensor of create_incidence_1_2
        (chords of a cycle count), when `dense`.  Every output is written in full.  Nothing is synchronised.  N > 64 raises
        NotImplementedError."""
        adj = self._adj("lift", adj)
        B, N = adj.shape[0], adj.shape[1]
        procs = {"path_based": _lib.LIFT_PATHS, "cycles": _lib.LIFT_CYCLES}
        if procedure not in procs:
            raise ValueError(f"lift: procedure must be one of {sorted(procs)}, got {procedure!r}")
        d_min, d_max = int(d_min), int(d_max)
        mask = (1 << 64) - 1
        if sources is not None:
            mask = 0
            for n in sources:                                     # (a source that is no node of the graph starts no path, as in the reference)
                if not 0 <= int(n) < _lib.LIFT_MAX_NODES:
                    raise ValueError(f"lift: source node {n} outside 0..{_lib.LIFT_MAX_NODES - 1}")
                mask |= 1 << int(n)
        if B and not 2 <= N <= _lib.LIFT_MAX_NODES:               # (the C call names the limit; it launches nothing)
            self.lib.check(self.lib.ccsd_lift(_ptr(adj), B, N, _adj_mode(mol), float(thr), procs[procedure], int(path_length), mask, d_min, d_max,
                                              None, None, None, None, None, None, self._stream()))
        if not 1 <= d_min <= d_max <= N:
            raise ValueError(f"lift: bad cell sizes d_min = {d_min}, d_max = {d_max} for N = {N}")
        K = sum(math.comb(N, d) for d in range(d_min, d_max + 1))
        if K > 1 << 24:
            raise ValueError(f"lift: sum C(N, d) for d = {d_min}..{d_max} exceeds 2^24")
        dev = adj.device
        res = {"rank2_cell_bits": torch.empty((B, (K + 63) // 64), dtype=torch.int64, device=dev),
               "rank2_cell_count": torch.empty((B,), dtype=torch.int32, device=dev),
               "rank2_cell_hist": torch.empty((B, d_max - d_min + 1), dtype=torch.int32, device=dev),
               "rank2_nnz": torch.empty((B,), dtype=torch.int32, device=dev),
               "lift_dropped": torch.empty((B,), dtype=torch.int32, device=dev)}
        if dense:
            res["rank2"] = torch.empty((B, N * (N - 1) // 2, K), dtype=torch.float32, device=dev)
        self.lib.check(self.lib.ccsd_lift(_ptr(adj), B, N, _adj_mode(mol), float(thr), procs[procedure], int(path_length), mask, d_min, d_max,
                                          _ptr(res["rank2_cell_bits"]), _ptr(res["rank2_cell_count"]), _ptr(res["rank2_cell_hist"]),
                                          _ptr(res["rank2_nnz"]), _ptr(res["lift_dropped"]), _ptr(res.get("rank2")), self._stream()))
        return res

    def mol_correct(self, adj: torch.Tensor, labels: torch.Tensor, *, dataset: str = "QM9", max_valence=None, charge_base=None,
                    largest_fragment: bool = True) -> dict:
        """Molecule post-processing (ccsd_mol_correct): what gen_mol of the reference (utils/mol_utils.py:191-229) does to every sample
        of a molecule run before it is scored -- construct_mol's formal charges, correct_mol's lowering of over-valent bonds, the
        largest fragment of valid_mol_can_with_seg -- on integer bond orders, without rdkit.  adj (B,N,N) float32 raw samples,
        N <= 64, quantised with finish()'s molecule quantiser (bond orders 0..3); pair (i, j), i < j, is read from row i, as lift reads
        it.  labels (B,N) integer, as evaluation.mol_labels gives them: -1 = no atom (bonds to such a slot are ignored).  `dataset`
        names a row of evaluation.MOL_TABLES ("QM9", "ZINC250k"); max_valence (L,2) = [neutral, charge +1] and charge_base (L,)
        replace its tables (integers 0..255, L <= 16).
          mol_adj (B,N,N) uint8         symmetric bond orders, zero diagonal
          mol_labels (B,N) int32, mol_charge (B,N) int8     -1 / 0 for a slot without an atom; slots are not compacted
          mol_no_correct (B,) uint8     no atom was over-valent after construction (the reference's "validity w/o correction" counts these)
          mol_n_corrections (B,) int32  the decrements of correct_mol
          mol_n_fragments (B,) int32    connected components after correction, before selection
          mol_atoms (B,) int32          the atoms kept
        largest_fragment=True keeps the fragment with the most atoms (tie: the one holding the lowest slot) and drops every other
        atom -- the reference compares the lengths of the fragments' SMILES strings instead; False keeps every fragment, as the
        reference's largest_connected_comp=False.  Every output is written in full.  The call reads one flag back (a label >= L raises
        ValueError): it synchronises the stream once."""
        adj = self._adj("mol_correct", adj)
        B, N = adj.shape[0], adj.shape[1]
        if tuple(labels.shape) != (B, N) or labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.device.type != self.device.type:
            raise ValueError(f"mol_correct: labels must be integer of shape ({B}, {N}) on {self.device}, got {labels.dtype} {tuple(labels.shape)} {labels.device}")
        labels = labels.to(torch.int32).contiguous()
        if max_valence is None or charge_base is None:
            from .evaluation import MOL_TABLES

            if dataset not in MOL_TABLES:
                raise ValueError(f"mol_correct: dataset must be one of {sorted(MOL_TABLES)}, got {dataset!r}")
            max_valence = MOL_TABLES[dataset]["max_valence"] if max_valence is None else max_valence
            charge_base = MOL_TABLES[dataset]["charge_base"] if charge_base is None else charge_base
        tables = []
        for name, t in (("max_valence", max_valence), ("charge_base", charge_base)):
            t = np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t)
            if t.dtype.kind not in "iu":
                raise ValueError(f"mol_correct: {name} must hold integers, got {t.dtype}")
            tables.append(np.ascontiguousarray(t, dtype=np.int32))
        mv, cb = tables
        if mv.ndim != 2 or mv.shape[1] != 2 or cb.shape != (mv.shape[0],):
            raise ValueError(f"mol_correct: max_valence must be (L, 2) and charge_base (L,), got {mv.shape} and {cb.shape}")
        dev = adj.device
        shapes = {"mol_adj": ((B, N, N), torch.uint8), "mol_labels": ((B, N), torch.int32), "mol_charge": ((B, N), torch.int8),
                  "mol_no_correct": ((B,), torch.uint8), "mol_n_corrections": ((B,), torch.int32), "mol_n_fragments": ((B,), torch.int32),
                  "mol_atoms": ((B,), torch.int32)}
        res = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        dims = _lib.MolDims(B, N, mv.shape[0], int(bool(largest_fragment)))
        out = _lib.MolOut(*[_ptr(res[n]) for n in _lib.MOL_OUTPUTS])
        i32p = C.POINTER(C.c_int32)
        self.lib.check(self.lib.ccsd_mol_correct(C.byref(dims), _ptr(adj), _ptr(labels), mv.ctypes.data_as(i32p), cb.ctypes.data_as(i32p),
                                                 C.byref(out), self._stream()))
        return res


def cells_from_bits(bits_row, N: int, d_min: int, d_max: int):
    """Cell tuples of one complex from its bitmask row, in the reference's enumeration order (get_cells,
    cc_utils.py:72-94: itertools.combinations(range(N), d) for d = d_min..d_max)."""
    from itertools import combinations

    words = [int(w) & 0xFFFFFFFFFFFFFFFF for w in bits_row.tolist()]
    out, k = [], 0
    for d in range(d_min, d_max + 1):
        for combi in combinations(range(N), d):
            if (words[k >> 6] >> (k & 63)) & 1:
                out.append(combi)
            k += 1
    return out
