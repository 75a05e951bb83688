"""PCEngine: owns a ccsd_plan_t and drives the C ABI with torch tensors as device memory.

PyTorch is plumbing here (allocations, streams, RCCL): every score evaluation, mask, noise draw
and state update is done by the HIP kernels behind include/ccsd_hip.h.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, plan as _plan
from .sde import SDE, step_coefficients


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class PCEngine:
    def __init__(self, params_x: Optional[dict], sd_x, params_adj: Optional[dict], sd_adj, params_rank2: Optional[dict],
                 sd_rank2, *, N: int, F: int, is_cc: bool, d_min: int = 0, d_max: int = 0,
                 sdes: Optional[Sequence[SDE]] = None, predictor: str = "Euler", corrector: str = "None",
                 snr: float = 0.1, scale_eps: float = 1.0, n_steps: int = 1, probability_flow: bool = False,
                 denoise: bool = True, eps: float = 1e-3, device="cuda", lib: Optional[_lib.Library] = None,
                 batch_hint: int = 0):
        self.lib = lib if lib is not None else _lib.get_library()
        self.device = torch.device(device)
        if self.lib.is_hip:
            if self.device.type != "cuda":
                raise _lib.CcsdError("the HIP library needs a cuda (ROCm) device; ccsd_amd has no CPU path")
            if not torch.cuda.is_available():
                raise _lib.CcsdError("no MI355X visible: ccsd_amd has no CPU fallback")
        px, pa, pf = _plan.complete_params(params_x, params_adj, params_rank2 if is_cc else None, N, F, is_cc, d_min, d_max)
        self.is_cc, self.N, self.F = is_cc, N, F
        self.E, self.K = _plan.rank2_dim(N, d_min, d_max) if is_cc else (N * (N - 1) // 2, 0)
        if sdes is not None:
            coef = step_coefficients(list(sdes), predictor, probability_flow, eps)
            if not is_cc:
                coef[:, 2] = coef[:, 1]
            self.diff_steps = sdes[1].N
        else:
            coef = np.zeros((1, 3, 10), np.float32)
            coef[:, :, 0] = 1.0
            self.diff_steps = 1
        self.coef = np.ascontiguousarray(coef, np.float32)
        self.n_steps, self.corrector, self.denoise = n_steps, corrector, denoise
        cfg = _plan.make_config(px, pa, pf, predictor=predictor, corrector=corrector, snr=snr, scale_eps=scale_eps,
                                n_steps=n_steps, probability_flow=probability_flow, denoise=denoise,
                                diff_steps=self.diff_steps, batch_hint=batch_hint)
        blob = _plan.pack_weights(px, sd_x if params_x is not None else None, pa, sd_adj if params_adj is not None else None,
                                  pf, sd_rank2 if (is_cc and params_rank2 is not None) else None)
        self.cfg = cfg
        handle = C.c_void_p()
        with torch.cuda.device(self.device) if self.lib.is_hip else _Null():
            st = self.lib.ccsd_plan_create(C.byref(cfg), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size,
                                           self.coef.ctypes.data_as(C.POINTER(_lib.StepCoef)), C.byref(handle))
        self.lib.check(st)
        self.handle = handle
        self._ws: Optional[torch.Tensor] = None
        self._ws_B = 0
        self._edges: dict = {}          # (bins, device) -> np.linspace(0, 1, bins + 1) on the device (cluster_hist); ("spectral", bins, device) -> spectral_hist's

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                self.lib.ccsd_plan_destroy(h)
            except Exception:
                pass
            self.handle = None

    # -- helpers
    def _stream(self):
        if self.lib.is_hip:
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def _workspace(self, B: int) -> Tuple[C.c_void_p, int]:
        n = self.lib.ccsd_workspace_bytes(self.handle, B)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._ws.data_ptr()), self._ws.numel()

    def _check(self, t: Optional[torch.Tensor], shape, name):
        if t is None:
            return
        if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != self.device.type:
            raise ValueError(f"{name}: expected contiguous float32 {tuple(shape)} on {self.device}, got {tuple(t.shape)} {t.dtype} {t.device}")

    def shapes(self, B: int):
        return (B, self.N, self.F), (B, self.N, self.N), (B, self.E, self.K)

    def _state(self, x, adj, rank2, B, name="state") -> _lib.State:
        sx, sa, sr = self.shapes(B)
        self._check(x, sx, name + ".x")
        self._check(adj, sa, name + ".adj")
        if self.is_cc:
            if rank2 is None:
                raise ValueError(f"{name}.rank2 is required for combinatorial complexes")
            self._check(rank2, sr, name + ".rank2")
        return _lib.State(_ptr(x), _ptr(adj), _ptr(rank2) if self.is_cc else None)

    def _noise(self, z: Optional[Sequence[Optional[torch.Tensor]]], B: int):
        if z is None:
            return None
        sx, sa, sr = self.shapes(B)
        self._check(z[0], sx, "noise.x")
        self._check(z[1], sa, "noise.adj")
        if self.is_cc:
            self._check(z[2], sr, "noise.rank2")
        return C.byref(_lib.Noise(_ptr(z[0]), _ptr(z[1]), _ptr(z[2]) if self.is_cc and len(z) > 2 else None))

    def alloc_state(self, B: int) -> List[Optional[torch.Tensor]]:
        sx, sa, sr = self.shapes(B)
        out = [torch.empty(sx, device=self.device), torch.empty(sa, device=self.device)]
        out.append(torch.empty(sr, device=self.device) if self.is_cc else None)
        return out

    # -- API
    def score(self, target: int, x, adj, rank2, flags, sscale: float = 1.0) -> torch.Tensor:
        B = x.shape[0]
        st = self._state(x, adj, rank2, B)
        self._check(flags, (B, self.N), "flags")
        out = torch.empty(self.shapes(B)[target], device=self.device)
        ws, n = self._workspace(B)
        self.lib.check(self.lib.ccsd_score(self.handle, target, B, C.byref(st), _ptr(flags), float(sscale), _ptr(out), ws, n,
                                           self._stream()))
        return out

    def init_state(self, flags, state, prior=None, seed: int = 0, sample_offset: int = 0):
        B = flags.shape[0]
        st = self._state(*state, B)
        self.lib.check(self.lib.ccsd_init_state(self.handle, B, _ptr(flags), self._noise(prior, B), seed, sample_offset,
                                                C.byref(st), self._stream()))

    def noise_draws(self, flags, step: int, phase: int, out, seed: int = 0, sample_offset: int = 0):
        """The masked Philox noise of half-step (step, phase) as the kernels consume it (ccsd_noise_draws): phase 0..n_steps-1
        = corrector inner iterations, n_steps = predictor; S4: 0, 1, 2.  `out` = [x, adj, rank2] tensors of the state's shapes."""
        B = flags.shape[0]
        so = self._state(*out, B, "out")
        self.lib.check(self.lib.ccsd_noise_draws(self.handle, B, _ptr(flags), seed, sample_offset, int(step), int(phase),
                                                 C.byref(so), self._stream()))

    def query(self, what: str) -> int:
        """Which kernels the plan selected (ccsd_plan_query): "fused_r2", "xa_variant", "r2_lds_bytes", "xa_lds_bytes", "fused_loop", "merged_r2", "ew1", "large_graph";
        the rest of the route: "r2_family", "r2_instance", "loop_form", "tiled_fuse", "ew1_fuse", "h_general", "geo_ek", "p0_narrow" and, for the
        plan's batch_hint, "h_full", "hp_full" (include/ccsd_hip.h: CCSD_QUERY_*)."""
        v = C.c_int64(0)
        self.lib.check(self.lib.ccsd_plan_query(self.handle, _lib.QUERIES[what], C.byref(v)))
        return v.value

    def corrector_norms(self, step, it, base, cur, flags, noise, seed, sample_offset, sums):
        B = flags.shape[0]
        sb, sc = self._state(*base, B, "base"), self._state(*cur, B, "cur")
        ws, n = self._workspace(B)
        self.lib.check(self.lib.ccsd_corrector_norms(self.handle, B, step, it, C.byref(sb), C.byref(sc), _ptr(flags),
                                                     self._noise(noise, B), seed, sample_offset, _ptr(sums), ws, n,
                                                     self._stream()))

    def corrector_apply(self, step, it, cur, flags, noise, seed, sample_offset, sums, out):
        B = flags.shape[0]
        sc, so = self._state(*cur, B, "cur"), self._state(*out, B, "out")
        ws, n = self._workspace(B)
        self.lib.check(self.lib.ccsd_corrector_apply(self.handle, B, step, it, C.byref(sc), _ptr(flags),
                                                     self._noise(noise, B), seed, sample_offset, _ptr(sums), C.byref(so),
                                                     ws, n, self._stream()))

    def predictor(self, step, inp, flags, noise, seed, sample_offset, out, mean=None):
        B = flags.shape[0]
        si, so = self._state(*inp, B, "in"), self._state(*out, B, "out")
        sm = C.byref(self._state(*mean, B, "mean")) if mean is not None else None
        ws, n = self._workspace(B)
        self.lib.check(self.lib.ccsd_predictor(self.handle, B, step, C.byref(si), _ptr(flags), self._noise(noise, B), seed,
                                               sample_offset, C.byref(so), sm, ws, n, self._stream()))

    def s4_apply(self, step, cur, flags, noise1, noise2, noise3, seed, sample_offset, sums, out, mean=None):
        """Update half of one S4_solver step; corrector_norms(step, 0, cur, cur, ...) must have filled `sums`."""
        B = flags.shape[0]
        sc, so = self._state(*cur, B, "cur"), self._state(*out, B, "out")
        sm = C.byref(self._state(*mean, B, "mean")) if mean is not None else None
        ws, n = self._workspace(B)
        self.lib.check(self.lib.ccsd_s4_apply(self.handle, B, step, C.byref(sc), _ptr(flags), self._noise(noise1, B),
                                              self._noise(noise2, B), self._noise(noise3, B), seed, sample_offset,
                                              _ptr(sums), C.byref(so), sm, ws, n, self._stream()))

    def _reduce_options(self, reduce):
        """ccsd_run_options_t around a Python `reduce(sums)` callable -> (options or None, keep-alive objects, error cell).  The
        hook hands `reduce` a float32 view of the six norm sums inside the engine's own workspace tensor (a slice of self._ws: no
        copy, the all-reduce lands where the kernels read).  An exception raised by `reduce` is kept in the cell and turned into a
        non-zero return: the C loop stops, and the caller re-raises it once the C call is back."""
        if reduce is None:
            return None, None, None
        ws, err = self._ws, []

        def hook(sums_dev, n, stream, user):
            try:
                off = sums_dev - ws.data_ptr()
                if off < 0 or off + 4 * n > ws.numel():
                    raise _lib.CcsdError("reduce hook: the norm sums lie outside the engine's workspace")
                reduce(ws[off:off + 4 * n].view(torch.float32))
                return 0
            except BaseException as e:      # (nothing may propagate into the C frame)
                err.append(e)
                return 1

        cb = _lib.REDUCE_FN(hook)
        opts = _lib.RunOptions(cb, None)
        return opts, (cb, opts, hook), err

    def run(self, flags, state, scratch, result, seed: int = 0, sample_offset: int = 0, first_step: int = 0,
            last_step: Optional[int] = None, traj: Optional[torch.Tensor] = None, reduce=None):
        """The library loop (ccsd_sampler_run; ccsd_sampler_run_ex when `reduce` is given).  PRECONDITION: `state` is MASKED by
        `flags` -- x rows, adj rows / columns and rank2 rows / columns of switched-off nodes hold zeros, as in everything init_state
        or an earlier run wrote; the loop's rank-2 kernels skip re-masking rank2 (include/ccsd_hip.h).
        reduce: callable taking the six Langevin norm sums as a float32 device tensor of 6 elements, called once per norms pass
        (every Langevin inner iteration, every S4 step); it reduces them IN PLACE, ordered on the current stream
        (torch.distributed.all_reduce does).  An exception it raises stops the loop and is re-raised here; the state buffers
        are then undefined."""
        B = flags.shape[0]
        s, sc, r = self._state(*state, B), self._state(*scratch, B, "scratch"), self._state(*result, B, "result")
        ws, n = self._workspace(B)
        last = self.diff_steps if last_step is None else last_step
        opts, keep, err = self._reduce_options(reduce)
        if opts is None:
            rc = self.lib.ccsd_sampler_run(self.handle, B, _ptr(flags), seed, sample_offset, first_step, last,
                                           C.byref(s), C.byref(sc), C.byref(r), _ptr(traj), ws, n, self._stream())
        else:
            rc = self.lib.ccsd_sampler_run_ex(self.handle, B, _ptr(flags), seed, sample_offset, first_step, last,
                                              C.byref(s), C.byref(sc), C.byref(r), _ptr(traj), ws, n, self._stream(), C.byref(opts))
            del keep                        # (the callback object lived through the call)
            if err:
                raise err[0]
        self.lib.check(rc)

    def init_and_run(self, flags, state, scratch, result, seed: int = 0, sample_offset: int = 0, first_step: int = 0,
                     last_step: Optional[int] = None, traj: Optional[torch.Tensor] = None, reduce=None):
        """init_state (in-kernel Philox prior) followed by run, with every argument of both calls prepared BEFORE the first one is
        issued: the two C calls go out back to back, so the GPU is not left idle between the prior draw and the loop's first
        launches while Python checks shapes and builds structs (a 20-step call is ~5 ms: ~25 us of that gap is 0.5 %).
        init_state writes a masked prior, which is the masked-state PRECONDITION of run (see there); `reduce`: as in run."""
        B = flags.shape[0]
        s, sc, r = self._state(*state, B), self._state(*scratch, B, "scratch"), self._state(*result, B, "result")
        ws, n = self._workspace(B)
        last = self.diff_steps if last_step is None else last_step
        fp, tp, stream, lib, h = _ptr(flags), _ptr(traj), self._stream(), self.lib, self.handle
        opts, keep, err = self._reduce_options(reduce)
        rc0 = lib.ccsd_init_state(h, B, fp, None, seed, sample_offset, C.byref(s), stream)
        if rc0 != 0:
            rc1 = 0
        elif opts is None:
            rc1 = lib.ccsd_sampler_run(h, B, fp, seed, sample_offset, first_step, last, C.byref(s), C.byref(sc), C.byref(r), tp, ws, n, stream)
        else:
            rc1 = lib.ccsd_sampler_run_ex(h, B, fp, seed, sample_offset, first_step, last, C.byref(s), C.byref(sc), C.byref(r), tp, ws, n, stream,
                                          C.byref(opts))
            del keep
        lib.check(rc0)
        if err:
            raise err[0]
        lib.check(rc1)

    def profile_kernel(self, name: Optional[str]):
        """Add a kernel to the set timed with HIP events on the launch stream (None clears the set)."""
        self.lib.check(self.lib.ccsd_profile_kernel(self.handle, -1 if name is None else _lib.KERNEL_IDS[name]))

    def profile_stride(self, stride: int):
        """Bracket only every `stride`-th launch of the selected kernels with events."""
        self.lib.check(self.lib.ccsd_profile_stride(self.handle, int(stride)))

    def profile_read(self, name: str) -> Tuple[int, float]:
        n, ms = C.c_int64(0), C.c_double(0.0)
        self.lib.check(self.lib.ccsd_profile_read(self.handle, _lib.KERNEL_IDS[name], C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_launches(self, name: str) -> int:
        """All launches of a selected kernel since the selection / stride was set (bracketed by events or not)."""
        n = C.c_int64(0)
        self.lib.check(self.lib.ccsd_profile_launches(self.handle, _lib.KERNEL_IDS[name], C.byref(n)))
        return n.value

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
        dims = _lib.FinishDims(B, N, F, E, K, int(d_min), int(d_max), _lib.FINISH_ADJ_MOL if mol else _lib.FINISH_ADJ_QUANTIZE, float(thr))
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
        if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
            raise ValueError(f"cluster_hist: adj must be (B, N, N), got {tuple(adj.shape)}")
        if adj.dtype != torch.float32 or adj.device.type != self.device.type:
            raise ValueError(f"cluster_hist: adj must be float32 on {self.device}, got {adj.dtype} {adj.device}")
        adj = adj.contiguous()
        B, N = adj.shape[0], adj.shape[1]
        bins = int(bins)
        if not 1 <= bins <= _lib.CLUSTER_MAX_BINS:
            raise ValueError(f"cluster_hist: bins = {bins} outside 1..{_lib.CLUSTER_MAX_BINS}")
        key = (bins, adj.device)
        if key not in self._edges:
            self._edges[key] = torch.from_numpy(np.linspace(0.0, 1.0, bins + 1)).to(adj.device)
        edges = self._edges[key]
        res = {"cluster_hist": torch.empty((B, bins), dtype=torch.int32, device=adj.device)}
        if tri2:
            res["tri2"] = torch.empty((B, N), dtype=torch.int32, device=adj.device)
        self.lib.check(self.lib.ccsd_cluster_hist(_ptr(adj), B, N, _lib.FINISH_ADJ_MOL if mol else _lib.FINISH_ADJ_QUANTIZE, float(thr),
                                                  _ptr(edges), bins, _ptr(res.get("tri2")), _ptr(res["cluster_hist"]), self._stream()))
        return res

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
        lens1 = None if lens1 is None else lens1.contiguous()
        lens2 = None if lens2 is None else lens2.contiguous()
        n1, n2, L = s1.shape[0], s2.shape[0], s1.shape[1]
        out = torch.empty(4, dtype=torch.float64, device=s1.device)
        nbytes = self.lib.ccsd_mmd_workspace_bytes(n1, n2, L)
        ws = torch.empty(max(nbytes, 8) // 8 + 1, dtype=torch.float64, device=s1.device)        # (8-byte aligned)
        flags = (_lib.MMD_IS_HIST if is_hist else 0) | (_lib.MMD_DEGREE if degree else 0) | (_lib.MMD_F32_PMF if f32_pmf else 0)
        self.lib.check(self.lib.ccsd_mmd(_ptr(s1), n1, _ptr(lens1), _ptr(s2), n2, _ptr(lens2), L,
                                         _lib.MMD_FP64 if s1.dtype == torch.float64 else _lib.MMD_INT32, kinds[kind], flags, float(sigma),
                                         float(distance_scaling), _ptr(ws), ws.numel() * 8, _ptr(out), self._stream()))
        return out

    def _scratch(self, nbytes: int, device) -> torch.Tensor:
        return torch.empty(max(int(nbytes), 8) // 8 + 1, dtype=torch.float64, device=device)        # (8-byte aligned)

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
            nbytes = self.lib.ccsd_eig_workspace_bytes(B, min(n, _lib.EIG_MAXN))
            ws = self._scratch(nbytes, a.device)
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
        if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
            raise ValueError(f"spectral_hist: adj must be (B, N, N), got {tuple(adj.shape)}")
        if adj.dtype != torch.float32 or adj.device.type != self.device.type:
            raise ValueError(f"spectral_hist: adj must be float32 on {self.device}, got {adj.dtype} {adj.device}")
        adj = adj.contiguous()
        B, N = adj.shape[0], adj.shape[1]
        bins = int(bins)
        if not 1 <= bins <= _lib.CLUSTER_MAX_BINS:
            raise ValueError(f"spectral_hist: bins = {bins} outside 1..{_lib.CLUSTER_MAX_BINS}")
        key = ("spectral", bins, adj.device)
        if key not in self._edges:
            self._edges[key] = torch.from_numpy(np.linspace(-1e-5, 2, bins + 1)).to(adj.device)
        edges = self._edges[key]
        res = {"spectral_hist": torch.empty((B, bins), dtype=torch.int32, device=adj.device)}
        if eig:
            res["spectral_eig"] = torch.empty((B, N), dtype=torch.float64, device=adj.device)
            res["spectral_n"] = torch.empty((B,), dtype=torch.int32, device=adj.device)
        nbytes = self.lib.ccsd_spectral_workspace_bytes(B, N)
        if nbytes == 0:
            self.lib.check(_lib.ERR_INVALID)
        ws = self._scratch(nbytes, adj.device)
        self.lib.check(self.lib.ccsd_spectral_hist(_ptr(adj), B, N, _lib.FINISH_ADJ_MOL if mol else _lib.FINISH_ADJ_QUANTIZE, float(thr),
                                                   _ptr(edges), bins, _ptr(res["spectral_hist"]), _ptr(res.get("spectral_eig")),
                                                   _ptr(res.get("spectral_n")), _ptr(ws), ws.numel() * 8, self._stream()))
        return res

    def hodge_spectrum(self, adj: torch.Tensor, cell_bits: torch.Tensor, *, d_min: int, d_max: int, mol: bool = False, thr: float = 0.5,
                       sweeps: bool = False):
        """Eigenvalues of the hodge Laplacian F F^T per complex (ccsd_hodge_spectrum): hodge_laplacian_spectrum_worker of the reference
        (cc_utils.py:994-1060) on the complex cc_from_incidence builds from the quantised sample.  adj (B,N,N) float32 (finish()'s
        quantiser `mol`, `thr`), cell_bits (B, ceil(K/64)) int64 = finish()'s rank2_cell_bits for the cell sizes d_min..d_max.
        -> (B,E) float32, ascending, E = N (N - 1) / 2; exact zeros for a complex without a cell.  E > 512 raises NotImplementedError.
        sweeps=True also returns the solver's (B,) int32 sweep counts.  The call allocates its workspace, which holds every H:
        8 B E^2 bytes (296 MB for 1024 complexes at E = 190) -- split a large batch into several calls."""
        if adj.dim() != 3 or adj.shape[1] != adj.shape[2]:
            raise ValueError(f"hodge_spectrum: adj must be (B, N, N), got {tuple(adj.shape)}")
        if adj.dtype != torch.float32 or adj.device.type != self.device.type:
            raise ValueError(f"hodge_spectrum: adj must be float32 on {self.device}, got {adj.dtype} {adj.device}")
        adj = adj.contiguous()
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
        self.lib.check(self.lib.ccsd_hodge_spectrum(_ptr(adj), _ptr(cell_bits), B, N, d_min, d_max,
                                                    _lib.FINISH_ADJ_MOL if mol else _lib.FINISH_ADJ_QUANTIZE, float(thr), _ptr(out), _ptr(sw),
                                                    _ptr(ws), ws.numel() * 8, self._stream()))
        return (out, sw) if sweeps else out


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


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
