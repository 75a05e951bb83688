"""ctypes binding of libccsd_hip.so (include/ccsd_hip.h).

The product path has exactly one backend: the hand-written HIP library built in-tree by
`__graft_entry__.build()`.  If it is missing, or no MI355X is visible, everything that needs
compute raises -- there is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(HERE, "libccsd_hip.so")

ABI_VERSION = 5
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WEIGHTS, ERR_RUNTIME, ERR_WORKSPACE, ERR_CALLBACK = range(7)
SDE_VP, SDE_VE, SDE_SUBVP = 0, 1, 2
PRED_EULER, PRED_REVERSE, PRED_S4 = 0, 1, 2
CORR_NONE, CORR_LANGEVIN = 0, 1
TARGET_X, TARGET_ADJ, TARGET_RANK2 = 0, 1, 2

EXPORTS = [
    "ccsd_plan_create", "ccsd_plan_destroy", "ccsd_weight_count", "ccsd_rank2_dims", "ccsd_workspace_bytes",
    "ccsd_last_error", "ccsd_score", "ccsd_init_state", "ccsd_corrector_norms", "ccsd_corrector_apply",
    "ccsd_predictor", "ccsd_s4_apply", "ccsd_sampler_run", "ccsd_quantize", "ccsd_rank2_cells", "ccsd_profile_kernel", "ccsd_profile_stride", "ccsd_profile_read", "ccsd_profile_launches", "ccsd_debug_stamps",
    "ccsd_noise_draws", "ccsd_noise_draws_at", "ccsd_plan_query", "ccsd_sampler_run_ex", "ccsd_finish",
    "ccsd_cluster_hist", "ccsd_orbit_counts", "ccsd_mmd_workspace_bytes", "ccsd_mmd",
    "ccsd_eig_workspace_bytes", "ccsd_eigvalsh", "ccsd_spectral_workspace_bytes", "ccsd_spectral_hist",
    "ccsd_hodge_workspace_bytes", "ccsd_hodge_spectrum",
    "ccsd_nspdk_row_capacity", "ccsd_nspdk_workspace_bytes", "ccsd_nspdk_features", "ccsd_nspdk_mmd_workspace_bytes", "ccsd_nspdk_mmd",
    "ccsd_lift", "ccsd_mol_correct",
]
QUERIES = {"fused_r2": 0, "xa_variant": 1, "r2_lds_bytes": 2, "xa_lds_bytes": 3, "fused_loop": 4, "merged_r2": 5, "ew1": 6, "large_graph": 7,
           "r2_family": 8, "r2_instance": 9, "loop_form": 10, "h_full": 11, "hp_full": 12, "p0_narrow": 13, "tiled_fuse": 14, "ew1_fuse": 15,
           "h_general": 16, "geo_ek": 17, "h_wide": 18, "mlp_forms": 19, "fold_sums": 20, "fold_last_run": 21}
KERNEL_IDS = {"k_xa": 0, "k_gemm_p": 1, "k_hf_score": 2, "k_gemm_h": 3, "k_langevin_apply": 4, "k_r2": 5, "k_s4_apply": 6, "k_ew1": 7}


class StepCoef(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("sscale", "alpha", "pa", "pb", "pc", "m1", "s1", "d", "m2", "s2")]


class Config(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in (
            "abi_version", "N", "F", "is_cc", "d_min", "d_max",
            "x_depth", "x_nhid",
            "a_num_layers", "a_num_linears", "a_c_init", "a_c_hid", "a_c_final", "a_nhid", "a_adim", "a_num_heads",
            "a_is_cc_net", "h_num_layers", "h_num_linears", "h_nhid", "h_adim", "h_c_hid", "h_c_final", "h_num_heads",
            "f_num_layers", "f_num_linears", "f_nhid", "f_c_hid", "f_c_final", "f_cnum", "f_num_layers_mlp",
            "f_use_hodge_mask",
            "predictor", "corrector", "n_corr_steps", "probability_flow", "denoise")]
        + [("snr", C.c_float), ("scale_eps", C.c_float), ("diff_steps", C.c_int32), ("batch_hint", C.c_int32)]
        + [(n, C.c_int32) for n in ("x_gmh", "x_num_linears", "x_c_init", "x_c_hid", "x_c_final", "x_adim", "x_num_heads",
                                    "a_conv_mlp", "x_conv_mlp")]
    )


class State(C.Structure):
    _fields_ = [("x", C.c_void_p), ("adj", C.c_void_p), ("rank2", C.c_void_p)]


class Noise(C.Structure):
    _fields_ = [("zx", C.c_void_p), ("zadj", C.c_void_p), ("zrank2", C.c_void_p)]


FINISH_ADJ_QUANTIZE, FINISH_ADJ_MOL = 0, 1
MMD_EMD, MMD_TV, MMD_L2 = 0, 1, 2
MMD_INT32, MMD_FP64 = 0, 1
MMD_IS_HIST, MMD_DEGREE, MMD_F32_PMF = 1, 2, 4
CLUSTER_MAX_BINS, MMD_MAX_ROWS, MMD_MAX_BINS = 1024, 1 << 20, 1 << 16      # CCSD_CLUSTER_MAX_BINS, CCSD_MMD_MAX_ROWS, CCSD_MMD_MAX_BINS
ORBITS = 15                                                               # CCSD_ORBITS: ORCA's orbits of the graphlets on 2..4 nodes
NSPDK_MAX_NODES, NSPDK_FEATURES = 64, 65537                               # CCSD_NSPDK_MAX_NODES, CCSD_NSPDK_FEATURES
LIFT_PATHS, LIFT_CYCLES, LIFT_MAX_NODES = 0, 1, 64                         # CCSD_LIFT_PATHS, CCSD_LIFT_CYCLES; the node limit of ccsd_lift
MOL_MAX_ATOMS, MOL_MAX_LABELS = 64, 16                                    # CCSD_MOL_MAX_ATOMS, CCSD_MOL_MAX_LABELS
EIG_MAXN, EIG_MAX_SWEEPS = 512, 30                                        # CCSD_EIG_MAXN; the sweep cap of k_eigvalsh


class FinishDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("F", C.c_int32), ("E", C.c_int32), ("K", C.c_int64),
                ("d_min", C.c_int32), ("d_max", C.c_int32), ("adj_mode", C.c_int32), ("thr", C.c_float)]


FINISH_OUTPUTS = ("adj_int", "degree", "degree_hist", "edge_hist", "n_nodes", "x_hist", "rank2_u8", "rank2_cell_bits",
                  "rank2_cell_count", "rank2_cell_hist", "rank2_nnz")


class FinishOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FINISH_OUTPUTS]


class MolDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("L", C.c_int32), ("largest_fragment", C.c_int32)]


MOL_OUTPUTS = ("mol_adj", "mol_labels", "mol_charge", "mol_no_correct", "mol_n_corrections", "mol_n_fragments", "mol_atoms")


class MolOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MOL_OUTPUTS]


# ccsd_reduce_fn: int (*)(float* sums_dev, int32_t n, void* stream, void* user)
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)


class RunOptions(C.Structure):
    _fields_ = [("reduce", REDUCE_FN), ("user", C.c_void_p)]


class CcsdError(RuntimeError):
    pass


def raise_status(lib, status: int):
    """Map status codes onto the exception types the reference raises on this path."""
    if status == OK:
        return
    msg = lib.ccsd_last_error().decode("utf-8", "replace")
    if status == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if status in (ERR_INVALID, ERR_WEIGHTS, ERR_WORKSPACE):
        raise ValueError(msg)
    raise CcsdError(msg)


class Library:
    """A loaded C-ABI library with typed entry points."""

    def __init__(self, path: str, is_hip: bool):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = path
        self.is_hip = is_hip
        L = self.c = C.CDLL(path)
        vp, i32, i64, u64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_size_t
        P = C.POINTER
        L.ccsd_plan_create.argtypes = [P(Config), P(C.c_float), sz, P(StepCoef), P(vp)]
        L.ccsd_plan_create.restype = C.c_int
        L.ccsd_plan_destroy.argtypes = [vp]
        L.ccsd_plan_destroy.restype = None
        L.ccsd_weight_count.argtypes = [P(Config)]
        L.ccsd_weight_count.restype = sz
        L.ccsd_rank2_dims.argtypes = [P(Config), P(i32), P(i64)]
        L.ccsd_rank2_dims.restype = None
        L.ccsd_workspace_bytes.argtypes = [vp, i32]
        L.ccsd_workspace_bytes.restype = sz
        L.ccsd_last_error.argtypes = []
        L.ccsd_last_error.restype = C.c_char_p
        L.ccsd_score.argtypes = [vp, i32, i32, P(State), vp, f32, vp, vp, sz, vp]
        L.ccsd_score.restype = C.c_int
        L.ccsd_init_state.argtypes = [vp, i32, vp, P(Noise), u64, i64, P(State), vp]
        L.ccsd_init_state.restype = C.c_int
        L.ccsd_corrector_norms.argtypes = [vp, i32, i32, i32, P(State), P(State), vp, P(Noise), u64, i64, vp, vp, sz, vp]
        L.ccsd_corrector_norms.restype = C.c_int
        L.ccsd_corrector_apply.argtypes = [vp, i32, i32, i32, P(State), vp, P(Noise), u64, i64, vp, P(State), vp, sz, vp]
        L.ccsd_corrector_apply.restype = C.c_int
        L.ccsd_predictor.argtypes = [vp, i32, i32, P(State), vp, P(Noise), u64, i64, P(State), P(State), vp, sz, vp]
        L.ccsd_predictor.restype = C.c_int
        L.ccsd_s4_apply.argtypes = [vp, i32, i32, P(State), vp, P(Noise), P(Noise), P(Noise), u64, i64, vp, P(State), P(State), vp, sz, vp]
        L.ccsd_s4_apply.restype = C.c_int
        L.ccsd_sampler_run.argtypes = [vp, i32, vp, u64, i64, i32, i32, P(State), P(State), P(State), vp, vp, sz, vp]
        L.ccsd_sampler_run.restype = C.c_int
        L.ccsd_sampler_run_ex.argtypes = L.ccsd_sampler_run.argtypes + [P(RunOptions)]
        L.ccsd_sampler_run_ex.restype = C.c_int
        L.ccsd_quantize.argtypes = [vp, i64, f32, vp, vp]
        L.ccsd_quantize.restype = C.c_int
        L.ccsd_rank2_cells.argtypes = [vp, i32, i32, i64, f32, vp, vp, vp]
        L.ccsd_rank2_cells.restype = C.c_int
        L.ccsd_profile_kernel.argtypes = [vp, i32]
        L.ccsd_profile_kernel.restype = C.c_int
        L.ccsd_profile_stride.argtypes = [vp, i32]
        L.ccsd_profile_stride.restype = C.c_int
        L.ccsd_profile_read.argtypes = [vp, i32, P(i64), P(C.c_double)]
        L.ccsd_profile_read.restype = C.c_int
        L.ccsd_profile_launches.argtypes = [vp, i32, P(i64)]
        L.ccsd_profile_launches.restype = C.c_int
        L.ccsd_debug_stamps.argtypes = [vp, vp]
        L.ccsd_debug_stamps.restype = C.c_int
        L.ccsd_noise_draws.argtypes = [vp, i32, vp, u64, i64, i32, i32, P(State), vp]
        L.ccsd_noise_draws.restype = C.c_int
        L.ccsd_noise_draws_at.argtypes = [vp, i32, vp, u64, i64, C.c_uint32, i32, P(State), vp]
        L.ccsd_noise_draws_at.restype = C.c_int
        L.ccsd_plan_query.argtypes = [vp, i32, P(i64)]
        L.ccsd_plan_query.restype = C.c_int
        L.ccsd_finish.argtypes = [P(FinishDims), P(State), vp, P(FinishOut), vp]
        L.ccsd_finish.restype = C.c_int
        L.ccsd_cluster_hist.argtypes = [vp, i32, i32, i32, f32, vp, i32, vp, vp, vp]
        L.ccsd_cluster_hist.restype = C.c_int
        L.ccsd_orbit_counts.argtypes = [vp, i32, i32, i32, f32, vp, vp, vp, vp]
        L.ccsd_orbit_counts.restype = C.c_int
        L.ccsd_mmd_workspace_bytes.argtypes = [i32, i32, i32]
        L.ccsd_mmd_workspace_bytes.restype = sz
        L.ccsd_mmd.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, C.c_double, C.c_double, vp, sz, vp, vp]
        L.ccsd_mmd.restype = C.c_int
        L.ccsd_eig_workspace_bytes.argtypes = [i32, i32]
        L.ccsd_eig_workspace_bytes.restype = sz
        L.ccsd_eigvalsh.argtypes = [vp, i32, i32, vp, vp, vp, sz, vp]
        L.ccsd_eigvalsh.restype = C.c_int
        L.ccsd_spectral_workspace_bytes.argtypes = [i32, i32]
        L.ccsd_spectral_workspace_bytes.restype = sz
        L.ccsd_spectral_hist.argtypes = [vp, i32, i32, i32, f32, vp, i32, vp, vp, vp, vp, sz, vp]
        L.ccsd_spectral_hist.restype = C.c_int
        L.ccsd_hodge_workspace_bytes.argtypes = [i32, i32]
        L.ccsd_hodge_workspace_bytes.restype = sz
        L.ccsd_hodge_spectrum.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, sz, vp]
        L.ccsd_hodge_spectrum.restype = C.c_int
        L.ccsd_nspdk_row_capacity.argtypes = [i32]
        L.ccsd_nspdk_row_capacity.restype = i32
        L.ccsd_nspdk_workspace_bytes.argtypes = [i32, i32]
        L.ccsd_nspdk_workspace_bytes.restype = sz
        L.ccsd_nspdk_features.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]
        L.ccsd_nspdk_features.restype = C.c_int
        L.ccsd_nspdk_mmd_workspace_bytes.argtypes = [i32, i32]
        L.ccsd_nspdk_mmd_workspace_bytes.restype = sz
        L.ccsd_nspdk_mmd.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, sz, vp, vp]
        L.ccsd_nspdk_mmd.restype = C.c_int
        L.ccsd_lift.argtypes = [vp, i32, i32, i32, f32, i32, i32, u64, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.ccsd_lift.restype = C.c_int
        L.ccsd_mol_correct.argtypes = [P(MolDims), vp, vp, P(i32), P(i32), P(MolOut), vp]
        L.ccsd_mol_correct.restype = C.c_int

    def __getattr__(self, name):
        return getattr(self.c, name)

    def check(self, status: int):
        raise_status(self.c, status)


_hip: Optional[Library] = None


def get_library() -> Library:
    """The HIP library.  Fails loudly when it has not been built (python __graft_entry__.py).
    CCSD_LIB_PATH (developer A/B runs only, tools/dev/*.sh) names another build of the SAME HIP library -- e.g. a diagnostic build with
    cycle stamps -- instead of overwriting the product file; it is still a HIP library (is_hip: a GPU is required) and a missing
    file is an error, never a fallback."""
    global _hip
    if _hip is None:
        # torch first: its bundled HIP runtime (libamdhip64) must be the one in the process before libccsd_hip.so asks for that SONAME --
        # loaded the other way round (library, then torch) the two copies do not share their device state and the library's first
        # hipMalloc reports "no ROCm-capable device is detected" (seen with __graft_entry__.build() called ahead of any torch import)
        import torch  # noqa: F401

        path = os.environ.get("CCSD_LIB_PATH") or HIP_LIB_PATH
        if not os.path.exists(path):
            raise CcsdError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  ccsd_amd has no CPU fallback."
            )
        _hip = Library(path, is_hip=True)
    return _hip
