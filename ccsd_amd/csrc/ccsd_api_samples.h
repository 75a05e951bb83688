// ccsd_api_samples.h -- host side of the PLAN-FREE entry points of include/ccsd_hip.h: the operations on finished samples, which take
// tensors and sizes and never a ccsd_plan_t (ccsd_quantize, ccsd_rank2_cells, ccsd_finish, ccsd_cluster_hist, ccsd_orbit_counts, ccsd_nspdk_features, ccsd_nspdk_mmd, ccsd_mmd, ccsd_eigvalsh,
// ccsd_spectral_hist, ccsd_hodge_spectrum, ccsd_lift, ccsd_mol_correct and their *_workspace_bytes).  Included by ccsd_api.h as its last line; of what stands above it
// there, this file uses set_err, grid_for, RT_CHECK and LAUNCH_CHECK only.
//
// One definition per rule: check_batch (B, N, the quantiser), check_hist (bins, edges), check_scratch (workspace), no_bytes, quant_thr,
// cell_count.
// Every check of an entry point comes before its first launch.
#pragma once

// ---------------- the shared argument rules ----------------
// B >= 1, the quantiser of ccsd_finish (adj_mode, thr) and -- fin_n -- the node count of the graphs ccsd_finish takes
static int check_batch(const char* who, int B, int N, int adj_mode, float thr, bool fin_n = true) {
    const std::string w = std::string(who) + ": ";
    if (B < 1) return set_err(CCSD_ERR_INVALID, w + "B must be >= 1");
    if (fin_n && (N < 2 || N > CCSD_FIN_MAXN)) return set_err(CCSD_ERR_INVALID, w + "N = " + std::to_string(N) + " outside 2.." + std::to_string(CCSD_FIN_MAXN));
    if (adj_mode != CCSD_FINISH_ADJ_QUANTIZE && adj_mode != CCSD_FINISH_ADJ_MOL) return set_err(CCSD_ERR_INVALID, w + "unknown adj_mode");
    if (!(thr >= 0.f)) return set_err(CCSD_ERR_INVALID, w + "thr must be >= 0");
    return CCSD_OK;
}
// the histogram of k_cluster_hist / k_eigvalsh's epilogue: bins + 1 edges on the device (the limit is the public header's)
static_assert(CCSD_CLUSTER_MAX_BINS == CCSD_EVAL_MAXBINS, "the header's bin limit is k_cluster_hist's LDS histogram");
static int check_hist(const char* who, const double* edges, int bins) {
    if (bins < 1 || bins > CCSD_CLUSTER_MAX_BINS)
        return set_err(CCSD_ERR_INVALID, std::string(who) + ": bins = " + std::to_string(bins) + " outside 1.." + std::to_string(CCSD_CLUSTER_MAX_BINS));
    if (!edges) return set_err(CCSD_ERR_INVALID, std::string(who) + ": NULL edges");
    return CCSD_OK;
}
// a caller's scratch of `need` bytes (need = 0: none is read)
static int check_scratch(const char* who, const void* workspace, size_t ws_bytes, size_t need) {
    if (!need) return CCSD_OK;
    if (!workspace || ws_bytes < need) return set_err(CCSD_ERR_WORKSPACE, std::string(who) + ": workspace too small");
    if ((uintptr_t)workspace & 7) return set_err(CCSD_ERR_INVALID, std::string(who) + ": workspace must be 8-byte aligned");
    return CCSD_OK;
}
// a *_workspace_bytes function refuses its sizes: the reason is left for ccsd_last_error, the size is 0
static size_t no_bytes(int st, const std::string& m) { set_err(st, m); return 0; }
// the threshold argument of the quantising kernels: negative selects quantize_mol's 0/1/2/3 bins
static float quant_thr(int adj_mode, float thr) { return adj_mode == CCSD_FINISH_ADJ_MOL ? -1.0f : thr; }
// K = sum C(N, d) over d = d_min..d_max, the number of candidate cells, or -1 above 2^24 (the limit of ccsd_finish); `end`: the running
// sum per size (FinishTab::end)
static int64_t cell_count(int N, int d_min, int d_max, int* end = nullptr) {
    int64_t K = 0;
    for (int s = d_min; s <= d_max; ++s) {
        K += ccsd_comb(N, s);
        if (K > (1 << 24)) return -1;
        if (end) end[s - d_min] = (int)K;
    }
    return K;
}

// ---------------- quantised outputs and descriptors (ccsd_k_update.h, ccsd_k_finish.h) ----------------
extern "C" int ccsd_quantize(const float* in, int64_t n, float thr, int64_t* out, void* stream) {
    if (!in || !out || n < 0) return set_err(CCSD_ERR_INVALID, "bad argument");
    if (n == 0) return CCSD_OK;
    CCSD_LAUNCH(k_quantize, dim3(grid_for(n, 256)), dim3(CCSD_NTHREADS), 0, stream, in, (long long)n, thr, (long long*)out);
    LAUNCH_CHECK();
    return CCSD_OK;
}

extern "C" int ccsd_rank2_cells(const float* rank2, int32_t B, int32_t E, int64_t K, float thr, uint64_t* bits, int32_t* counts,
                                void* stream) {
    if (!rank2 || !bits || !counts || B < 1 || E < 1 || K < 1 || K > (1 << 24)) return set_err(CCSD_ERR_INVALID, "bad argument");
    CCSD_LAUNCH(k_rank2_cells, dim3(B), dim3(CCSD_NTHREADS), 0, stream, rank2, (int)E, (int)K, thr, (unsigned long long*)bits, (int*)counts);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// ccsd_finish: quantised outputs, cell bitmask and per-complex descriptors of finished samples.  The graph pass (k_finish_graph) and
// the rank-2 pass (k_finish_rank2) are launched only when one of their outputs is requested.
extern "C" int ccsd_finish(const ccsd_finish_dims_t* d, const ccsd_state_t* in, const float* flags, const ccsd_finish_out_t* out,
                           void* stream) {
    (void)flags;      // (no output depends on the node flags: finished samples are masked, masked slots count as isolated / empty)
    if (!d || !in || !out) return set_err(CCSD_ERR_INVALID, "ccsd_finish: NULL argument");
    const int B = d->B, N = d->N, F = d->F;
    if (int st = check_batch("ccsd_finish", B, N, d->adj_mode, d->thr)) return st;
    if (d->E != N * (N - 1) / 2)
        return set_err(CCSD_ERR_INVALID, "ccsd_finish: E = " + std::to_string(d->E) + " is not N (N - 1) / 2 = " + std::to_string(N * (N - 1) / 2));
    const bool want_adj = out->adj_int || out->degree || out->degree_hist || out->edge_hist;
    const bool want_x = out->n_nodes || out->x_hist;
    const bool want_r = out->rank2_u8 || out->rank2_cell_bits || out->rank2_cell_count || out->rank2_cell_hist || out->rank2_nnz;
    if (want_adj && !in->adj) return set_err(CCSD_ERR_INVALID, "ccsd_finish: adjacency outputs requested without in->adj");
    if (want_x && (!in->x || F < 1 || F > CCSD_FIN_MAXN))
        return set_err(CCSD_ERR_INVALID, "ccsd_finish: x outputs need in->x and 1 <= F <= " + std::to_string(CCSD_FIN_MAXN));
    if (want_r && !in->rank2) return set_err(CCSD_ERR_INVALID, "ccsd_finish: rank-2 outputs requested without in->rank2");
    FinishTab tab;
    memset(&tab, 0, sizeof tab);
    int64_t K = 0;
    if (want_r) {
        const int d_min = d->d_min, d_max = d->d_max;
        if (d_min < 1 || d_max < d_min || d_max > N || d_max - d_min + 1 > CCSD_FIN_MAXBINS)
            return set_err(CCSD_ERR_INVALID, "ccsd_finish: bad cell sizes d_min = " + std::to_string(d_min) + ", d_max = " + std::to_string(d_max));
        K = cell_count(N, d_min, d_max, tab.end);
        tab.nb = d_max - d_min + 1;
        if (K < 0 || K != d->K)
            return set_err(CCSD_ERR_INVALID, "ccsd_finish: K = " + std::to_string((long long)d->K) + " is not sum C(N, d) for d = " + std::to_string(d_min) +
                                                 ".." + std::to_string(d_max) + (K < 0 ? " (which exceeds 2^24)" : " = " + std::to_string((long long)K)));
        if ((int64_t)d->E * K >= (int64_t(1) << 31)) return set_err(CCSD_ERR_INVALID, "ccsd_finish: E K must be below 2^31");
        if (((uintptr_t)in->rank2 & 15) || ((uintptr_t)out->rank2_u8 & 3) || ((uintptr_t)out->rank2_cell_bits & 7))
            return set_err(CCSD_ERR_INVALID, "ccsd_finish: rank2 must be 16-byte, rank2_u8 4-byte and rank2_cell_bits 8-byte aligned");
        if (B > 65535) return set_err(CCSD_ERR_INVALID, "ccsd_finish: B must be at most 65535 with rank-2 outputs");
    }
    if (want_adj || want_x) {
        CCSD_LAUNCH(k_finish_graph, dim3(B), dim3(CCSD_NTHREADS), 0, stream, want_x ? (const float*)in->x : (const float*)nullptr,
                    want_adj ? (const float*)in->adj : (const float*)nullptr, N, F, quant_thr(d->adj_mode, d->thr),
                    (long long*)out->adj_int, (int*)out->degree, (int*)out->degree_hist, (int*)out->edge_hist, (int*)out->n_nodes, (int*)out->x_hist);
        LAUNCH_CHECK();
    }
    if (want_r) {
        const int W = (int)((K + 63) / 64), nslab = (int)((K + CCSD_FIN_SLAB - 1) / CCSD_FIN_SLAB);
        // the accumulated outputs start from zero (atomicOr / atomicAdd per workgroup)
        if (out->rank2_cell_bits) RT_CHECK(rt_memset_async(out->rank2_cell_bits, 0, (size_t)B * W * 8, stream));
        if (out->rank2_cell_count) RT_CHECK(rt_memset_async(out->rank2_cell_count, 0, (size_t)B * 4, stream));
        if (out->rank2_cell_hist) RT_CHECK(rt_memset_async(out->rank2_cell_hist, 0, (size_t)B * tab.nb * 4, stream));
        if (out->rank2_nnz) RT_CHECK(rt_memset_async(out->rank2_nnz, 0, (size_t)B * 4, stream));
        CCSD_LAUNCH(k_finish_rank2, dim3(nslab, B), dim3(CCSD_NTHREADS), 0, stream, (const float*)in->rank2, (int)d->E, (int)K, d->thr, tab,
                    (long long)B * d->E * K, (unsigned char*)out->rank2_u8, (unsigned long long*)out->rank2_cell_bits, (int*)out->rank2_cell_count,
                    (int*)out->rank2_cell_hist, (int*)out->rank2_nnz);
        LAUNCH_CHECK();
    }
    return CCSD_OK;
}

// ---------------- clustering histograms and the MMD (ccsd_k_eval.h) ----------------
// ccsd_cluster_hist: the clustering-coefficient histogram of every graph (k_cluster_hist; same quantiser arguments as ccsd_finish)
extern "C" int ccsd_cluster_hist(const float* adj, int32_t B, int32_t N, int32_t adj_mode, float thr, const double* edges, int32_t bins,
                                 int32_t* tri2, int32_t* cluster_hist, void* stream) {
    if (!adj) return set_err(CCSD_ERR_INVALID, "ccsd_cluster_hist: NULL adj");
    if (int st = check_batch("ccsd_cluster_hist", B, N, adj_mode, thr)) return st;
    if (int st = check_hist("ccsd_cluster_hist", edges, bins)) return st;
    if (!tri2 && !cluster_hist) return CCSD_OK;
    CCSD_LAUNCH(k_cluster_hist, dim3(B), dim3(CCSD_NTHREADS), 0, stream, adj, (int)N, quant_thr(adj_mode, thr), edges, (int)bins, (int*)tri2,
                (int*)cluster_hist);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// ccsd_orbit_counts: the 4-node graphlet orbit counts of every graph (k_orbit_counts, ccsd_k_orbit.h; same quantiser arguments as ccsd_finish)
static_assert(CCSD_ORBITS == CCSD_NORBITS, "the header's orbit count is k_orbit_counts' row length");
extern "C" int ccsd_orbit_counts(const float* adj, int32_t B, int32_t N, int32_t adj_mode, float thr, int64_t* node_orbits,
                                 int64_t* graph_orbits, int32_t* orbit_nodes, void* stream) {
    if (!adj) return set_err(CCSD_ERR_INVALID, "ccsd_orbit_counts: NULL adj");
    if (int st = check_batch("ccsd_orbit_counts", B, N, adj_mode, thr)) return st;
    if (!node_orbits && !graph_orbits && !orbit_nodes) return CCSD_OK;
    CCSD_LAUNCH(k_orbit_counts, dim3(B), dim3(CCSD_NTHREADS), 0, stream, adj, (int)N, quant_thr(adj_mode, thr), (long long*)node_orbits,
                (long long*)graph_orbits, (int*)orbit_nodes);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// ---------------- NSPDK feature vectors and their MMD (ccsd_k_nspdk.h) ----------------
static_assert(CCSD_NSPDK_MAX_NODES == CCSD_NSPDK_MAXN && CCSD_NSPDK_FEATURES == CCSD_NSPDK_COLS + 1, "the header's limits are k_nspdk_features'");
// the workgroups of k_nspdk_features: each owns one 2^16-entry table of the workspace, so their number is bounded and does not grow with B
#define CCSD_NSPDK_MAX_GRID 512
static int nspdk_grid(int B) { return B < CCSD_NSPDK_MAX_GRID ? B : CCSD_NSPDK_MAX_GRID; }
static int nspdk_dims(const char* who, int B, int N) {
    const std::string w = std::string(who) + ": ";
    if (B < 1) return set_err(CCSD_ERR_INVALID, w + "B must be >= 1");
    if (N < 1) return set_err(CCSD_ERR_INVALID, w + "N = " + std::to_string(N) + " must be >= 1");
    if (N > CCSD_NSPDK_MAXN)
        return set_err(CCSD_ERR_UNSUPPORTED, w + "N = " + std::to_string(N) + " is above CCSD_NSPDK_MAX_NODES = " + std::to_string(CCSD_NSPDK_MAXN) +
                                                 ": a row of the adjacency is one 64-bit mask and the breadth-first layers are operations on such masks");
    return CCSD_OK;
}
// two keys per (ordered pair of nodes within distance 4, radius 0..4): at most 10 N^2 non-zeros, and never more than the 2^16 indices
extern "C" int32_t ccsd_nspdk_row_capacity(int32_t N) {
    if (nspdk_dims("ccsd_nspdk_row_capacity", 1, N)) return 0;
    const int c = 2 * CCSD_NSPDK_NL * N * N;
    return c < CCSD_NSPDK_COLS ? c : CCSD_NSPDK_COLS;
}
extern "C" size_t ccsd_nspdk_workspace_bytes(int32_t B, int32_t N) {
    if (nspdk_dims("ccsd_nspdk_workspace_bytes", B, N)) return 0;
    return (size_t)nspdk_grid(B) * CCSD_NSPDK_COLS * 4;
}

// ccsd_nspdk_features: the NSPDK feature vector of every graph (k_nspdk_features; same quantiser arguments as ccsd_finish)
extern "C" int ccsd_nspdk_features(const float* adj, const int32_t* labels, int32_t B, int32_t N, int32_t adj_mode, float thr, int32_t* nnz,
                                   int32_t* indices, double* values, void* workspace, size_t ws_bytes, void* stream) {
    if (!adj || !nnz || !indices || !values) return set_err(CCSD_ERR_INVALID, "ccsd_nspdk_features: NULL argument");
    if (int st = nspdk_dims("ccsd_nspdk_features", B, N)) return st;
    if (int st = check_batch("ccsd_nspdk_features", B, N, adj_mode, thr, /*fin_n=*/false)) return st;
    const size_t need = (size_t)nspdk_grid(B) * CCSD_NSPDK_COLS * 4;
    if (int st = check_scratch("ccsd_nspdk_features", workspace, ws_bytes, need)) return st;
    RT_CHECK(rt_memset_async(workspace, 0, need, stream));          // (the tables start from zero; the kernel leaves them zero)
    CCSD_LAUNCH(k_nspdk_features, dim3(nspdk_grid(B)), dim3(CCSD_NTHREADS), 0, stream, adj, (const int*)labels, (int)B, (int)N,
                quant_thr(adj_mode, thr), (int)ccsd_nspdk_row_capacity(N), (unsigned*)workspace, (int*)nnz, (int*)indices, values);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// Workspace of ccsd_nspdk_mmd: the chunk offsets of both sets (n x 257 int64 each), the 256 x 3 partial
// products, the count of non-empty rows of the second set.
struct NspdkMmdWs {
    size_t cp[2], part, cnt, bytes;
};
static NspdkMmdWs carve_nspdk_mmd(int64_t n1, int64_t n2) {
    NspdkMmdWs w;
    size_t o = 0;
    w.cp[0] = o; o += (size_t)n1 * (CCSD_NSPDK_CHUNKS + 1) * 8;
    w.cp[1] = o; o += (size_t)n2 * (CCSD_NSPDK_CHUNKS + 1) * 8;
    w.part = o; o += (size_t)CCSD_NSPDK_CHUNKS * 3 * 8;
    w.cnt = o; o += 8;
    w.bytes = o;
    return w;
}
static bool nspdk_mmd_dims_ok(int64_t n1, int64_t n2) { return n1 >= 1 && n2 >= 1 && n1 <= CCSD_MMD_MAX_ROWS && n2 <= CCSD_MMD_MAX_ROWS; }
extern "C" size_t ccsd_nspdk_mmd_workspace_bytes(int32_t n1, int32_t n2) {
    if (!nspdk_mmd_dims_ok(n1, n2))
        return no_bytes(CCSD_ERR_INVALID, "ccsd_nspdk_mmd_workspace_bytes: n1, n2 must be in 1.." + std::to_string(CCSD_MMD_MAX_ROWS));
    return carve_nspdk_mmd(n1, n2).bytes;
}

// ccsd_nspdk_mmd: compute_nspdk_mmd (mmd.py:352-377) of two sets of feature rows: k_nspdk_chunks per set, k_nspdk_dots, k_nspdk_final
extern "C" int ccsd_nspdk_mmd(const int64_t* indptr1, const int32_t* indices1, const double* values1, int32_t n1, const int64_t* indptr2,
                              const int32_t* indices2, const double* values2, int32_t n2, void* workspace, size_t ws_bytes, double* out,
                              void* stream) {
    if (!nspdk_mmd_dims_ok(n1, n2))
        return set_err(CCSD_ERR_INVALID, "ccsd_nspdk_mmd: n1 = " + std::to_string(n1) + ", n2 = " + std::to_string(n2) + " outside 1.." + std::to_string(CCSD_MMD_MAX_ROWS));
    if (!indptr1 || !indices1 || !values1 || !indptr2 || !indices2 || !values2 || !out) return set_err(CCSD_ERR_INVALID, "ccsd_nspdk_mmd: NULL argument");
    const NspdkMmdWs w = carve_nspdk_mmd(n1, n2);
    if (int st = check_scratch("ccsd_nspdk_mmd", workspace, ws_bytes, w.bytes)) return st;
    char* base = (char*)workspace;
    int* cnt = (int*)(base + w.cnt);
    RT_CHECK(rt_memset_async(cnt, 0, 8, stream));
    for (int i = 0; i < 2; ++i) {
        const int n = i ? n2 : n1;
        CCSD_LAUNCH(k_nspdk_chunks, dim3(grid_for((int64_t)n * (CCSD_NSPDK_CHUNKS + 1), 256)), dim3(CCSD_NTHREADS), 0, stream,
                    (const long long*)(i ? indptr2 : indptr1), (const int*)(i ? indices2 : indices1), n, (long long*)(base + w.cp[i]),
                    i ? cnt : (int*)nullptr);
        LAUNCH_CHECK();
    }
    double* part = (double*)(base + w.part);
    CCSD_LAUNCH(k_nspdk_dots, dim3(CCSD_NSPDK_CHUNKS), dim3(CCSD_NTHREADS), 0, stream, (const int*)indices1, values1,
                (const long long*)(base + w.cp[0]), (int)n1, (const int*)indices2, values2, (const long long*)(base + w.cp[1]), (int)n2,
                (const int*)cnt, part);
    LAUNCH_CHECK();
    CCSD_LAUNCH(k_nspdk_final, dim3(1), dim3(CCSD_NTHREADS == 1 ? 1 : 64), 0, stream, (const double*)part, out);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// Workspace of ccsd_mmd: the two transposed fp64 operands (rows padded to the pair kernel's tile), one fp64 partial per tile of each of
// the three pair reductions, then the mass flags and lengths of each set.
struct MmdSet {      // one set of rows: its offsets in the workspace; rows, padded rows, tiles
    size_t op, mass, len;
    int n, np, T;
};
struct MmdWs {
    MmdSet s[2];
    size_t part, bytes;
};
static MmdWs carve_mmd(int64_t n1, int64_t n2, int64_t L) {
    MmdWs w;
    size_t o = 0;
    w.s[0].n = (int)n1, w.s[1].n = (int)n2;
    for (MmdSet& s : w.s) {
        s.T = (s.n + CCSD_EVAL_TILE - 1) / CCSD_EVAL_TILE;
        s.np = s.T * CCSD_EVAL_TILE;
        s.op = o; o += (size_t)L * s.np * 8;
    }
    const size_t T1 = w.s[0].T, T2 = w.s[1].T;
    w.part = o; o += (T1 * T1 + T2 * T2 + T1 * T2) * 8;
    for (MmdSet& s : w.s) {
        s.mass = o; o += (size_t)s.np * 4;
        s.len = o; o += (size_t)s.np * 4;
    }
    w.bytes = o;
    return w;
}
// (the limits are the public header's: CCSD_MMD_MAX_ROWS, CCSD_MMD_MAX_BINS)
static bool mmd_dims_ok(int64_t n1, int64_t n2, int64_t L) {
    return n1 >= 1 && n2 >= 1 && L >= 1 && n1 <= CCSD_MMD_MAX_ROWS && n2 <= CCSD_MMD_MAX_ROWS && L <= CCSD_MMD_MAX_BINS;
}

extern "C" size_t ccsd_mmd_workspace_bytes(int32_t n1, int32_t n2, int32_t L) {
    if (!mmd_dims_ok(n1, n2, L))
        return no_bytes(CCSD_ERR_INVALID, "ccsd_mmd_workspace_bytes: n1, n2 must be in 1.." + std::to_string(CCSD_MMD_MAX_ROWS) + " and L in 1.." + std::to_string(CCSD_MMD_MAX_BINS));
    return carve_mmd(n1, n2, L).bytes;
}

// ccsd_mmd: compute_mmd (mmd.py:230-257) of two sets of histograms: k_mmd_prep per set, k_mmd_pairs for disc(1, 1), disc(2, 2) (both by
// symmetry) and disc(1, 2), k_mmd_final.  out (4 doubles, device) = disc(1, 1), disc(2, 2), disc(1, 2), mmd.
extern "C" int ccsd_mmd(const void* h1, int32_t n1, const int32_t* lens1, const void* h2, int32_t n2, const int32_t* lens2, int32_t L,
                        int32_t dtype, int32_t kind, int32_t flags, double sigma, double distance_scaling, void* workspace, size_t ws_bytes,
                        double* out, void* stream) {
    if (n1 < 1 || n2 < 1) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: n1 = " + std::to_string(n1) + ", n2 = " + std::to_string(n2) + ": every set needs n >= 1 rows");
    if (L < 1) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: L = " + std::to_string(L) + " must be >= 1");
    if (!mmd_dims_ok(n1, n2, L)) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: n above " + std::to_string(CCSD_MMD_MAX_ROWS) + " or L above " + std::to_string(CCSD_MMD_MAX_BINS));
    if (!h1 || !h2 || !out) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: NULL argument");
    if (dtype != CCSD_MMD_INT32 && dtype != CCSD_MMD_FP64) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: unknown dtype");
    if (kind != CCSD_MMD_EMD && kind != CCSD_MMD_TV && kind != CCSD_MMD_L2) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: unknown kind");
    if (flags & ~(CCSD_MMD_IS_HIST | CCSD_MMD_DEGREE | CCSD_MMD_F32_PMF)) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: unknown flag");
    if (kind == CCSD_MMD_EMD && !(flags & CCSD_MMD_IS_HIST))
        return set_err(CCSD_ERR_INVALID, "ccsd_mmd: the EMD kind needs is_hist (rows of unequal mass have no closed form on the line metric)");
    if (!(sigma > 0.0)) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: sigma must be > 0");
    if (kind == CCSD_MMD_EMD && !(distance_scaling > 0.0)) return set_err(CCSD_ERR_INVALID, "ccsd_mmd: distance_scaling must be > 0");
    const MmdWs w = carve_mmd(n1, n2, L);
    if (int st = check_scratch("ccsd_mmd", workspace, ws_bytes, w.bytes)) return st;
    static_assert((int)CCSD_MMD_EMD == (int)EVAL_EMD && (int)CCSD_MMD_TV == (int)EVAL_TV && (int)CCSD_MMD_L2 == (int)EVAL_L2 &&
                  (int)CCSD_MMD_IS_HIST == (int)EVAL_F_HIST && (int)CCSD_MMD_DEGREE == (int)EVAL_F_DEGREE &&
                  (int)CCSD_MMD_F32_PMF == (int)EVAL_F_F32PMF, "the header's constants are the kernels'");
    char* base = (char*)workspace;
    for (int i = 0; i < 2; ++i) {      // (k_mmd_prep: 256 rows per workgroup; the emulation's one thread takes them in turn)
        const MmdSet& s = w.s[i];
        CCSD_LAUNCH(k_mmd_prep, dim3((s.np + 255) / 256), dim3(256), 0, stream, i ? h2 : h1, (int)(dtype == CCSD_MMD_FP64),
                    (const int*)(i ? lens2 : lens1), s.n, s.np, (int)L, (int)kind, (int)flags, (double*)(base + s.op), (int*)(base + s.mass),
                    (int*)(base + s.len));
        LAUNCH_CHECK();
    }
    // disc(1, 1), disc(2, 2) -- a set against itself takes the symmetric half --, disc(1, 2): one partial per pair of tiles, b's tiles along grid x
    const MmdSet* const sets[3][2] = {{&w.s[0], &w.s[0]}, {&w.s[1], &w.s[1]}, {&w.s[0], &w.s[1]}};
    double* const part = (double*)(base + w.part);
    int c[3], done = 0;
    for (int p = 0; p < 3; done += c[p++]) {
        const MmdSet &a = *sets[p][0], &b = *sets[p][1];
        c[p] = a.T * b.T;
        CCSD_LAUNCH(k_mmd_pairs, dim3(b.T, a.T), dim3(CCSD_NTHREADS), 0, stream, (const double*)(base + a.op), (const int*)(base + a.mass),
                    (const int*)(base + a.len), a.n, a.np, (const double*)(base + b.op), (const int*)(base + b.mass), (const int*)(base + b.len),
                    b.n, b.np, (int)L, (int)kind, distance_scaling, 2 * sigma * sigma, (int)(&a == &b), part + done);
        LAUNCH_CHECK();
    }
    CCSD_LAUNCH(k_mmd_final, dim3(1), dim3(CCSD_NTHREADS), 0, stream, (const double*)part, c[0], c[1], c[2], (double)n1, (double)n2, out);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// ---------------- spectra (ccsd_k_eig.h) ----------------
static_assert(CCSD_EIG_MAXN == 512 && CCSD_EIG_MAX_SWEEPS == 30, "the public header states these limits in words");
// The workspace-resident placement of k_eigvalsh: a bounded grid of workgroups, one slab each -- the size does not grow with B.
static int eig_grid(int B, int n) { return n <= CCSD_EIG_LDS_MAXN || B < CCSD_EIG_MAX_GRID ? B : CCSD_EIG_MAX_GRID; }
static size_t eig_slab_bytes(int B, int n) {
    return n <= CCSD_EIG_LDS_MAXN ? 0 : (size_t)eig_grid(B, n) * n * (n | 1) * 8;
}
static std::string eig_too_large(const char* who, const char* what, int n) {
    return std::string(who) + ": " + what + " = " + std::to_string(n) + " is above CCSD_EIG_MAXN = " + std::to_string(CCSD_EIG_MAXN) +
           ": the solver is a Jacobi iteration of O(n^3) per sweep with one matrix per compute unit, which larger matrices are out of reach of";
}
// one launch of k_eigvalsh over matrices of order <= nmax (every argument checked by the caller)
static int eig_launch(const double* a, int B, int nmax, long long a_stride, int lda, const int* n_arr, void* slabs, double* w, float* w32,
                      int* sweeps, const double* edges, int bins, int* hist, void* stream) {
    const int threads = CCSD_NTHREADS == 1 ? 1 : nmax <= 64 ? 256 : CCSD_EIG_THREADS;
    if (nmax <= CCSD_EIG_LDS_MAXN) {
        const size_t lds = (size_t)nmax * (nmax | 1) * 8;
        // (the kernel's static arrays take another 18 KB: the attribute is raised as soon as the two together could pass 64 KB)
        if (lds + 20 * 1024 > 64 * 1024) RT_CHECK(rt_set_max_dyn_smem((const void*)k_eigvalsh<true>, lds));
        CCSD_LAUNCH(k_eigvalsh<true>, dim3(B), dim3(threads), lds, stream, a, B, nmax, a_stride, lda, n_arr, (double*)nullptr, w, w32, sweeps,
                    edges, bins, hist);
    } else {
        CCSD_LAUNCH(k_eigvalsh<false>, dim3(eig_grid(B, nmax)), dim3(threads), 0, stream, a, B, nmax, a_stride, lda, n_arr, (double*)slabs, w,
                    w32, sweeps, edges, bins, hist);
    }
    LAUNCH_CHECK();
    return CCSD_OK;
}

extern "C" size_t ccsd_eig_workspace_bytes(int32_t B, int32_t n) {
    if (B < 1 || n < 1 || n > CCSD_EIG_MAXN)
        return no_bytes(CCSD_ERR_INVALID, "ccsd_eig_workspace_bytes: B must be >= 1 and n in 1.." + std::to_string(CCSD_EIG_MAXN));
    return eig_slab_bytes(B, n);
}

// ccsd_eigvalsh: the eigenvalues of B symmetric n x n fp64 matrices, ascending (k_eigvalsh)
extern "C" int ccsd_eigvalsh(const double* a, int32_t B, int32_t n, double* w, int32_t* sweeps, void* workspace, size_t ws_bytes,
                             void* stream) {
    if (!a || !w) return set_err(CCSD_ERR_INVALID, "ccsd_eigvalsh: NULL argument");
    if (B < 1) return set_err(CCSD_ERR_INVALID, "ccsd_eigvalsh: B must be >= 1");
    if (n < 1) return set_err(CCSD_ERR_INVALID, "ccsd_eigvalsh: n = " + std::to_string(n) + " must be >= 1");
    if (n > CCSD_EIG_MAXN) return set_err(CCSD_ERR_UNSUPPORTED, eig_too_large("ccsd_eigvalsh", "n", n));
    if (int st = check_scratch("ccsd_eigvalsh", workspace, ws_bytes, eig_slab_bytes(B, n))) return st;
    return eig_launch(a, B, n, (long long)n * n, n, nullptr, workspace, w, nullptr, (int*)sweeps, nullptr, 0, nullptr, stream);
}

// Workspace of ccsd_spectral_hist: the fp64 Laplacians (B, N, N), the eigenvalues (B, N) when the caller does not take them, the
// orders (B,) likewise, and the solver's slabs.
struct SpectralWs {
    size_t lap, eig, neff, slabs, bytes;
};
static SpectralWs carve_spectral(int64_t B, int64_t N) {
    SpectralWs w;
    size_t o = 0;
    w.lap = o; o += (size_t)B * N * N * 8;
    w.eig = o; o += (size_t)B * N * 8;
    w.neff = o; o += ((size_t)B * 4 + 7) & ~(size_t)7;
    w.slabs = o; o += eig_slab_bytes((int)B, (int)N);
    w.bytes = o;
    return w;
}
extern "C" size_t ccsd_spectral_workspace_bytes(int32_t B, int32_t N) {
    if (B < 1 || N < 2 || N > CCSD_FIN_MAXN)
        return no_bytes(CCSD_ERR_INVALID, "ccsd_spectral_workspace_bytes: B must be >= 1 and N in 2.." + std::to_string(CCSD_FIN_MAXN));
    return carve_spectral(B, N).bytes;
}

// ccsd_spectral_hist: spectral_worker (evaluation/stats.py:125-137) of every graph: k_norm_laplacian, then k_eigvalsh with the
// histogram in its epilogue
extern "C" int ccsd_spectral_hist(const float* adj, int32_t B, int32_t N, int32_t adj_mode, float thr, const double* edges, int32_t bins,
                                  int32_t* hist, double* eig, int32_t* n_eff, void* workspace, size_t ws_bytes, void* stream) {
    static_assert(CCSD_FIN_MAXN <= CCSD_EIG_MAXN, "every graph ccsd_finish takes has a Laplacian the solver takes");
    if (!adj) return set_err(CCSD_ERR_INVALID, "ccsd_spectral_hist: NULL adj");
    if (int st = check_batch("ccsd_spectral_hist", B, N, adj_mode, thr)) return st;
    if (int st = check_hist("ccsd_spectral_hist", edges, bins)) return st;
    if (!hist && !eig && !n_eff) return CCSD_OK;
    const SpectralWs w = carve_spectral(B, N);
    if (int st = check_scratch("ccsd_spectral_hist", workspace, ws_bytes, w.bytes)) return st;
    char* base = (char*)workspace;
    double* lap = (double*)(base + w.lap);
    int* ne = n_eff ? (int*)n_eff : (int*)(base + w.neff);
    CCSD_LAUNCH(k_norm_laplacian, dim3(B), dim3(CCSD_NTHREADS), 0, stream, adj, (int)N, quant_thr(adj_mode, thr), lap, ne);
    LAUNCH_CHECK();
    if (!hist && !eig) return CCSD_OK;
    return eig_launch(lap, B, N, (long long)N * N, N, ne, base + w.slabs, eig ? eig : (double*)(base + w.eig), nullptr, nullptr, edges,
                      hist ? (int)bins : 0, (int*)hist, stream);
}

// The node rule of the hodge entry points is their own, not ccsd_finish's 2..CCSD_FIN_MAXN: N >= 2 (CCSD_ERR_INVALID), then the solver's
// limit on E = N (N - 1) / 2 (CCSD_ERR_UNSUPPORTED).  Fills *E on success.
static_assert(CCSD_EIG_HODGE_MAXN * (CCSD_EIG_HODGE_MAXN - 1) / 2 <= CCSD_EIG_MAXN &&
              (CCSD_EIG_HODGE_MAXN + 1) * CCSD_EIG_HODGE_MAXN / 2 > CCSD_EIG_MAXN, "k_hodge_laplacian's node list holds every N with E <= CCSD_EIG_MAXN");
static int hodge_edges(const char* who, int N, int* E) {
    if (N < 2) return set_err(CCSD_ERR_INVALID, std::string(who) + ": N = " + std::to_string(N) + " must be >= 2");
    const int64_t E64 = (int64_t)N * (N - 1) / 2;
    if (E64 > CCSD_EIG_MAXN)
        return set_err(CCSD_ERR_UNSUPPORTED, eig_too_large(who, ("N = " + std::to_string(N) + ": E = N (N - 1) / 2").c_str(), (int)E64));
    *E = (int)E64;
    return CCSD_OK;
}

extern "C" size_t ccsd_hodge_workspace_bytes(int32_t B, int32_t N) {
    int E = 0;
    if (B < 1 || N < 2) return no_bytes(CCSD_ERR_INVALID, "ccsd_hodge_workspace_bytes: B must be >= 1 and N >= 2");
    if (hodge_edges("ccsd_hodge_workspace_bytes", N, &E)) return 0;
    return (size_t)B * E * E * 8 + eig_slab_bytes(B, E);      // the fp64 hodge Laplacians (B, E, E), then the solver's slabs
}

// ccsd_hodge_spectrum: hodge_laplacian_spectrum_worker (cc_utils.py:994-1060) of every complex: k_hodge_laplacian, then k_eigvalsh
extern "C" int ccsd_hodge_spectrum(const float* adj, const uint64_t* cell_bits, int32_t B, int32_t N, int32_t d_min, int32_t d_max,
                                   int32_t adj_mode, float thr, float* spectrum, int32_t* sweeps, void* workspace, size_t ws_bytes,
                                   void* stream) {
    if (!adj || !cell_bits || !spectrum) return set_err(CCSD_ERR_INVALID, "ccsd_hodge_spectrum: NULL argument");
    if (int st = check_batch("ccsd_hodge_spectrum", B, N, adj_mode, thr, /*fin_n=*/false)) return st;
    int E = 0;
    if (int st = hodge_edges("ccsd_hodge_spectrum", N, &E)) return st;
    if (d_min < 1 || d_max < d_min || d_max > N)
        return set_err(CCSD_ERR_INVALID, "ccsd_hodge_spectrum: bad cell sizes d_min = " + std::to_string(d_min) + ", d_max = " + std::to_string(d_max));
    const int64_t K = cell_count(N, d_min, d_max);
    if (K < 0) return set_err(CCSD_ERR_INVALID, "ccsd_hodge_spectrum: sum C(N, d) for d = d_min..d_max exceeds 2^24");
    const size_t hbytes = (size_t)B * E * E * 8;
    if (int st = check_scratch("ccsd_hodge_spectrum", workspace, ws_bytes, hbytes + eig_slab_bytes(B, E))) return st;
    double* H = (double*)workspace;
    RT_CHECK(rt_memset_async(H, 0, hbytes, stream));              // (k_hodge_laplacian adds onto zeros)
    CCSD_LAUNCH(k_hodge_laplacian, dim3(B), dim3(CCSD_NTHREADS), 0, stream, adj, (const unsigned long long*)cell_bits, (int)N, (int)d_min,
                (int)d_max, (int)K, quant_thr(adj_mode, thr), H);
    LAUNCH_CHECK();
    return eig_launch(H, B, E, (long long)E * E, E, nullptr, (char*)workspace + hbytes, nullptr, spectrum, (int*)sweeps, nullptr, 0, nullptr, stream);
}

// ---------------- graphs lifted to combinatorial complexes (ccsd_k_lift.h) ----------------
static_assert(CCSD_LIFT_MAXN == CCSD_NSPDK_MAX_NODES && CCSD_LIFT_MAXN <= CCSD_FIN_MAXBINS, "a row of the adjacency is one 64-bit mask; FinishTab holds every size");
// ccsd_lift: convert_graphs_to_CCs (cc_utils.py:816-880) of every graph: k_lift_paths or k_lift_cycles, then k_lift_dense on request
extern "C" int ccsd_lift(const float* adj, int32_t B, int32_t N, int32_t adj_mode, float thr, int32_t procedure, int32_t path_length,
                         uint64_t sources_mask, int32_t d_min, int32_t d_max, uint64_t* cell_bits, int32_t* count, int32_t* cell_hist,
                         int32_t* nnz, int32_t* dropped, float* rank2, void* stream) {
    if (B == 0) return CCSD_OK;
    if (int st = check_batch("ccsd_lift", B, N, adj_mode, thr, /*fin_n=*/false)) return st;
    if (N < 2) return set_err(CCSD_ERR_INVALID, "ccsd_lift: N = " + std::to_string(N) + " must be >= 2");
    if (N > CCSD_LIFT_MAXN)
        return set_err(CCSD_ERR_UNSUPPORTED, "ccsd_lift: N = " + std::to_string(N) + " is above " + std::to_string(CCSD_LIFT_MAXN) +
                                                 ": a row of the adjacency is one 64-bit mask and both liftings are operations on such masks");
    if (procedure != CCSD_LIFT_PATHS && procedure != CCSD_LIFT_CYCLES)
        return set_err(CCSD_ERR_INVALID, "ccsd_lift: unknown procedure " + std::to_string(procedure));
    if (d_min < 1 || d_max < d_min || d_max > N)
        return set_err(CCSD_ERR_INVALID, "ccsd_lift: bad cell sizes d_min = " + std::to_string(d_min) + ", d_max = " + std::to_string(d_max));
    FinishTab tab;
    memset(&tab, 0, sizeof tab);
    const int64_t K64 = cell_count(N, d_min, d_max, tab.end);
    if (K64 < 0) return set_err(CCSD_ERR_INVALID, "ccsd_lift: sum C(N, d) for d = d_min..d_max exceeds 2^24");
    tab.nb = d_max - d_min + 1;
    if (procedure == CCSD_LIFT_PATHS) {
        if (path_length < 1) return set_err(CCSD_ERR_INVALID, "ccsd_lift: path_length = " + std::to_string(path_length) + " must be >= 1");
        if (path_length != 3)
            return set_err(CCSD_ERR_UNSUPPORTED, "ccsd_lift: path_length = " + std::to_string(path_length) +
                                                     " is not built: the path rule is a closed form for paths of 3 nodes, the length every shipped config uses");
        if (path_length < d_min || path_length > d_max)
            return set_err(CCSD_ERR_INVALID, "ccsd_lift: path_length = " + std::to_string(path_length) + " outside d_min..d_max = " +
                                                 std::to_string(d_min) + ".." + std::to_string(d_max) + ": its cells have no column");
    }
    if (!adj || !cell_bits || !count) return set_err(CCSD_ERR_INVALID, "ccsd_lift: NULL argument");
    if ((uintptr_t)cell_bits & 7) return set_err(CCSD_ERR_INVALID, "ccsd_lift: cell_bits must be 8-byte aligned");
    const int K = (int)K64, W = (K + 63) / 64, nb = tab.nb;
    // the counters start from zero (one atomicAdd per workgroup of k_lift_paths; the walking lane of k_lift_cycles adds per cell)
    RT_CHECK(rt_memset_async(count, 0, (size_t)B * 4, stream));
    if (cell_hist) RT_CHECK(rt_memset_async(cell_hist, 0, (size_t)B * nb * 4, stream));
    if (nnz) RT_CHECK(rt_memset_async(nnz, 0, (size_t)B * 4, stream));
    if (dropped) RT_CHECK(rt_memset_async(dropped, 0, (size_t)B * 4, stream));
    if (procedure == CCSD_LIFT_PATHS) {
        const int bin3 = 3 - d_min, off3 = bin3 ? tab.end[bin3 - 1] : 0, C3 = tab.end[bin3] - off3;
        CCSD_LAUNCH(k_lift_paths, dim3(B, (W + CCSD_LIFT_WPG - 1) / CCSD_LIFT_WPG), dim3(CCSD_NTHREADS), 0, stream, adj, (int)N,
                    quant_thr(adj_mode, thr), (unsigned long long)sources_mask, W, off3, C3, nb, bin3, (unsigned long long*)cell_bits,
                    (int*)count, (int*)cell_hist, (int*)nnz);
    } else {
        RT_CHECK(rt_memset_async(cell_bits, 0, (size_t)B * W * 8, stream));      // (the walk sets bits)
        CCSD_LAUNCH(k_lift_cycles, dim3(B), dim3(CCSD_NTHREADS == 1 ? 1 : 64), 0, stream, adj, (int)N, quant_thr(adj_mode, thr), tab, (int)d_min,
                    (int)d_max, W, (unsigned long long*)cell_bits, (int*)count, (int*)cell_hist, (int*)nnz, (int*)dropped);
    }
    LAUNCH_CHECK();
    if (rank2) {
        RT_CHECK(rt_memset_async(rank2, 0, (size_t)B * (N * (N - 1) / 2) * K * 4, stream));      // the zero fill: the ones are scattered onto it
        CCSD_LAUNCH(k_lift_dense, dim3(B, (W + CCSD_LIFT_DENSE_WPG - 1) / CCSD_LIFT_DENSE_WPG), dim3(CCSD_NTHREADS), 0, stream, adj, (int)N,
                    quant_thr(adj_mode, thr), tab, (int)d_min, K, W, (const unsigned long long*)cell_bits, rank2);
        LAUNCH_CHECK();
    }
    return CCSD_OK;
}

// ---------------- molecule post-processing (ccsd_k_mol.h) ----------------
static_assert(CCSD_MOL_MAX_ATOMS == CCSD_MOL_MAXN && CCSD_MOL_MAX_LABELS == CCSD_MOL_MAXL, "the header's limits are k_mol_correct's");
#define CCSD_MOL_WAVES 4                                                 // molecules (waves) per workgroup of k_mol_correct
// ccsd_mol_correct: construct_mol, correct_mol and the largest fragment (utils/mol_utils.py:144-326) of every molecule: k_mol_check_labels,
// whose flag is read back -- the one host round trip --, then k_mol_correct
extern "C" int ccsd_mol_correct(const ccsd_mol_dims_t* d, const float* adj, const int32_t* labels, const int32_t* max_valence,
                                const int32_t* charge_base, const ccsd_mol_out_t* out, void* stream) {
    if (!d || !out) return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: NULL argument");
    const int B = d->B, N = d->N, L = d->L;
    if (B == 0) return CCSD_OK;
    if (B < 0) return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: B must be >= 0");
    if (N < 1 || N > CCSD_MOL_MAXN)
        return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: N = " + std::to_string(N) + " outside 1.." + std::to_string(CCSD_MOL_MAXN) +
                                             ": lane i of a wave owns atom slot i");
    if (L < 1 || L > CCSD_MOL_MAXL)
        return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: L = " + std::to_string(L) + " outside 1.." + std::to_string(CCSD_MOL_MAXL));
    if (!adj || !labels || !max_valence || !charge_base || !out->mol_adj || !out->mol_labels || !out->mol_charge || !out->no_correct ||
        !out->n_corrections || !out->n_fragments || !out->atoms)
        return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: NULL argument");
    MolTab tab;
    memset(&tab, 0, sizeof tab);
    tab.L = L;
    for (int i = 0; i < L; ++i) {
        for (int c = 0; c < 2; ++c) {
            // (an atom over-valent without a bond would have nothing to lower; 255 bounds the sums of 63 triple bonds from above)
            if (max_valence[2 * i + c] < 0 || max_valence[2 * i + c] > 255)
                return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: max_valence of label " + std::to_string(i) + " outside 0..255");
            tab.maxv[i][c] = max_valence[2 * i + c];
        }
        if (charge_base[i] < 0 || charge_base[i] > 255)
            return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: charge_base of label " + std::to_string(i) + " outside 0..255");
        tab.cbase[i] = charge_base[i];
    }
    // a label >= L has no row in the table: the flag is raised in out->atoms[0], which k_mol_correct then overwrites
    int* flag = (int*)out->atoms;
    int bad = 0;
    RT_CHECK(rt_memset_async(flag, 0, 4, stream));
    const int64_t n = (int64_t)B * N;
    CCSD_LAUNCH(k_mol_check_labels, dim3(n < 256 * 1024 ? grid_for(n, 256) : 1024), dim3(CCSD_NTHREADS), 0, stream, (const int*)labels,
                (long long)n, L, flag);
    LAUNCH_CHECK();
    RT_CHECK(rt_d2h_sync(&bad, flag, 4, stream));
    if (bad) return set_err(CCSD_ERR_INVALID, "ccsd_mol_correct: a label is >= L = " + std::to_string(L));
    const int waves = CCSD_NTHREADS == 1 ? 1 : CCSD_MOL_WAVES;
    CCSD_LAUNCH(k_mol_correct, dim3((B + waves - 1) / waves), dim3(CCSD_NTHREADS == 1 ? 1 : 64 * waves), (size_t)waves * mol_lds_bytes(N), stream,
                adj, (const int*)labels, B, N, tab, (int)(d->largest_fragment != 0), (unsigned char*)out->mol_adj, (int*)out->mol_labels,
                (signed char*)out->mol_charge, (unsigned char*)out->no_correct, (int*)out->n_corrections, (int*)out->n_fragments,
                (int*)out->atoms);
    LAUNCH_CHECK();
    return CCSD_OK;
}
