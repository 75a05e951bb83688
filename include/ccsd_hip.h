/*
 * ccsd_hip.h -- C ABI of the MI355X-native CCSD reverse-SDE sampling path (libccsd_hip.so).
 *
 * Drop-in boundary.  The reference (AdrienC21/CCSD v0.3.3) is pure Python; its seam for this
 * path is  load_sampling_fn(...) -> sampling_fn(model_x, model_adj[, model_rank2], init_flags)
 * (ccsd/src/utils/loader.py:337-458, ccsd/src/solver.py:856-1176).  A maintainer binds this
 * library with ctypes; every pointer marked `dev` is a device pointer into a
 * caller-owned allocation (PyTorch-ROCm tensors in practice), fp32, contiguous, batch-major.
 * No torch types appear in any signature.  All calls are asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = the default stream) and return an int status.
 *
 * Entry point                  replaces (reference file:line)
 * ---------------------------  -----------------------------------------------------------------
 * ccsd_plan_create/destroy     load_model_from_ckpt + load_sde + get_pc_sampler closure setup
 *                              (loader.py:619-657, 242-267; solver.py:856-1104)
 * ccsd_score                   get_score_fn / get_score_fn_cc applied to ScoreNetworkX /
 *                              ScoreNetworkA(_CC) / ScoreNetworkF.forward
 *                              (losses.py:18-198; models/ScoreNetwork_{X,A,A_CC,F}.py)
 * ccsd_init_state              sde.prior_sampling(_sym) + mask_x/mask_adjs/mask_rank2
 *                              (solver.py:1111-1118; sde.py:426-449, 583-608)
 * ccsd_corrector_norms         first half of LangevinCorrector.update_fn_* : score, noise, the two
 *                              batch norms (solver.py:759-767, 773-780, 787-797)
 * ccsd_corrector_apply         second half: step_size, x_mean, x (solver.py:767-769, 781-783, 797-801)
 * ccsd_predictor               ReverseDiffusionPredictor / EulerMaruyamaPredictor.update_fn_*
 *                              (solver.py:210-313, 367-463) + RSDE.sde/discretize (sde.py:180-340)
 * ccsd_s4_apply                the update half of one S4_solver step (solver.py:1296-1352, 1446-1529)
 * ccsd_sampler_run             the whole pc_sampler / s4_solver loop (solver.py:1109-1174, 1266-1352)
 * ccsd_sampler_run_ex          the same loop with a reduce hook on the Langevin norm sums: the hook stands where DataParallel
 *                              gathers the replicas' scores before torch.norm(...).mean() (solver.py:763-767;
 *                              utils/loader.py:649-650)
 * ccsd_quantize                quantize_mol / quantize (graph_utils.py:181-213)
 * ccsd_rank2_cells             the rank-2 part of cc_from_incidence's input, as a cell bitmask (cc_utils.py:243-262)
 * ccsd_finish                  everything after the last predictor step in one pass per tensor: quantize / quantize_mol of adj and
 *                              quantize of rank2 (sampler.py:1216-1225, 520-535), the cell bitmask, and the per-complex integers the
 *                              evaluators histogram (degree_worker, evaluation/stats.py:36; rank1_distrib_worker /
 *                              rank2_distrib_worker, cc_utils.py:1208-1334)
 * ccsd_cluster_hist            clustering_worker on adjs_to_graphs(adj): np.histogram of nx.clustering per graph
 *                              (evaluation/stats.py:206-220; graph_utils.py:216-251)
 * ccsd_orbit_counts            what orbit_stats_all reads from the external orca program (`orca node 4`): the 4-node graphlet orbit
 *                              counts per node and per graph, and the node count it divides by (evaluation/stats.py:343-435)
 * ccsd_nspdk_features          eden.py's vectorize(graphs, complexity=4, discrete=True) for graphs with INTEGER node labels: the NSPDK
 *                              feature row of every graph (evaluation/eden.py; mmd.py:331-337)
 * ccsd_nspdk_mmd               compute_nspdk_mmd on two sets of such rows (evaluation/mmd.py:352-377; nspdk_stats, stats.py:438-467)
 * ccsd_mmd                     compute_mmd with gaussian_emd / gaussian_tv / gaussian: the scores of degree_stats, clustering_stats,
 *                              rank1_distrib_stats, rank2_distrib_stats (evaluation/mmd.py:27-257; evaluation/stats.py:60-310;
 *                              cc_utils.py:1235-1406); ccsd_mmd_workspace_bytes sizes its workspace
 * ccsd_eigvalsh                the eigenvalues of many small dense symmetric fp64 matrices (what scipy.linalg.eigvalsh /
 *                              torch.linalg.eigvalsh are called for in the two workers below); ccsd_eig_workspace_bytes sizes its workspace
 * ccsd_spectral_hist           spectral_worker: the histogram of the normalised Laplacian's eigenvalues per graph
 *                              (evaluation/stats.py:125-137); ccsd_spectral_workspace_bytes sizes its workspace
 * ccsd_hodge_spectrum          hodge_laplacian_spectrum_worker: the eigenvalues of F F^T of the complex's rank-1 / rank-2 incidence
 *                              matrix (cc_utils.py:994-1060); ccsd_hodge_workspace_bytes sizes its workspace
 * ccsd_lift                    convert_graphs_to_CCs + CC_to_incidence_matrices for the two lifting rules the configs ship:
 *                              path_based_lift_CC with path_length 3 and cycles_lift_CC (cc_utils.py:816-880, 1644-1754, 265-330), as the
 *                              cell bitmask and descriptors ccsd_finish writes, and on request the dense rank-2 incidence tensor
 * ccsd_mol_correct             gen_mol without rdkit: construct_mol's formal charges, correct_mol and the largest fragment of
 *                              valid_mol_can_with_seg on integer bond orders (utils/mol_utils.py:144-326)
 */
#ifndef CCSD_HIP_H
#define CCSD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCSD_ABI_VERSION 5

/* status codes; the Python shim re-raises the reference's exception types */
enum {
    CCSD_OK = 0,
    CCSD_ERR_INVALID = 1,       /* ValueError: bad argument / shape / NULL */
    CCSD_ERR_UNSUPPORTED = 2,   /* NotImplementedError: config outside the HIP path's envelope */
    CCSD_ERR_WEIGHTS = 3,       /* ValueError: weight blob size does not match the config */
    CCSD_ERR_RUNTIME = 4,       /* RuntimeError: HIP runtime failure (hipGetLastError text via ccsd_last_error) */
    CCSD_ERR_WORKSPACE = 5,     /* ValueError: workspace too small */
    CCSD_ERR_CALLBACK = 6       /* the reduce hook of ccsd_sampler_run_ex returned non-zero; the Python shim re-raises the hook's exception */
};

enum { CCSD_SDE_VP = 0, CCSD_SDE_VE = 1, CCSD_SDE_SUBVP = 2 };
enum { CCSD_PRED_EULER = 0, CCSD_PRED_REVERSE = 1, CCSD_PRED_S4 = 2 };
enum { CCSD_CORR_NONE = 0, CCSD_CORR_LANGEVIN = 1 };
enum { CCSD_TARGET_X = 0, CCSD_TARGET_ADJ = 1, CCSD_TARGET_RANK2 = 2 };

/* Per diffusion step, per target (x, adj, rank2) scalars.  The host computes them with the same
 * fp32 arithmetic as the reference's SDE classes (sde.py) so that the device never re-derives a
 * table index or a sigma:
 *   sscale : score = sscale * net(...)      (1 for VE, -1/std(t) for VP/subVP; losses.py:157-163)
 *   alpha  : Langevin alpha                 (alphas[timestep] for VP/subVP, 1 for VE; solver.py:752-756)
 *   pa,pb,pc : predictor  v_mean = pa*v + pb*net ; v = v_mean + pc*z   (pb already includes sscale)
 *   m1,s1,d,m2,s2 : S4_solver (solver.py:1179-1563), after its Langevin-style correction v1:
 *              v2 = m1*v1 + s1*z2   (sde.transition(v, t, dt/2));   v3 = v2 + d*net   (Sdrift*dt, d = -g(t)^2*sscale*dt);
 *              v_mean = m2*v3 ; v = v_mean + s2*z3   (sde.transition(v, t + dt/2, dt/2)).  Zero for the PC predictors.
 */
typedef struct {
    float sscale, alpha, pa, pb, pc;
    float m1, s1, d, m2, s2;
} ccsd_step_coef_t;

typedef struct {
    int32_t abi_version;        /* = CCSD_ABI_VERSION */
    /* shapes */
    int32_t N, F, is_cc, d_min, d_max;   /* E and K are derived: E=N(N-1)/2, K=sum C(N,k) */
    /* ScoreNetworkX (ScoreNetwork_X.py:26-75) */
    int32_t x_depth, x_nhid;
    /* ScoreNetworkA / ScoreNetworkA_CC graph branch (ScoreNetwork_A.py:351-460) */
    int32_t a_num_layers, a_num_linears, a_c_init, a_c_hid, a_c_final, a_nhid, a_adim, a_num_heads;
    /* ScoreNetworkA_CC hodge branch (ScoreNetwork_A_CC.py:155-205); a_is_cc_net=0 -> ScoreNetworkA;
     * a_is_cc_net=2 -> ScoreNetworkA_Base_CC (ScoreNetwork_A_Base_CC.py:105-195): HodgeBaselineLayers, h_nhid = nhid_h,
     * h_adim = hidden_h, h_num_heads unused */
    int32_t a_is_cc_net, h_num_layers, h_num_linears, h_nhid, h_adim, h_c_hid, h_c_final, h_num_heads;
    /* ScoreNetworkF (ScoreNetwork_F.py:24-145) */
    int32_t f_num_layers, f_num_linears, f_nhid, f_c_hid, f_c_final, f_cnum, f_num_layers_mlp, f_use_hodge_mask;
    /* sampler (solver.py:856-875) */
    int32_t predictor, corrector, n_corr_steps, probability_flow, denoise;
    float snr, scale_eps;
    int32_t diff_steps;         /* sde_adj.N == number of rows of step_coef */
    int32_t batch_hint;         /* expected batch per launch (0 = unknown): picks the LDS layout of the graph-network kernel so
                                 * that ceil(batch / #CUs) workgroups are co-resident per CU; any batch stays correct */
    /* ScoreNetworkX_GMH (ScoreNetwork_X.py:156-341) when x_gmh=1: x_depth AttentionLayers (x_nhid wide) instead of GCN layers */
    int32_t x_gmh, x_num_linears, x_c_init, x_c_hid, x_c_final, x_adim, x_num_heads;
    /* conv="MLP" (attention.py:168-178): Q and K of every Attention are 2-layer tanh MLPs of x (no adjacency) instead of
     * DenseGCNConv; V stays a DenseGCNConv.  a_: the A-network's AttentionLayers, x_: ScoreNetworkX_GMH's */
    int32_t a_conv_mlp, x_conv_mlp;
} ccsd_config_t;

typedef struct ccsd_plan ccsd_plan_t;

/* Build a plan: validates the config, uploads weights and tables to the current HIP device.
 * `weights` is a HOST pointer to the canonical weight blob (order documented in DESIGN.md,
 * produced by ccsd_amd.plan.pack_weights); `step_coef` is a HOST array [diff_steps][3]. */
int ccsd_plan_create(const ccsd_config_t* cfg, const float* weights, size_t n_weights,
                     const ccsd_step_coef_t* step_coef, ccsd_plan_t** out);
void ccsd_plan_destroy(ccsd_plan_t* plan);

/* number of floats the canonical weight blob must hold for this config (0 on invalid config) */
size_t ccsd_weight_count(const ccsd_config_t* cfg);
/* E and K for the config */
void ccsd_rank2_dims(const ccsd_config_t* cfg, int32_t* E, int64_t* K);
/* bytes of device scratch the step/run calls need for batch B
 *
 * THE WORKSPACE CONTRACT (every call that takes `workspace`, `workspace_bytes`; pinned by tests/purity_cases.py):
 *   - Contents on entry are ARBITRARY: stale bytes of another call, another batch size or another plan, NaN patterns, anything.  No
 *     call clears the workspace as a whole; whatever a kernel reads it either wrote earlier in the same call (or in the first call of
 *     a pair, below) or discards with a select.  So one workspace may serve several plans in turn.
 *   - Nothing outside [workspace, workspace + ccsd_workspace_bytes(plan, B)) is touched, whatever `workspace_bytes` says beyond that;
 *     a smaller `workspace_bytes` returns CCSD_ERR_WORKSPACE and launches nothing.
 *   - A call is self-contained, with these exceptions, which carry state through the workspace (the raw network outputs and the
 *     noise norms of the norms pass): ccsd_corrector_norms -> ccsd_corrector_apply and ccsd_corrector_norms -> ccsd_s4_apply.  The
 *     second call must receive the same workspace, plan, B and stream, with no other call on that workspace in between.
 *     ccsd_sampler_run(_ex) is one call: everything it carries from step to step, the third state buffer of n_steps > 1 included,
 *     it writes itself.  The reduce hook sees the six sums INSIDE the workspace.
 *   - Alignment: the base must be a multiple of 256 bytes.  The buffers are carved from the base at multiples of 256 bytes, and the
 *     kernels read them with 16-byte loads (float4 rows of H at stride h_ld(E), the Kp / Ep byte tables in words), so a base that is
 *     not 16-byte aligned is undefined behaviour; 256 is what the carve assumes and what every hipMalloc / torch allocation gives.
 *   The plan-free operations (ccsd_mmd, ccsd_eigvalsh, ...) state the size and the 8-byte alignment of their scratch with their
 *   declarations; the same holds for it: arbitrary contents on entry, nothing touched outside the stated size.
 *
 * HOST SYNCHRONISATION.  Every call only enqueues work on `stream` and returns, except: ccsd_plan_create and ccsd_plan_destroy
 * (uploads, frees); ccsd_init_state, ccsd_noise_draws and ccsd_noise_draws_at when B exceeds every B these three have seen on the
 * plan (the plan-owned off-bit buffer grows: the DEVICE is synchronised, then the buffer is reallocated); ccsd_profile_read (waits
 * for its events).  No other call waits for the device, allocates or frees.  (ccsd_amd's Python wrapper of ccsd_nspdk_features
 * reads the row counts back to compact the rows: that round trip is the wrapper's, not the C call's.) */
size_t ccsd_workspace_bytes(const ccsd_plan_t* plan, int32_t B);

const char* ccsd_last_error(void);

/* Device state of one batch shard: caller-owned, fp32, contiguous.  rank2 may be NULL when !is_cc. */
typedef struct {
    float* x;      /* dev (B,N,F) */
    float* adj;    /* dev (B,N,N) */
    float* rank2;  /* dev (B,E,K) */
} ccsd_state_t;

/* Noise of one half-step.  NULL pointers => counter-based Philox4x32-10 in-kernel, keyed by
 * (seed, draw index, global sample index, element).  Non-NULL => the RAW standard-normal draw the
 * reference would have obtained from randn_like (full (B,N,N) for adj; the kernel applies
 * triu(1)+transpose and the flag masks exactly as gen_noise does, graph_utils.py:171-178). */
typedef struct {
    const float* zx;     /* dev (B,N,F) or NULL */
    const float* zadj;   /* dev (B,N,N) or NULL */
    const float* zrank2; /* dev (B,E,K) or NULL */
} ccsd_noise_t;

/* score = sscale(t) * net(x, adj, rank2, flags) for one target; `sscale` is passed by the caller
 * (1 for VE, -1/std(t) for VP).  out has the target's shape. */
int ccsd_score(ccsd_plan_t* plan, int32_t target, int32_t B, const ccsd_state_t* in, const float* flags_dev,
               float sscale, float* out_dev, void* workspace, size_t workspace_bytes, void* stream);

/* state <- masked prior.  prior==NULL: Philox draws (draw index 0..2); else mask the given raw draws.
 * Takes no workspace: its off-bit table lives in a plan-owned buffer.  Like every call on a plan it is reentrant per handle
 * only, and all calls on one plan belong on ONE stream (the buffer is shared between calls; when it has to grow the call
 * synchronises the device). */
int ccsd_init_state(ccsd_plan_t* plan, int32_t B, const float* flags_dev, const ccsd_noise_t* prior,
                    uint64_t seed, int64_t sample_offset, ccsd_state_t* state, void* stream);

/* The masked noise of one half-step exactly as the kernels of ccsd_sampler_run / the step calls consume it with NULL noise
 * pointers: out->{x, adj, rank2} <- gen_noise / gen_noise_rank2 (graph_utils.py:158-178, cc_utils.py:594-615) of the Philox
 * draws keyed by (seed, sample_offset + b, draw index of (step, phase)).  phase: 0 .. n_steps-1 = the Langevin corrector's
 * inner iterations, n_steps = the predictor (S4 plans: 0, 1, 2 = the three draws of a step).  Test / audit hook: feeding
 * these tensors to a CPU run of the reference algorithm as its noise stream makes the production loop (in-kernel noise,
 * fused corrector apply) comparable with it value for value.  Same generator code as the kernels (philox_normal4). */
int ccsd_noise_draws(ccsd_plan_t* plan, int32_t B, const float* flags_dev, uint64_t seed, int64_t sample_offset,
                     int32_t step, int32_t phase, ccsd_state_t* out, void* stream);

/* The same masked draws at an explicit draw index: x, adj and rank2 take draws `draw`, `draw` + 1 and `draw` + 2 (mod 2^32);
 * flat_rank2 selects the element -> group map of the rank-2 draw (0: four edge rows of a column, 1: four consecutive elements).
 * Test hook for the ends of the counter range, which no (step, phase) of a plan reaches.  Arguments are checked as ccsd_init_state
 * checks them.  (A library built before this entry point existed does not load under the Python binding, which resolves every
 * declared symbol: to compare against such a build, run it from its own source tree.) */
int ccsd_noise_draws_at(ccsd_plan_t* plan, int32_t B, const float* flags_dev, uint64_t seed, int64_t sample_offset,
                        uint32_t draw, int32_t flat_rank2, ccsd_state_t* out, void* stream);

/* Which kernels a plan selected (host-side facts, no device work). */
enum {
    CCSD_QUERY_FUSED_R2 = 0,      /* 1: the LDS-resident fused rank-2 kernel k_r2 serves the rank-2 side; 0: the tiled kernels */
    CCSD_QUERY_XA_VARIANT = 1,    /* instantiation of the graph-network kernel k_xa: 0 plain, 1 HodgeBaseline, 2 X_GMH, 3 general; 4 / 5 / 6 plain with
                                     the qm9 / community_small / zinc250k geometry compiled in; 7 .. 10 the whole plan of a shipped configuration
                                     compiled in (qm9_CC, community_small_CC, zinc250k, ENZYMES_small_CC at their bench batch) */
    CCSD_QUERY_R2_LDS_BYTES = 2,
    CCSD_QUERY_XA_LDS_BYTES = 3,
    CCSD_QUERY_FUSED_LOOP = 4,    /* 1: ccsd_sampler_run fuses the Langevin apply into the predictor launches */
    CCSD_QUERY_MERGED_R2 = 5,     /* 1: ... and k_r2 runs the predictor half-step of step i and the rank-2 side of the norms pass of step i + 1
                                     in one launch (one block load per PC step) */
    CCSD_QUERY_EW1 = 6,           /* 1: element-wise rank-2 kernel k_ew1 (affine ScoreNetworkF without a Hodge Laplacian term, cnum = 1) */
    CCSD_QUERY_LARGE_GRAPH = 7,   /* 1: the tiled graph-network kernels k_lg_* serve the graph networks instead of k_xa (graph-only plans above
                                     64 nodes or without a k_xa LDS layout, up to N = 512; combinatorial complexes with ScoreNetworkA_CC and one
                                     hodge layer without a k_xa LDS layout, N <= 64; CCSD_LARGE_GRAPH=1 at plan creation forces it for
                                     eligible graph-only plans, CCSD_LARGE_GRAPH=2 for eligible combinatorial complexes too) */
    /* the rest of the plan's route; answers that depend on the batch are given for config.batch_hint */
    CCSD_QUERY_R2_FAMILY = 8,     /* rank-2 side: 0 none (graph-only), 1 fused k_r2, 2 element-wise k_ew1, 3 tiled (k_gemm_h + k_hf_score) */
    CCSD_QUERY_R2_INSTANCE = 9,   /* k_r2<MT, RS, AFFINE, GEN1, QM9> as the decimal digits MT RS AFFINE GEN1 QM9 (31102 = k_r2<3, 1, true, false, 2>); -1: no k_r2 */
    CCSD_QUERY_LOOP_FORM = 10,    /* ccsd_sampler_run: 0 predictor only, 1 Langevin with an apply launch of its own, 2 Langevin with the apply fused into
                                     the predictor launches, 3 S4, 4 Langevin with n_steps != 1 (the inner iterations one after the other, every apply a launch
                                     of its own, through a third state buffer in the workspace) */
    CCSD_QUERY_H_FULL = 11,       /* 1: H = F F^T comes from k_gemm_h_full (one workgroup per complex) */
    CCSD_QUERY_HP_FULL = 12,      /* k_hp_full (P_0, H and the corrector's rank2 work in one pass): bit 0 in the predictor pass, bit 1 in the norms pass */
    CCSD_QUERY_P0_NARROW = 13,    /* layer-0 hodge projection: 0 wide (k_gemm_p) or none; else k_gemm_p0<NT, KC, .> as NT * 100000 + KC */
    CCSD_QUERY_TILED_FUSE = 14,   /* 1: tiled rank-2 side, the Langevin corrector's rank2 work rides on the layer-0 projection pass */
    CCSD_QUERY_EW1_FUSE = 15,     /* 1: k_ew1 plans, the whole rank-2 side of a half-step rides on the layer-0 projection pass */
    CCSD_QUERY_H_GENERAL = 16,    /* 1: general hodge stack (R_l materialised layer by layer) */
    CCSD_QUERY_GEO_EK = 17,       /* general-path kernels: 0 run-time (E, K); 1 community_small, 2 zinc250k, 3 ENZYMES_small compiled in */
    CCSD_QUERY_H_WIDE = 18,       /* 1: ScoreNetworkA_CC hodge MLPs wider than 8 (16-wide kernels of the tiled route and the tiled rank-2 family) */
    CCSD_QUERY_FOLD_SUMS = 20,    /* 1: fused loop of a k_r2 plan, and the predictor's k_r2 launch reduces the batch norm sums itself: ccsd_sampler_run
                                     launches no k_normsum (three launches per PC step with merged k_r2).  A call of ccsd_sampler_run_ex with a reduce
                                     hook keeps the k_normsum launches; CCSD_NO_SUM_FOLD at plan creation turns the fold off */
    CCSD_QUERY_FOLD_LAST_RUN = 21, /* 1: the plan's latest ccsd_sampler_run[_ex] call ran with the folded sums (0: with k_normsum launches, or no call yet) */
    CCSD_QUERY_MLP_FORMS = 19     /* the form of the graph networks' MLPs: x_fin + 16 * a_fin + 256 * edge_mask.  x_fin / a_fin: the register-resident chain
                                     shape of ScoreNetworkX's / ScoreNetworkA's final MLP (1 .. 7; 0: un-chained, the block-wise Linear form) on the route the
                                     plan takes -- on the tiled route the shape of k_lg_fin_w (7) where that kernel runs the final MLP; bit l of edge_mask: the
                                     edge MLP of AttentionLayer l of ScoreNetworkA is chained */
};
int ccsd_plan_query(const ccsd_plan_t* plan, int32_t what, int64_t* value);

/* Langevin corrector, phase 1: evaluate the three scores (all correctors see the same pre-corrector
 * state `base`, solver.py:1129-1137; with n_steps > 1 each target's own tensor is taken from `cur`, its
 * current inner iterate, solver.py:760-769; cur == base for the first inner step), keep them in the
 * workspace, and write
 * norm_sums_dev[6] = { sum_b ||net_x[b]||, sum_b ||net_adj[b]||, sum_b ||net_rank2[b]||,
 *                      sum_b ||z_x[b]||,  sum_b ||z_adj[b]||,  sum_b ||z_rank2[b]|| }.
 * In multi-GPU exact mode the caller all-reduces these six floats (RCCL) between the two phases (ccsd_sampler_run_ex does so
 * inside the library loop, through its reduce hook). */
int ccsd_corrector_norms(ccsd_plan_t* plan, int32_t B, int32_t step, int32_t corr_iter,
                         const ccsd_state_t* base, const ccsd_state_t* cur, const float* flags_dev, const ccsd_noise_t* noise,
                         uint64_t seed, int64_t sample_offset, float* norm_sums_dev,
                         void* workspace, size_t workspace_bytes, void* stream);
/* phase 2: step_size = (snr*zn/gn)^2*2*alpha from norm_sums_dev; out = cur + step*score + sqrt(2 step)*z*scale_eps */
int ccsd_corrector_apply(ccsd_plan_t* plan, int32_t B, int32_t step, int32_t corr_iter,
                         const ccsd_state_t* cur, const float* flags_dev, const ccsd_noise_t* noise,
                         uint64_t seed, int64_t sample_offset, const float* norm_sums_dev,
                         ccsd_state_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* predictor half-step: out = pa*in + pb*net(in) + pc*z; mean (nullable) = pa*in + pb*net(in). */
int ccsd_predictor(ccsd_plan_t* plan, int32_t B, int32_t step, const ccsd_state_t* in, const float* flags_dev,
                   const ccsd_noise_t* noise, uint64_t seed, int64_t sample_offset,
                   ccsd_state_t* out, ccsd_state_t* mean, void* workspace, size_t workspace_bytes, void* stream);

/* S4_solver (plans created with predictor = CCSD_PRED_S4): one step = ccsd_corrector_norms(step, corr_iter 0, base = cur =
 * state) -- the three scores at the current state, the first noise draw and the six norm sums -- followed by
 * ccsd_s4_apply: Langevin-style correction with that score and noise (solver.py:1296-1334), transition kernel over dt/2
 * with a second draw, the score drift over dt, transition kernel over dt/2 with a third draw (solver.py:1337-1352).
 * noise1 must be the draws given to ccsd_corrector_norms; NULL noise pointers select in-kernel Philox.  `mean`
 * (nullable) receives the last transition's mean. */
int ccsd_s4_apply(ccsd_plan_t* plan, int32_t B, int32_t step, const ccsd_state_t* cur, const float* flags_dev,
                  const ccsd_noise_t* noise1, const ccsd_noise_t* noise2, const ccsd_noise_t* noise3, uint64_t seed,
                  int64_t sample_offset, const float* norm_sums_dev, ccsd_state_t* out, ccsd_state_t* mean,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The whole loop with in-kernel Philox noise and per-shard Langevin norms (the reference's own
 * divide_batch semantics, sampler.py:1199-1211).  `state` holds the prior on entry (see
 * ccsd_init_state) and the last state on exit; `result` receives the means (denoise) or the state;
 * `scratch` is a second state used for ping-pong.  PRECONDITION: `state` is MASKED by `flags_dev` -- x rows, adj rows / columns
 * and rank2 rows / columns of switched-off nodes hold zeros, as in every state the reference's loop ever sees (its prior is masked,
 * solver.py:1111-1118, and every update preserves the masks) and in everything ccsd_init_state or an earlier ccsd_sampler_run
 * wrote.  The loop's rank-2 kernels rely on it (they skip re-masking rank2 in the hodge-projection loader).
 * EVERY call -- this one and the step calls above (ccsd_score, ccsd_corrector_norms, ccsd_corrector_apply, ccsd_predictor,
 * ccsd_s4_apply, ccsd_init_state, ccsd_noise_draws) -- accepts ANY node mask: flags_dev is 0 / 1 per node, the live nodes need not
 * be a prefix (the reference's node_flags(adj) switches an isolated node off wherever it sits).  The step calls also accept states
 * that are NOT masked -- values in the rows / columns of switched-off nodes -- and an adjacency with a NON-ZERO DIAGONAL: the
 * networks see them as the reference's modules do.  What the update calls write for switched-off nodes is what the reference's update
 * carries there, whose score and noise are masked: pa * in for ccsd_predictor, the input for ccsd_corrector_apply, the two
 * transition factors times the input for ccsd_s4_apply (zero on a masked state).
 * The adjacency must be SYMMETRIC.  For an asymmetric one the result is undefined and depends on the route the planner picks: k_xa
 * reads the E unordered pairs (i < j) and takes adj[j][i] = adj[i][j], the tiled graph-network route (CCSD_QUERY_LARGE_GRAPH) reads
 * the whole matrix as the reference does.  traj_dev (nullable): [diff_steps][N*F+N*N+E*K]
 * receives sample 0 of every step (diff_traj, solver.py:1150-1165).  first_step/last_step allow
 * running a sub-range [first_step, last_step) of the diff_steps steps.  Every sampler.n_steps runs here: with n_steps != 1 the
 * Langevin inner iterations (solver.py:1131-1137) go through a third state buffer that ccsd_workspace_bytes includes. */
int ccsd_sampler_run(ccsd_plan_t* plan, int32_t B, const float* flags_dev, uint64_t seed, int64_t sample_offset,
                     int32_t first_step, int32_t last_step, ccsd_state_t* state, ccsd_state_t* scratch,
                     ccsd_state_t* result, float* traj_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Exact multi-GPU mode inside the library loop.  With DataParallel the reference gathers the replicas' scores before
 * torch.norm(...).mean() (solver.py:763-767; utils/loader.py:649-650), so the Langevin step size is batch-global; a sharded run
 * reproduces it by summing the six norm sums (see ccsd_corrector_norms: sums, not means; the step size uses only the ratio
 * zn / gn) over the shards.  The hook is called on the calling thread ONCE PER NORMS PASS -- every Langevin inner iteration of
 * every step, every S4 step, never on corrector-free plans -- after the kernel that writes the sums has been enqueued on `stream`
 * and before any kernel that reads them is.  sums_dev: dev, n = 6 floats in a buffer of at least 8.  The hook leaves the reduced
 * values in place, ordered on `stream` (an RCCL all-reduce enqueued on it, or on a stream that waits for it and that it then
 * waits for); it must not synchronise the device for correctness' sake.  A non-zero return stops the loop at once: nothing
 * further is enqueued, the call returns CCSD_ERR_CALLBACK and state / scratch / result are undefined. */
typedef int (*ccsd_reduce_fn)(float* sums_dev, int32_t n, void* stream, void* user);
typedef struct {
    ccsd_reduce_fn reduce;   /* NULL: no hook */
    void* user;              /* handed to the hook */
} ccsd_run_options_t;
/* ccsd_sampler_run with options (NULL options or a NULL hook: exactly ccsd_sampler_run).  With a hook the launches are the same in
 * number, order and arguments too, except on plans that fold the norm sums into k_r2 (CCSD_QUERY_FOLD_SUMS): there a hooked call
 * launches k_normsum ahead of the hook, as CCSD_NO_SUM_FOLD would; the results are bit-identical either way. */
int ccsd_sampler_run_ex(ccsd_plan_t* plan, int32_t B, const float* flags_dev, uint64_t seed, int64_t sample_offset,
                        int32_t first_step, int32_t last_step, ccsd_state_t* state, ccsd_state_t* scratch,
                        ccsd_state_t* result, float* traj_dev, void* workspace, size_t workspace_bytes, void* stream,
                        const ccsd_run_options_t* options);

/* quantize_mol: >=2.5->3, [1.5,2.5)->2, [0.5,1.5)->1, <0.5->0 (int64 out); thr<0 selects it, otherwise
 * quantize(t, thr): t<thr ? 0 : 1. */
int ccsd_quantize(const float* in_dev, int64_t n, float thr, int64_t* out_dev, void* stream);

/* Sparse form of the quantised rank-2 incidence matrix, the input of cc_from_incidence (cc_utils.py:243-262): column k
 * of rank2 (B,E,K) holds a rank-2 cell iff any entry of the column is >= thr (quantize(), graph_utils.py:181-192).
 * bits_dev: (B, ceil(K/64)) uint64, bit (k % 64) of word k / 64; counts_dev: (B,) int32 number of cells.  The column index
 * k enumerates itertools.combinations(range(N), d) for d = d_min..d_max (get_cells, cc_utils.py:72-94).  Replaces the
 * (B,E,K) fp32 device-to-host copy after sampling by ~K/8 bytes per complex. */
int ccsd_rank2_cells(const float* rank2_dev, int32_t B, int32_t E, int64_t K, float thr, uint64_t* bits_dev,
                     int32_t* counts_dev, void* stream);

/* The finish of a sampling run: one streaming pass over rank2 and one over (x, adj) give the quantised tensors, the cell bitmask and
 * the per-complex descriptors.  Plan-free, like ccsd_quantize and ccsd_rank2_cells, whose results it reproduces bit for bit. */
enum { CCSD_FINISH_ADJ_QUANTIZE = 0,   /* adj_int = quantize(adj, thr)   (graph_utils.py:181-192) */
       CCSD_FINISH_ADJ_MOL = 1 };      /* adj_int = quantize_mol(adj)    (graph_utils.py:195-213) */
typedef struct {
    int32_t B, N, F, E;        /* E must be N (N - 1) / 2; 2 <= N <= 512, F <= 512 */
    int64_t K;                 /* must be sum C(N, d), d = d_min..d_max (get_rank2_dim, cc_utils.py:269-283); ignored without rank-2 outputs */
    int32_t d_min, d_max;
    int32_t adj_mode;          /* CCSD_FINISH_ADJ_* */
    float thr;                 /* threshold of quantize() for rank2 and, in CCSD_FINISH_ADJ_QUANTIZE mode, for adj (the harness: 0.5) */
} ccsd_finish_dims_t;
/* Every pointer is nullable: NULL = that output is not produced; a pass none of whose outputs is requested is not launched.
 * All dev.  The four accumulated rank-2 outputs are cleared by the call itself. */
typedef struct {
    int64_t* adj_int;            /* (B,N,N)  quantize / quantize_mol of adj, as ccsd_quantize (sampler.py:1216, 520) */
    int32_t* degree;             /* (B,N)    number of j != i with adj_int[i][j] != 0: G.degree() of adjs_to_graphs (graph_utils.py:216-251) */
    int32_t* degree_hist;        /* (B,N)    bin d = node slots of degree d; bins 1.. = nx.degree_histogram(G) of degree_worker
                                  *          (evaluation/stats.py:36; adjs_to_graphs drops isolated nodes, so bin 0 -- isolated and masked slots -- has no twin) */
    int32_t* edge_hist;          /* (B,4)    pairs i < j by adj_int[i][j]: the rank-1 cells (and their bond types) rank1_distrib_worker counts
                                  *          (cc_utils.py:1208-1243, 217-238) */
    int32_t* n_nodes;            /* (B,)     rows of x with a non-zero entry: the rank-0 cells of cc_from_incidence (cc_utils.py:199-213) */
    int32_t* x_hist;             /* (B,F)    nodes with x[i][f] > 0.5: column sums of the one-hot atom types (sampler.py:1222-1225) */
    uint8_t* rank2_u8;           /* (B,E,K)  quantize(rank2, thr) (sampler.py:1216 / graph_utils.py:181-192), one byte per entry */
    uint64_t* rank2_cell_bits;   /* (B, ceil(K/64))  as ccsd_rank2_cells (cc_utils.py:243-262) */
    int32_t* rank2_cell_count;   /* (B,)     as ccsd_rank2_cells */
    int32_t* rank2_cell_hist;    /* (B, d_max - d_min + 1)  rank-2 cells per size: rank2_distrib_worker's histogram (cc_utils.py:1315-1334) */
    int32_t* rank2_nnz;          /* (B,)     entries of rank2 that are >= thr */
} ccsd_finish_out_t;
/* in->rank2 == NULL: a graph-only call (the rank-2 outputs must be NULL).  flags_dev (B,N), nullable: accepted for symmetry with the
 * other entry points; no output depends on it (finished samples are masked).  Returns CCSD_ERR_INVALID with a message when E or K do
 * not belong to (N, d_min, d_max). */
int ccsd_finish(const ccsd_finish_dims_t* dims, const ccsd_state_t* in, const float* flags_dev,
                const ccsd_finish_out_t* out, void* stream);

/* The clustering-coefficient histogram of every graph of adj_dev (B,N,N), 2 <= N <= 512: clustering_worker (evaluation/stats.py:206-220)
 * on adjs_to_graphs (graph_utils.py:216-251).  An edge i -- j is a non-zero quantised entry adj[i][j], j != i, with the quantiser of
 * ccsd_finish (adj_mode, thr); row i alone is read for node i: adj must be SYMMETRIC.  Nodes without an edge are not counted, a graph
 * without any edge counts as one node in bin 0.
 * edges_dev: bins + 1 doubles, the host's np.linspace(0.0, 1.0, bins + 1) (1 <= bins <= 1024): a coefficient c = t2 / (d (d - 1)) (fp64,
 * IEEE division) goes to the largest bin i with edges[i] <= c, the last bin closed at 1, exactly as np.histogram places it.
 * tri2_dev (B,N) int32: t2 = twice the triangles through each node; cluster_hist_dev (B,bins) int32.  Both nullable.
 * CCSD_ERR_INVALID with a message for N outside 2..512 or bins outside 1..CCSD_CLUSTER_MAX_BINS (the histogram of a graph is kept in LDS). */
#define CCSD_CLUSTER_MAX_BINS 1024
int ccsd_cluster_hist(const float* adj_dev, int32_t B, int32_t N, int32_t adj_mode, float thr, const double* edges_dev, int32_t bins,
                      int32_t* tri2_dev, int32_t* cluster_hist_dev, void* stream);

/* The graphlet orbit counts of every graph of adj_dev (B,N,N), 2 <= N <= 512: the integers orbit_stats_all (evaluation/stats.py:382-435)
 * gets from `orca node 4` on adjs_to_graphs (graph_utils.py:216-251), computed from the adjacency bit masks by a closed form -- no
 * program is started.  Edges, the quantiser (adj_mode, thr) and the SYMMETRIC-adjacency contract are ccsd_cluster_hist's.
 * The CCSD_ORBITS = 15 orbits are ORCA's: 0 edge; 1, 2 end and middle of the 3-path; 3 triangle; 4, 5 end and inner node of the 4-path;
 * 6, 7 leaf and centre of the claw; 8 4-cycle; 9, 10, 11 the paw's pendant, its triangle nodes without and with the tail; 12, 13 the
 * diamond's nodes of degree 2 and 3; 14 K4.
 * node_orbits_dev (B,N,15) int64: node_orbits[b][v][k] = the induced connected subgraphs on 2, 3 or 4 nodes in which node v sits at orbit
 * k; zeros for nodes without an edge.  The rows of the nodes that have an edge, in slot order, are orca's output rows.
 * graph_orbits_dev (B,15) int64: the column sums over the nodes (above 2^32 for dense graphs of a few hundred nodes).
 * orbit_nodes_dev (B,) int32: the nodes that have an edge, or 1 for a graph without any: G.number_of_nodes(), orbit_stats_all's divisor.
 * All three nullable; with all three NULL nothing is launched.  No workspace.  CCSD_ERR_INVALID with a message for N outside 2..512. */
#define CCSD_ORBITS 15
int ccsd_orbit_counts(const float* adj_dev, int32_t B, int32_t N, int32_t adj_mode, float thr, int64_t* node_orbits_dev,
                      int64_t* graph_orbits_dev, int32_t* orbit_nodes_dev, void* stream);

/* The NSPDK feature vector of every graph of adj_dev (B,N,N), 1 <= N <= 64: the row eden.py's vectorize(graphs, complexity = 4,
 * discrete = True) gives for the graph whose nodes carry INTEGER labels (Python's hash of an int is the int, so the row is deterministic;
 * the reference's atom-symbol strings hash differently in every process).  labels_dev (B,N) int32: the label per node slot, negative = the
 * slot holds no node; NULL = every slot is a node with label 0.  Edges, the quantiser (adj_mode, thr) and the SYMMETRIC-adjacency contract
 * are ccsd_cluster_hist's; an edge with an absent endpoint is ignored; the edge label is the quantised bond order 1..3 with
 * CCSD_FINISH_ADJ_MOL and 1 otherwise.  The vectoriser's steps are written out in ccsd_amd/csrc/ccsd_k_nspdk.h.
 * Output, a row-capacity layout with cap = ccsd_nspdk_row_capacity(N) = min(65536, 10 N^2):
 *   nnz_dev (B,) int32            non-zeros of the row; 0 for a graph without a node
 *   indices_dev (B,cap) int32     the feature indices, ascending, 1 .. 65536 (the feature space is CCSD_NSPDK_FEATURES = 65537 wide)
 *   values_dev (B,cap) fp64       the values (the row has unit L2 norm); entries at and past nnz are not written
 * All counting is integer and every floating-point sum has a fixed order: two calls give identical bits.
 * workspace: ccsd_nspdk_workspace_bytes(B, N) bytes, 8-byte aligned (it does not grow with B past 512 graphs).
 * N > 64: CCSD_ERR_UNSUPPORTED; other bad sizes: CCSD_ERR_INVALID (the size functions then return 0). */
#define CCSD_NSPDK_MAX_NODES 64
#define CCSD_NSPDK_FEATURES 65537
int32_t ccsd_nspdk_row_capacity(int32_t N);
size_t ccsd_nspdk_workspace_bytes(int32_t B, int32_t N);
int ccsd_nspdk_features(const float* adj_dev, const int32_t* labels_dev, int32_t B, int32_t N, int32_t adj_mode, float thr,
                        int32_t* nnz_dev, int32_t* indices_dev, double* values_dev, void* workspace, size_t ws_bytes, void* stream);

/* compute_nspdk_mmd (evaluation/mmd.py:352-377) of two sets of feature rows in CSR form on the device: indptr (n + 1) int64, indices
 * int32 ascending within a row and in 1 .. 65536, values fp64.  Under the linear kernel the mean over all pairs of K(x, x') is the squared
 * norm of the set's mean vector, so out_dev (4 doubles) = [mean Kxx, mean Kyy, mean Kxy, mmd = Kxx + Kyy - 2 Kxy] comes from the two
 * mean vectors, every sum in a fixed order.  Rows of the FIRST set without a non-zero count as zero vectors; rows of the SECOND
 * (predicted) set without a non-zero are left out, as nspdk_stats drops graphs without a node (stats.py:452-454) -- a second set with
 * no row left gives NaN.  1 <= n1, n2 <= CCSD_MMD_MAX_ROWS.  workspace: ccsd_nspdk_mmd_workspace_bytes(n1, n2) bytes, 8-byte aligned. */
size_t ccsd_nspdk_mmd_workspace_bytes(int32_t n1, int32_t n2);
int ccsd_nspdk_mmd(const int64_t* indptr1_dev, const int32_t* indices1_dev, const double* values1_dev, int32_t n1,
                   const int64_t* indptr2_dev, const int32_t* indices2_dev, const double* values2_dev, int32_t n2, void* workspace,
                   size_t ws_bytes, double* out_dev, void* stream);

/* compute_mmd (evaluation/mmd.py:230-257) of two sets of histograms, in fp64 and bit-reproducible from call to call:
 *   mmd = disc(1,1) + disc(2,2) - 2 disc(1,2),  disc = mean over all pairs of exp(-dist(x, y)^2 / (2 sigma^2)). */
enum { CCSD_MMD_EMD = 0,    /* gaussian_emd: dist = EMD on the ground distance toeplitz(range(L)) / distance_scaling, computed as
                             *   sum |cdf_x - cdf_y| / distance_scaling (exact on a line metric); needs CCSD_MMD_IS_HIST */
       CCSD_MMD_TV = 1,     /* gaussian_tv:  dist = 0.5 sum |x - y| */
       CCSD_MMD_L2 = 2 };   /* gaussian:     dist = sqrt(sum (x - y)^2) */
enum { CCSD_MMD_INT32 = 0, CCSD_MMD_FP64 = 1 };
enum { CCSD_MMD_IS_HIST = 1,   /* compute_mmd's is_hist: every row with a non-zero sum is divided by it */
       CCSD_MMD_DEGREE = 2,    /* rows are degree_hist of ccsd_finish: bin 0 is cleared (isolated and masked slots are no nodes of the
                                *   reference's graphs), a row that is then empty becomes [1], and the row's length is its last non-zero bin + 1 */
       CCSD_MMD_F32_PMF = 4 }; /* the division of CCSD_MMD_IS_HIST is rounded to fp32, as numpy does for the float32 histograms of
                                *   rank1_distrib_worker / rank2_distrib_worker */
/* h1_dev (n1,L), h2_dev (n2,L): int32 or fp64 rows (dtype), shorter histograms zero padded to the common L.  lens1_dev (n1,), lens2_dev
 * (n2,) int32, nullable: the length of each row's original array (default L).  A length matters only to the EMD of a row of sum zero
 * against one that has mass: pyemd's default extra_mass_penalty makes that distance (max(len_x, len_y) - 1) / distance_scaling; two
 * rows of sum zero are at distance 0.  workspace_dev: at least ccsd_mmd_workspace_bytes(n1, n2, L) bytes, 8-byte aligned.
 * out_dev: 4 doubles = disc(1,1), disc(2,2), disc(1,2), mmd.
 * Limits: 1 <= n1, n2 <= CCSD_MMD_MAX_ROWS, 1 <= L <= CCSD_MMD_MAX_BINS; CCSD_ERR_INVALID with a message outside them (ccsd_mmd_workspace_bytes
 * then returns 0).  The workspace grows as 8 L (n1 + n2) bytes for the operands plus 8 bytes per 64 x 64 tile of pairs. */
#define CCSD_MMD_MAX_ROWS (1 << 20)
#define CCSD_MMD_MAX_BINS (1 << 16)
size_t ccsd_mmd_workspace_bytes(int32_t n1, int32_t n2, int32_t L);
int ccsd_mmd(const void* h1_dev, int32_t n1, const int32_t* lens1_dev, const void* h2_dev, int32_t n2, const int32_t* lens2_dev, int32_t L,
             int32_t dtype, int32_t kind, int32_t flags, double sigma, double distance_scaling, void* workspace_dev, size_t ws_bytes,
             double* out_dev, void* stream);

/* The eigenvalues of B symmetric n x n fp64 matrices a_dev (B,n,n), 1 <= n <= CCSD_EIG_MAXN, ascending into w_dev (B,n): a parallel
 * cyclic two-sided Jacobi iteration, one workgroup per matrix, eigenvalues only.  a_dev is not modified; only its upper triangle
 * decides the rotations, a SYMMETRIC matrix is the contract.  The eigenvalues agree with LAPACK's to a small multiple of
 * n 2^-53 ||A||_F each; two calls give the same bits.
 * sweeps_dev (B,) int32, nullable: the sweeps used (0 for a diagonal matrix), or -30 when the compile-time cap of 30 sweeps ended
 * the iteration (not seen on any input; a converging matrix takes 5 to 9).
 * Up to n = 128 the matrix lives in LDS and no workspace is needed (ccsd_eig_workspace_bytes returns 0, workspace_dev may be NULL).
 * Above, it lives in a slab of workspace_dev, one slab per workgroup of a bounded grid that walks the batch:
 * ccsd_eig_workspace_bytes(B, n) = min(B, 256) n (n | 1) 8 bytes, 8-byte aligned.
 * n > CCSD_EIG_MAXN returns CCSD_ERR_UNSUPPORTED with the reason (O(n^3) per sweep on one compute unit), other bad dimensions CCSD_ERR_INVALID.
 * Range: the stopping test squares the entries without scaling, so ||A||_F^2 has to be a normal fp64 number -- entries between about
 * 1e-150 and 1e+150 in magnitude, zeros aside; outside that range the diagonal comes back unsolved with sweeps = 0.  Scale first. */
#define CCSD_EIG_MAXN 512
size_t ccsd_eig_workspace_bytes(int32_t B, int32_t n);
int ccsd_eigvalsh(const double* a_dev, int32_t B, int32_t n, double* w_dev, int32_t* sweeps_dev, void* workspace_dev, size_t ws_bytes,
                  void* stream);

/* spectral_worker (evaluation/stats.py:125-137) of every graph of adj_dev (B,N,N), 2 <= N <= 512, with the quantiser of ccsd_finish
 * (adj_mode, thr; the diagonal is ignored, row i alone is read for node i: adj must be SYMMETRIC).  Per graph: the weights are the
 * quantised entries (0/1, or bond orders 1..3 in CCSD_FINISH_ADJ_MOL mode), nodes without an edge are removed, a graph without any
 * edge is one node; L = I - D^-1/2 A D^-1/2 in fp64; its n_eff eigenvalues; np.histogram(eigenvalues, bins, range=(edges[0], edges[bins])).
 * edges_dev: bins + 1 doubles, the host's np.linspace(-1e-5, 2, bins + 1) (the reference: bins = 200; 1 <= bins <= 1024): an
 * eigenvalue goes to the largest bin i with edges[i] <= v, the last bin closed, as np.histogram places it.
 * ONE deliberate difference from the reference: every eigenvalue is clamped to [0, edges[bins]] before it is binned.  [0, 2] is the
 * exact range of this spectrum, a bipartite component has the eigenvalue 2 exactly, and LAPACK returns it as 2 - 2e-16, 2.0 or
 * 2 + 4e-16 depending on the graph; np.histogram drops the last of these.  Here the eigenvalue always counts in the last bin.
 * hist_dev (B,bins) int32 counts; eig_dev (B,N) fp64: the n_eff eigenvalues ascending, the rest zero; n_eff_dev (B,) int32.  Each nullable.
 * workspace_dev: at least ccsd_spectral_workspace_bytes(B, N) bytes, 8-byte aligned.  It holds every Laplacian of the batch, so it GROWS
 * with B: 8 B N^2 bytes plus the solver's slabs -- 16 MB for 1024 graphs of N = 45, 2 GB for 1024 graphs of N = 512.  Split a large
 * batch into several calls to bound it; the rows of the outputs are independent. */
size_t ccsd_spectral_workspace_bytes(int32_t B, int32_t N);
int ccsd_spectral_hist(const float* adj_dev, int32_t B, int32_t N, int32_t adj_mode, float thr, const double* edges_dev, int32_t bins,
                       int32_t* hist_dev, double* eig_dev, int32_t* n_eff_dev, void* workspace_dev, size_t ws_bytes, void* stream);

/* hodge_laplacian_spectrum_worker (cc_utils.py:994-1060) of every complex: the eigenvalues of H = F F^T, where F (E,K) is the incidence
 * matrix CC_to_incidence_matrices returns for the complex cc_from_incidence builds from the quantised sample: F[e][k] = 1 iff cell k
 * is present (bit k of cell_bits_dev (B, ceil(K/64)), as ccsd_finish / ccsd_rank2_cells write it; K = sum of C(N, d), d = d_min..d_max, in
 * get_cells order), both nodes of edge e lie in cell k, and edge e is in the quantised adjacency (adj_dev (B,N,N) with the quantiser of
 * ccsd_finish; symmetric).  H is built in exact integer arithmetic, solved in fp64, and rounded to fp32 once:
 * spectrum_dev (B,E) float32, ascending, E = N (N - 1) / 2; a complex without a cell gives exact zeros.  sweeps_dev (B,) int32, nullable: as ccsd_eigvalsh.
 * workspace_dev: at least ccsd_hodge_workspace_bytes(B, N) bytes, 8-byte aligned.  It holds every H of the batch, so it GROWS with B:
 * 8 B E^2 bytes plus the solver's slabs -- 296 MB for 1024 complexes at E = 190, 2 GB at E = 496.  Split a large batch into several
 * calls to bound it; the rows of the output are independent.
 * E > CCSD_EIG_MAXN (N > 32) returns CCSD_ERR_UNSUPPORTED with the reason (ccsd_hodge_workspace_bytes then returns 0): the E = 703 and
 * E = 1176 complexes are out of reach of a Jacobi iteration on one compute unit. */
size_t ccsd_hodge_workspace_bytes(int32_t B, int32_t N);
int ccsd_hodge_spectrum(const float* adj_dev, const uint64_t* cell_bits_dev, int32_t B, int32_t N, int32_t d_min, int32_t d_max,
                        int32_t adj_mode, float thr, float* spectrum_dev, int32_t* sweeps_dev, void* workspace_dev, size_t ws_bytes,
                        void* stream);

/* Graphs lifted to combinatorial complexes: the rank-2 cells convert_graphs_to_CCs (cc_utils.py:816-880) adds to every graph of
 * adj_dev (B,N,N), 2 <= N <= 64, in the sparse form ccsd_finish writes and ccsd_hodge_spectrum reads.  The graph is the quantised
 * adjacency (adj_mode, thr as in ccsd_finish; in mol mode every bond order is a plain edge); the diagonal is ignored and pair (i, j),
 * i < j, is read from row i, exactly as ccsd_hodge_spectrum reads it.  Column k names its nodes as get_cells does: sizes d_min..d_max,
 * itertools.combinations(range(N), d) order within a size; K = sum of C(N, d).
 * procedure CCSD_LIFT_PATHS (path_based_lift_CC, cc_utils.py:1692-1724) with path_length 3: {a, b, c} is a cell iff one of the three nodes
 *   is adjacent to the other two and at least one of those two is a source (bit n of sources_mask: node n starts paths; the reference's
 *   "basic" setting is all ones; the empty mask gives no cell).  Any other path_length: CCSD_ERR_UNSUPPORTED; path_length outside
 *   d_min..d_max: CCSD_ERR_INVALID.
 * procedure CCSD_LIFT_CYCLES (cycles_lift_CC, cc_utils.py:1727-1754): the node sets of networkx.cycle_basis(networkx.from_numpy_array(A))
 *   -- components in descending order of their highest node, which is the root; a LIFO stack walk that visits neighbours in ascending
 *   order.  path_length and sources_mask are ignored.  DIFFERENCE from the reference: it rebuilds the graph from frozenset edges first, so its
 *   root and neighbour order follow CPython's set-slot order and its basis is another one for about half of all random graphs; the
 *   NUMBER of cycles, E - V + C, is the same.  A cycle whose size lies outside d_min..d_max has no column (the reference raises KeyError
 *   there): it is counted in dropped_dev and not represented.
 * Outputs, every one fully written by the call (the caller need not clear anything):
 *   cell_bits_dev (B, ceil(K/64)) uint64   bit k % 64 of word k / 64 = column k is a cell; the tail bits of the last word are 0
 *   cell_count_dev (B,) int32              the set bits (a node set two cycles share counts once)
 *   cell_hist_dev (B, d_max-d_min+1) int32 the set bits per cell size                                         (nullable)
 *   nnz_dev (B,) int32                     the ones of the incidence matrix                                   (nullable)
 *   dropped_dev (B,) int32                 cycles without a column; 0 for paths                               (nullable)
 *   rank2_dev (B,E,K) fp32                 the incidence matrix of create_incidence_1_2 (cc_utils.py:265-330): F[e][k] = 1 iff column k
 *                                          is a cell and edge e of the graph lies inside it (chords of a cycle count), E = N (N - 1) / 2;
 *                                          zero-filled, then only the ones are stored                        (nullable)
 * B = 0 is a no-op.  N > 64: CCSD_ERR_UNSUPPORTED (a row of the adjacency is one 64-bit mask); 1 <= d_min <= d_max <= N and K <= 2^24, else
 * CCSD_ERR_INVALID. */
enum { CCSD_LIFT_PATHS = 0, CCSD_LIFT_CYCLES = 1 };
int ccsd_lift(const float* adj_dev, int32_t B, int32_t N, int32_t adj_mode, float thr, int32_t procedure, int32_t path_length,
              uint64_t sources_mask, int32_t d_min, int32_t d_max, uint64_t* cell_bits_dev, int32_t* cell_count_dev,
              int32_t* cell_hist_dev, int32_t* nnz_dev, int32_t* dropped_dev, float* rank2_dev, void* stream);

/* Molecule post-processing: what gen_mol (utils/mol_utils.py:191-229) does to every sample of a molecule run before it is scored, on
 * integer bond orders and without rdkit.  adj_dev (B,N,N) fp32 raw samples, quantised here in CCSD_FINISH_ADJ_MOL mode (bond orders
 * 0..3); pair (i, j), i < j, is read from row i, as ccsd_lift reads it -- for a symmetric adjacency the reference's adj[start, end],
 * start > end.  labels_dev (B,N) int32: the label per atom slot, negative = no atom (bonds to such a slot are ignored).  HOST tables, read
 * during the call: max_valence (L,2) int32, the largest permitted bond-order sum of a label's atom when neutral and with charge +1, and
 * charge_base (L,) int32, the valence above which by exactly one the atom takes charge +1 (the reference's ATOM_VALENCY), 0 for a label
 * that takes none.
 *   construct_mol   bonds enter in ascending (larger index, smaller index) order, each with the next insertion number; after every bond
 *                   the FIRST atom in slot order whose sum exceeds its maximum is looked up, and takes charge +1 when its sum is
 *                   charge_base + 1 (an earlier atom that stays over-valent masks the later ones, as in the reference);
 *                   no_correct = no atom is over-valent at the end
 *   correct_mol     while an atom is over-valent: the first one; its bond of highest order, on a tie of lowest insertion number, drops by
 *                   one; at 0 it is gone, otherwise it gets a fresh insertion number
 *   fragments       connected components of the result; largest_fragment != 0 keeps the one with the most atoms (tie: the one holding
 *                   the lowest slot) and drops every other atom.  DIFFERENCE from the reference, which keeps the fragment with the
 *                   longest SMILES string.
 * Outputs, every one required and fully written; slots are not compacted:
 *   mol_adj (B,N,N) uint8 symmetric bond orders, zero diagonal; mol_labels (B,N) int32 (-1: no atom); mol_charge (B,N) int8;
 *   no_correct (B,) uint8; n_corrections (B,) int32 decrements; n_fragments (B,) int32 after correction, before selection;
 *   atoms (B,) int32 the atoms kept.
 * The call reads one flag back from the device before its main launch (it synchronises the stream once).  B = 0 is a no-op.
 * CCSD_ERR_INVALID: N outside 1..CCSD_MOL_MAX_ATOMS, L outside 1..CCSD_MOL_MAX_LABELS, a label >= L, a table entry outside 0..255. */
#define CCSD_MOL_MAX_ATOMS 64
#define CCSD_MOL_MAX_LABELS 16
typedef struct {
    int32_t B, N;              /* molecules, atom slots per molecule */
    int32_t L;                 /* labels: rows of max_valence / charge_base */
    int32_t largest_fragment;  /* 0: keep every fragment (gen_mol's largest_connected_comp=False) */
} ccsd_mol_dims_t;
typedef struct {
    uint8_t* mol_adj;
    int32_t* mol_labels;
    int8_t* mol_charge;
    uint8_t* no_correct;
    int32_t* n_corrections;
    int32_t* n_fragments;
    int32_t* atoms;
} ccsd_mol_out_t;
int ccsd_mol_correct(const ccsd_mol_dims_t* dims, const float* adj_dev, const int32_t* labels_dev, const int32_t* max_valence,
                     const int32_t* charge_base, const ccsd_mol_out_t* out, void* stream);

/* Measurement hooks (bench.py): time every launch of selected kernels with HIP events on the launch stream.
 * kernel_id: 0 k_xa, 1 k_gemm_p, 2 k_hf_score, 3 k_gemm_h, 4 k_langevin_apply, 5 k_r2, 6 k_s4_apply, 7 k_ew1; each call adds one kernel to the
 * selection, -1 clears it.  ccsd_profile_read synchronises on that kernel's events and returns launches + summed ms. */
int ccsd_profile_kernel(ccsd_plan_t* plan, int32_t kernel_id);
/* bracket only every stride-th launch of the selected kernels (default 1 = every launch): event records break
 * back-to-back dispatch, so dense bracketing perturbs the timed region (~6 % of a qm9_CC step). */
int ccsd_profile_stride(ccsd_plan_t* plan, int32_t stride);
int ccsd_profile_read(ccsd_plan_t* plan, int32_t kernel_id, int64_t* launches, double* total_ms);
/* ALL launches of a selected kernel since the selection / stride was last set (bracketed or not): with the mean of the
 * bracketed ones this gives the kernel's share of a timed region */
int ccsd_profile_launches(ccsd_plan_t* plan, int32_t kernel_id, int64_t* launches);
/* Diagnostic: when dev_buffer (B x 64 int64, device) is non-NULL, thread 0 of every workgroup of k_r2 (slots 0-31)
 * and k_xa (slots 32-63) stores the shader clock at its phase boundaries (tools/stamps.py).  NULL disables. */
int ccsd_debug_stamps(ccsd_plan_t* plan, void* dev_buffer);

#ifdef __cplusplus
}
#endif
#endif /* CCSD_HIP_H */
