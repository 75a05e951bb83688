// ccsd_api.h -- host side of the C ABI declared in include/ccsd_hip.h: plan construction, workspace carve-up and the launch
// sequences of one corrector / predictor half-step.  Included once by ccsd_hip.hip (product) and by tests/emu/ccsd_emu.cpp (CPU
// emulation of the same kernels, test infrastructure only).
//
// Which kernel serves a plan is decided ONCE, by resolve_route() at the end of ccsd_plan_create, from (config, the weights'
// architecture, the Knobs read from the environment at creation): the k_xa / k_r2 instance and its launch entry out of the tables
// of ccsd_instances.h, the rank-2 family, the compiled-in geometry of the general-path kernels, the form of ccsd_sampler_run's loop.
// The launchers read the plan's Route; nothing on a launch path compares plans or tests a geometry.  What also depends on the
// batch of the CALL (threads per graph of k_xa, k_gemm_h_full / k_hp_full at >= 256 complexes, k_normsum's block) is a function of
// (route, B) next to resolve_route.  ccsd_plan_query reports the Route, on the product and on the emulation alike.
// What depends on the ARGUMENTS of a call is no Route field: corrector_norms / predictor name the form of their pass's rank-2 side (NR_* / PR_*) once.
#pragma once
#include "ccsd_kernels.h"
#define CCSD_INST_TABLES
#include "ccsd_instances.h"
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <string>
#include <vector>

static thread_local std::string g_last_error;
static int set_err(int st, const std::string& m) { g_last_error = m; return st; }

// widest layer of ScoreNetworkF's per-element MLPs
static inline int fnet_width(const PlanD& p) {
    int fw = p.f_fdim > p.f_cnum ? p.f_fdim : p.f_cnum;
    for (int l = 0; l < p.f_L; ++l) {
        const MlpD& m = p.fl[l];
        const int wd = m.n > 1 && m.hid > m.in ? (m.hid > m.out ? m.hid : m.out) : (m.in > m.out ? m.in : m.out);
        if (wd > fw) fw = wd;
    }
    if (p.f_fin.n > 1 && p.f_fin.hid > fw) fw = p.f_fin.hid;
    return fw;
}

// Every switch the library takes from the environment; read_knobs() is the only reader and runs first in ccsd_plan_create.
//   variable             field                 effect                                                          set by
//   CCSD_NO_FUSED_R2     no_fused_r2           no LDS-resident k_r2: the tiled / element-wise rank-2 kernels   tests (emu + gpu)
//   CCSD_HODGE_GENERAL   hodge_general         general hodge stack for any plan with > 2 hodge layers          tests
//   CCSD_NO_GEO          geo_off = 1           no instance with a geometry or plan compiled in                 tests (emu + gpu)
//   CCSD_NO_BAKE         geo_off = 2           geometry instances yes, baked-plan instances no                 tests (gpu), tools/dev
//   CCSD_NO_FUSED_APPLY  no_fused_apply        Langevin apply as a launch of its own in ccsd_sampler_run       tests (emu + gpu)
//   CCSD_NO_SUM_FOLD     no_sum_fold           k_normsum as a launch of its own in the fused loop of k_r2 plans tests (emu + gpu), A/B
//   CCSD_NO_H_FULL       no_h_full             k_gemm_h's 64 x 64 tiles instead of k_gemm_h_full / k_hp_full   tests (gpu)
//   CCSD_NO_HP_FULL      no_hp_full            k_gemm_p0 + k_gemm_h_full instead of the one k_hp_full pass     tests (gpu)
//   CCSD_HP_FULL_NORMS   hp_full_norms         k_hp_full in the norms pass too (slower: A/B only)              tests (gpu)
//   CCSD_SPLIT_BF16=3    split_bf16            EXPERIMENT: split-precision k_gemm_h_full, NOT bit-identical    tests (gpu), bench.py, tools/dev
//   CCSD_XA_THREADS      xa_threads            threads per graph of k_xa (64 .. 1024; 0 = by batch)            tests (gpu)
//   CCSD_XA_PRIO         xa_prio               k_xa issue priority: 0 rotating (default), 1 none, 2 static.    nobody
//                                              Lost on every workload (xiv); kept because k_xa<false, XA_HB> without the
//                                              mode test needs 104 bytes of scratch instead of 100 (profiles/README.md r08)
//   CCSD_LARGE_GRAPH=1|2 lg_force              tiled graph-network route for any eligible graph-only plan (1), (PlanBuilder)  tests (emu + gpu)
//                                              for eligible combinatorial-complex plans too (2: ScoreNetworkA_CC, ScoreNetworkA_Base_CC)
//   CCSD_XA_PASS=<n>     xa_pass               first k_xa LDS budget candidate tried            (PlanBuilder)  tests (emu + gpu)
//   CCSD_XA_GCH          xa_gch                channel stack in the HBM workspace first         (PlanBuilder)  tests (emu + gpu)
//   CCSD_NO_MLP_WT       no_mlp_wt             no transposed copies of the non-chained MLPs     (PlanBuilder)  tests (gpu)
//   CCSD_VERBOSE         verbose               print the k_xa LDS layout                        (PlanBuilder)  by hand
//   CCSD_DUMP_PLAN[_NAME] dump_plan[_name]     write the plan's architecture bytes as a C header               tools/bake_plan.py
struct Knobs {
    int no_fused_r2 = 0, hodge_general = 0, geo_off = 0, no_fused_apply = 0, no_h_full = 0, no_hp_full = 0, hp_full_norms = 0, split_bf16 = 0, no_sum_fold = 0;
    int xa_threads = 0, xa_prio = 0, lg_force = 0, xa_pass = -1, xa_gch = 0, no_mlp_wt = 0, verbose = 0;
    const char *dump_plan = nullptr, *dump_plan_name = nullptr;
};
static Knobs read_knobs() {
    Knobs k;
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    k.no_fused_r2 = on("CCSD_NO_FUSED_R2"); k.hodge_general = on("CCSD_HODGE_GENERAL");
    k.geo_off = on("CCSD_NO_GEO") ? 1 : on("CCSD_NO_BAKE") ? 2 : 0;
    k.no_fused_apply = on("CCSD_NO_FUSED_APPLY"); k.no_h_full = on("CCSD_NO_H_FULL"); k.no_hp_full = on("CCSD_NO_HP_FULL");
    k.hp_full_norms = on("CCSD_HP_FULL_NORMS"); k.no_sum_fold = on("CCSD_NO_SUM_FOLD");
    if (const char* v = getenv("CCSD_SPLIT_BF16")) k.split_bf16 = atoi(v) == 3 ? 3 : 0;
    if (const char* v = getenv("CCSD_XA_THREADS")) { const int t = atoi(v); if (t >= 64 && t <= 1024 && t % 64 == 0) k.xa_threads = t; }
    if (const char* v = getenv("CCSD_XA_PRIO")) k.xa_prio = atoi(v);
    if (const char* v = getenv("CCSD_LARGE_GRAPH")) { const int f = atoi(v); k.lg_force = (f == 1 || f == 2) ? f : 0; }
    if (const char* v = getenv("CCSD_XA_PASS")) k.xa_pass = atoi(v);
    k.xa_gch = on("CCSD_XA_GCH"); k.no_mlp_wt = on("CCSD_NO_MLP_WT"); k.verbose = on("CCSD_VERBOSE");
    k.dump_plan = getenv("CCSD_DUMP_PLAN"); k.dump_plan_name = getenv("CCSD_DUMP_PLAN_NAME");
    return k;
}

// Which kernels serve a plan: fixed by (config, the weights' architecture, knobs), resolved once by resolve_route().
enum { R2_NONE = 0, R2_FUSED = 1, R2_EW1 = 2, R2_TILED = 3 };       // rank-2 family: graph-only / k_r2 / k_ew1 / k_gemm_h + k_hf_score
// form of ccsd_sampler_run's loop (LOOP_LANGEVIN_MULTI: Langevin with n_corr_steps != 1 -- the inner iterations run one after the
// other through a third state buffer out of the workspace, every apply a launch of its own)
enum { LOOP_PRED_ONLY = 0, LOOP_LANGEVIN = 1, LOOP_LANGEVIN_FUSED = 2, LOOP_S4 = 3, LOOP_LANGEVIN_MULTI = 4 };
struct Route {
    // graph-network side
    int lg = 0;                     // tiled route (ccsd_k_lg.h) instead of k_xa: eligible plans (ccsd_lg_ineligible) k_xa cannot place (N > 64, no LDS
                                    // layout), or any eligible plan under CCSD_LARGE_GRAPH (1: graph-only plans, 2: all); launch_xa hands such plans to launch_lg
    int xa_variant = 0;             // XA_* (what CCSD_QUERY_XA_VARIANT reports)
    const XaEntry* xa = nullptr;    // its instance, and the run-time-geometry twin that serves launches of a fixed-256 instance with
    const XaEntry* xa_twin = nullptr;   // another (diagnostic) thread count
    int xa_threads = 0;             // CCSD_XA_THREADS (0: by batch, xa_launch)
    // rank-2 side
    int r2_family = R2_NONE;
    const R2Entry* r2 = nullptr;    // R2_FUSED: the k_r2 instance
    int r2_ldk = 0, r2_ldh = 0;     // ... and its LDS geometry
    size_t r2_lds = 0;
    // general hodge stack: more than two HodgeAdjAttentionLayers whose later projections cannot be folded into rank2's (a non-affine
    // mlp_value, or no fused rank-2 kernel for the geometry): R_l is materialised layer by layer (k_hodge_value) from the dense hodge
    // adjacencies k_xa<., XA_GEN> dumps (launch_xa); CCSD_HODGE_GENERAL forces it for any plan with more than two layers, and plans on
    // the tiled route always take it (launch_lg: the dense adjacencies are in its workspace buffer already)
    int h_general = 0;
    // hodge MLPs wider than 8 (PlanBuilder::h_wide; always on the tiled route and the tiled rank-2 family): mlp_attention on the last layer's
    // diagonal as the 16-wide MFMA chain (k_lg_hodge1_w / k_lg_hd_diag_w), mlp_value from 16 x 16 blocks (k_gemm_p_w / k_hodge_value_w)
    int h_wide = 0;
    int geo = 0;                    // index of the plan's (E, K) in CCSD_GEO_LIST (0: run-time values)
    int p0 = -1;                    // index of the narrow layer-0 projection's k_gemm_p0 in CCSD_P0_LIST (-1: wide, k_gemm_p)
    int h_full = 0;                 // launch_h's H = F F^T may come from k_gemm_h_full (use_h_full)
    unsigned hp_full_modes = 0;     // P0Fuse modes whose pass k_hp_full may serve, one bit each (use_hp_full)
    // ccsd_sampler_run
    int loop = LOOP_PRED_ONLY;
    int merged = 0;                 // LOOP_LANGEVIN_FUSED: k_r2 runs predictor i and the rank-2 side of norms pass i + 1 in one launch
    int fold_sums = 0;              // LOOP_LANGEVIN_FUSED, k_r2 plans: the predictor's k_r2 launch reduces the batch norm sums itself (R2Args::fold), no
                                    // k_normsum launch in the loop -- unless the call has a reduce hook, which needs the sums between two launches
    int tiled_fuse = 0;             // tiled rank-2 path, ONE hodge layer: the corrector's rank2 work rides on the layer-0 projection pass
    int ew1_fuse = 0;               // k_ew1 plans, ONE hodge layer: the whole rank-2 side of a half-step rides on it (P0Fuse modes 3 / 4)
    // The Langevin corrector's rank2 draws are keyed by flat groups of four consecutive elements (NoiseArgs::flat_r): they are
    // generated where rank2 streams through registers in 16-byte pieces (k_r2's block load, k_langevin_apply, k_noise_norm).
    // Priors, predictor draws and the three draws of an S4 step keep the 4-row groups of the MFMA epilogues -- except on k_ew1
    // plans, whose kernel streams 16-byte pieces for every draw.
    int corrector_flat = 0, predictor_flat = 0;
};

struct ccsd_plan : PlanRouteOut {   // (hbx, hdm, afin_lg, npacked: the planner's outputs beside PlanD, ccsd_plan.h)
    ccsd_config_t cfg;
    PlanD h;                    // host copy
    PlanD* d = nullptr;         // device copy
    float* w = nullptr;         // device weights
    float* wp = nullptr;        // device: zero-padded copies of the chain MLPs' linears (mlp_chain_tile)
    unsigned char* hpairs = nullptr;   // device: (e, e2), e <= e2, row-major: unordered pairs of the dense hodge layer
    unsigned char* edges = nullptr;
    unsigned long long* cells = nullptr;
    std::vector<ccsd_step_coef_t> coef;  // [diff_steps][3]
    size_t nweights = 0;
    long long* dbg = nullptr;   // diagnostic cycle stamps (ccsd_debug_stamps)
    unsigned long long* init_off = nullptr;   // device: off-bit table of ccsd_init_state (which takes no workspace), grown on demand
    size_t init_off_cap = 0;
    Knobs knobs;                // the environment, read ONCE at plan creation (read_knobs)
    Route rt;                   // which kernels serve the plan (resolve_route)
    int last_run_folded = 0;    // the plan's latest ccsd_sampler_run[_ex] call took the folded norm sums (CCSD_QUERY_FOLD_LAST_RUN)
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg); mutable: the launchers hold the plan const
    mutable unsigned prof_mask = 0;
    mutable size_t prof_used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // every prof_stride-th launch of a selected kernel is bracketed by events (event records break back-to-back dispatch:
    // bracketing every launch costs ~6 % of the step)
    mutable int prof_stride = 1;
    mutable size_t prof_calls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#ifndef CCSD_EMU
    mutable std::vector<hipEvent_t> prof_ev[8];
#endif
};

enum { KID_XA = 0, KID_GEMM_P = 1, KID_HF = 2, KID_GEMM_H = 3, KID_LANGEVIN = 4, KID_R2 = 5, KID_S4 = 6, KID_EW1 = 7 };
static void prof_mark(const ccsd_plan* pl, int kid, void* stream) {
#ifndef CCSD_EMU
    if (!(pl->prof_mask & (1u << kid))) return;
    const size_t call = pl->prof_calls[kid]++;                 // two calls per launch: before and after
    if (pl->prof_stride > 1 && (call >> 1) % (size_t)pl->prof_stride != 0) return;
    std::vector<hipEvent_t>& ev = pl->prof_ev[kid];
    if (pl->prof_used[kid] == ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        ev.push_back(e);
    }
    (void)hipEventRecord(ev[pl->prof_used[kid]++], (hipStream_t)stream);
#else
    (void)pl; (void)kid; (void)stream;
#endif
}
#define RT_CHECK(expr)                                                                    \
    do {                                                                                  \
        rtError_t _e = (expr);                                                            \
        if (_e != RT_OK) return set_err(CCSD_ERR_RUNTIME, std::string(#expr) + ": " + rt_error_string(_e)); \
    } while (0)
#define LAUNCH_CHECK()                                                                    \
    do {                                                                                  \
        rtError_t _e = rt_last_error();                                                   \
        if (_e != RT_OK) return set_err(CCSD_ERR_RUNTIME, std::string("kernel launch: ") + rt_error_string(_e)); \
    } while (0)

// ---------------- route ----------------
// Decides every field of pl->rt (but rt.lg, the planner's verdict) and nothing else; runs once, at the end of ccsd_plan_create.
static int resolve_route(ccsd_plan* pl) {
    const PlanD& p = pl->h;
    const ccsd_config_t& c = pl->cfg;
    const Knobs& k = pl->knobs;
    Route& r = pl->rt;
    const int E = p.E, K = p.K;
    const bool s4 = c.predictor == CCSD_PRED_S4, langevin = c.corrector == CCSD_CORR_LANGEVIN;
    // instances with the WHOLE plan as a compile-time constant: only for a plan whose architecture bytes equal a baked one's
    // (tools/bake_plan.py; ccsd_baked_*.h), and only in the instantiation the bake was made for
    unsigned char arch[sizeof(PlanD)];
    ccsd_plan_arch_bytes(p, arch);
    auto baked = [&](const unsigned char* plan, size_t size) { return size == sizeof(PlanD) && p.geo_off == 0 && memcmp(arch, plan, size) == 0; };

    // ---- graph-network side: what the network needs (XA_PLAIN / XA_HB / XA_GMH / XA_GEN), then the instance that has it compiled in
    bool conv_mlp = false;
    for (int l = 0; l < p.a_L; ++l) conv_mlp = conv_mlp || p.al[l].conv_mlp;
    if (p.x_gmh) for (int l = 0; l < p.x_depth; ++l) conv_mlp = conv_mlp || p.gl[l].conv_mlp;
    int v = p.hb_L ? XA_HB : p.x_gmh ? XA_GMH : XA_PLAIN;
    // the small-graph XA_PLAIN / XA_GMH variants are compiled without the two widest final-MLP chain shapes (ccsd_k_xa.h: they cost
    // them their registers -- 30 VGPRs spilled around the final MLP of every launch); the HodgeBaseline networks need them
    if (conv_mlp || (p.hb_L && p.x_gmh) || p.h_L > 2 || (!p.chan_global && !p.hb_L && p.a_fin.chain >= 5)) v = XA_GEN;
    if (v == XA_PLAIN && !p.chan_global && baked(CCSD_BAKED_QM9_PLAN, CCSD_BAKED_QM9_SIZE)) v = XA_BAKED9;
    else if (v == XA_PLAIN && p.chan_global && baked(CCSD_BAKED_CS_PLAN, CCSD_BAKED_CS_SIZE)) v = XA_BAKED20;
    else if (v == XA_PLAIN && p.chan_global && baked(CCSD_BAKED_Z_PLAN, CCSD_BAKED_Z_SIZE)) v = XA_BAKED38;
    else if (v == XA_GEN && !p.chan_global && baked(CCSD_BAKED_ENZ_PLAN, CCSD_BAKED_ENZ_SIZE)) v = XA_BAKEDENZ;
    else if (v == XA_PLAIN && p.geo_off != 1)
        for (const auto& g : XA_GEO_TABLE)
            if ((p.chan_global != 0) == (g.gch != 0) && p.N == g.N && (!g.F || p.F == g.F) && E == g.E && p.ldn == g.ldn) v = g.var;
    r.xa_variant = v;
    r.xa_threads = k.xa_threads;
    for (const XaEntry& e : XA_TABLE) {
        if ((e.gch != 0) != (p.chan_global != 0)) continue;
        if (e.var == v) r.xa = &e;
        if (e.var == XA_PLAIN) r.xa_twin = &e;
    }
    if (!r.xa || !r.xa_twin) return set_err(CCSD_ERR_RUNTIME, "k_xa variant " + std::to_string(v) + " has no instance in CCSD_XA_LIST");
    if (!r.xa->fixed256) r.xa_twin = nullptr;

    // ---- rank-2 side.  Fused path: one complex's rank2 block (E x K) LDS-resident, E <= 64
    const bool aff = p.f_affine != 0, gen1 = p.h_L > 1 && p.hl[0].mval.n > 1;
    const int mt = (E + 15) / 16, rem = E & 15, rs = (!aff || rem == 0 || rem > 12) ? 0 : (rem + 3) / 4;
    auto r2_find = [&](int qm9) -> const R2Entry* {
        for (const R2Entry& e : R2_TABLE)
            if (e.mt == mt && e.rs == rs && (e.affine != 0) == aff && (e.gen1 != 0) == gen1 && e.qm9 == qm9) return &e;
        return nullptr;
    };
    bool fused = false;
    if (c.is_cc && E <= 64 && !k.no_fused_r2 && !r.h_wide) {        // (k_r2 evaluates mlp_value 8 wide)
        const int Kp4 = (K + 31) & ~31, Ep4 = (E + 3) & ~3;   // K zero-padded to whole 8-step MFMA batches
        int ldk = Kp4; while ((ldk & 31) != 8 && (ldk & 31) != 24) ldk += 4;   // conflict-free ds_read_b128 fragment reads (16 rows x 4 k-quads)
        const int ldh = Ep4;                                                 // 16-byte aligned rows: phase 2 re-reads H's fragments per column tile as ds_read_b128
        const size_t fl = (size_t)E * ldk + (size_t)E * ldh + 64 * 2 + (size_t)p.a_cinit * E + 3 * c.N * c.N + 64 + (Kp4 + 3) / 4 + 4;
        // (the fused kernel's per-element MLPs are padded to <= 16; more Hodge powers than two: tiled kernels)
        if (fl * 4 + 64 <= 160 * 1024 && fnet_width(p) <= CCSD_FW && r2_find(0) && p.f_cnum <= 2) {
            fused = true; r.r2_ldk = ldk; r.r2_ldh = ldh; r.r2_lds = fl * 4;
            // the instances with the qm9 geometry compiled in (QM9 = 1), or the whole baked plan (2: affine ScoreNetworkF only)
            const bool qm9 = p.geo_off != 1 && !gen1 && E == CCSD_R2_QM9_E && K == CCSD_R2_QM9_K && p.N == CCSD_R2_QM9_N &&
                             ldk == CCSD_R2_QM9_LDK && ldh == CCSD_R2_QM9_LDH;
            r.r2 = r2_find(!qm9 ? 0 : aff && baked(CCSD_BAKED_QM9_PLAN, CCSD_BAKED_QM9_SIZE) ? 2 : 1);
            if (!r.r2) return set_err(CCSD_ERR_RUNTIME, "k_r2: the qm9-geometry instance is missing from CCSD_R2_LIST_*");
        }
    }
    if (p.h_L > 2) {
        bool affine_values = true;
        for (int l = 0; l + 1 < p.h_L; ++l) affine_values = affine_values && ccsd_hl(p, l).mval.n == 1;
        // (the folded route -- k_r2 hands over one consolidated projection, k_xa chains the M_j -- is built and tested for up to four layers;
        // r2_lds keeps reporting what the fused kernel would have taken)
        if (!affine_values || !fused || p.h_L > 4 || k.hodge_general || r.lg) { r.h_general = 1; fused = false; r.r2 = nullptr; }
    }
    // element-wise rank-2 side (k_ew1): affine ScoreNetworkF without a Hodge Laplacian term (cnum = 1), tiled path, PC samplers
    const bool ew1 = c.is_cc && !fused && aff && p.f_cnum == 1 && !s4 && !r.h_wide;
    r.r2_family = !c.is_cc ? R2_NONE : fused ? R2_FUSED : ew1 ? R2_EW1 : R2_TILED;
    if (p.geo_off != 1) for (const GeoEntry& g : GEO_TABLE) if (E == g.E && K == g.K) r.geo = g.idx;
    if (p.h_L >= 1) {       // narrow layer-0 projection (at most four 16-column tiles): no 64-column padding, K compiled in where listed
        auto p0_find = [&](int kc) {
            for (int i = 0; i < (int)(sizeof(P0_TABLE) / sizeof(P0_TABLE[0])); ++i)
                if (P0_TABLE[i].nt == (p.hl[0].wc + 15) / 16 && P0_TABLE[i].kc == kc) return i;
            return -1;
        };
        if (p.geo_off != 1) r.p0 = p0_find(K);
        if (r.p0 < 0) r.p0 = p0_find(0);
    }
    // tiled rank-2 path (k_gemm_h / k_gemm_p0 / k_hf_score: community_small_CC) with ONE hodge layer: the corrector's rank2 work rides on
    // the layer-0 projection pass (P0Fuse) -- flat-keyed corrector draws, K a multiple of 4 (a Philox group = one 16-byte piece of a row)
    // (plans on the tiled graph-network route take none of the three fusions below: launch_lg has no corrector prologue)
    r.tiled_fuse = !r.lg && r.r2_family == R2_TILED && p.h_L == 1 && (K & 3) == 0 && !s4 && langevin;
    // k_ew1 plans with ONE hodge layer: one read of rank2 per norms pass, one read + one write per predictor pass (P0Fuse modes 3 / 4)
    r.ew1_fuse = !r.lg && ew1 && p.h_L == 1 && (K & 3) == 0 && langevin;
    // community_small geometry: one workgroup per complex, F streamed once (k_gemm_h_full; bit-identical), and ONE fused pass per
    // half-step (k_hp_full) instead of k_gemm_p0<., ., 1 / 2> + k_gemm_h_full.  In the norms pass (mode 1, whose only extra is the
    // noise norm) the fused pass is slower -- 370 us against 129 + 213, the eight waves of the one workgroup a CU holds run in
    // lockstep --: CCSD_HP_FULL_NORMS turns it on for A/B
    const bool full_geo = c.is_cc && E == CCSD_FULL_E && K == CCSD_FULL_K && p.geo_off != 1 && !k.no_h_full;
    r.h_full = full_geo && r.r2_family == R2_TILED && p.f_cnum >= 2;

    // ---- ccsd_sampler_run.  The Langevin apply fuses into the predictor launches of k_r2 plans, of k_ew1 plans whose hodge
    // projections do not depend on the adjacency (at most one hodge layer) and of tiled plans with one hodge layer
    const bool fused_apply = !r.lg && (fused || (ew1 && p.h_L <= 1) || r.tiled_fuse) && !k.no_fused_apply;
    // (LOOP_LANGEVIN means n_corr_steps == 1: ccsd_sampler_run_ex runs it as the multi-iteration branch with its one iteration)
    r.loop = s4 ? LOOP_S4 : !langevin ? LOOP_PRED_ONLY : c.n_corr_steps != 1 ? LOOP_LANGEVIN_MULTI : fused_apply ? LOOP_LANGEVIN_FUSED : LOOP_LANGEVIN;
    // merged k_r2 launches (predictor of step i + rank-2 side of the norms pass of step i + 1): the row-strip instantiation of the
    // kernel (E = 33..36, affine ScoreNetworkF, linear mlp_value), pair-wise block load (K even, E K a multiple of 4)
    // (k_hp_full's mode 2 is the fused apply: only the fused loop's predictor pass carries it)
    if (full_geo && r.tiled_fuse && p.hl[0].wc <= 16 && p.f_cnum == 2 && !k.no_hp_full)
        r.hp_full_modes = (r.loop == LOOP_LANGEVIN_FUSED ? 1u << 2 : 0u) | (k.hp_full_norms ? 1u << 1 : 0u);
    r.merged = r.loop == LOOP_LANGEVIN_FUSED && fused && mt == 3 && rs == 1 && aff && !gen1 && (K & 1) == 0 && ((E * K) & 3) == 0;
    // folded norm sums: every k_r2 plan of the fused loop whose k_r2 reads no adjacency coefficient (the adjpow path of a non-linear
    // mlp_value takes sums[1] / sums[4] inside the kernel, and those are complete only one launch later)
    r.fold_sums = r.loop == LOOP_LANGEVIN_FUSED && fused && !gen1 && !k.no_sum_fold;
    r.corrector_flat = !s4;
    r.predictor_flat = ew1;
    return CCSD_OK;
}
// ---- what also depends on the batch of the call
static inline bool use_h_full(const Route& r, int B) { return r.h_full && B >= 256; }      // at least one complex per CU
static inline bool use_hp_full(const Route& r, int B, int mode) { return B >= 256 && ((r.hp_full_modes >> mode) & 1u); }
#define HP_FULL_LDS ((size_t)(2 * 192 * H_LD + 2 * 16 * H_LD) * 4)       /* dynamic LDS of k_hp_full */
// k_hodge_value[_w]: columns of Rin one workgroup holds in LDS as its [E][cw] slab, and the slab's bytes (the rule of ccsd_k_rank2.h)
static inline int hodge_value_cw(int E) { return E > 128 ? 32 : 64; }
static inline size_t hodge_value_lds(int E) { return (size_t)E * hodge_value_cw(E) * 4; }
// Threads per graph of k_xa, and the instance that takes them.  256 (four waves) is right when the batch fills the chip -- 1024 graphs =
// four co-resident workgroups per CU -- and k_xa is bound by the latency of one graph's critical path either way; when the batch leaves
// a CU with one or two workgroups (B <= 256 / <= 512) the same graph runs on sixteen / eight waves: every per-pair, per-tile and
// per-element loop of the kernel strides by the workgroup's thread count (zinc250k B = 256: 419 -> 293 us per launch;
// community_small_CC B = 512: 418 -> 349 us; ENZYMES_small_CC B = 64: 236 -> 180 us).  Only the instances compiled for 4 waves per SIMD
// without a fixed thread count take more than 256 (CCSD_XA_LIST); CCSD_XA_THREADS overrides the choice (diagnostic) and moves a plan
// off an instance that has its 256 compiled in, to the run-time-geometry twin.
static inline const XaEntry* xa_launch(const Route& r, int B, int* threads) {
    const XaEntry* e = r.xa;
    int t = r.xa_threads;
    if (t == 0) t = e->max_threads == 256 ? 256 : B <= 256 ? 1024 : B <= 512 ? 512 : 256;
    if (e->fixed256 && t != 256) e = r.xa_twin;
    *threads = t > e->max_threads ? e->max_threads : t;
    return e;
}

extern "C" const char* ccsd_last_error(void) { return g_last_error.c_str(); }

extern "C" void ccsd_rank2_dims(const ccsd_config_t* cfg, int32_t* E, int64_t* K) {
    int e = 0; int64_t k = 0;
    if (cfg) ccsd_dims(cfg, &e, &k);
    if (E) *E = e;
    if (K) *K = k;
}

extern "C" size_t ccsd_weight_count(const ccsd_config_t* cfg) {
    PlanD p; PlanBuilder pb;
    size_t n = ccsd_build_plan(cfg, &p, pb);
    if (pb.status != CCSD_OK) { set_err(pb.status, pb.err); return 0; }
    return n;
}

extern "C" int ccsd_debug_stamps(ccsd_plan_t* plan, void* dev_buffer) {
    if (!plan) return set_err(CCSD_ERR_INVALID, "NULL plan");
    plan->dbg = (long long*)dev_buffer;
    return CCSD_OK;
}
extern "C" int ccsd_profile_kernel(ccsd_plan_t* plan, int32_t kernel_id) {
    if (!plan) return set_err(CCSD_ERR_INVALID, "NULL plan");
    if (kernel_id < 0) plan->prof_mask = 0;
    else if (kernel_id < 8) plan->prof_mask |= 1u << kernel_id;
    for (int k = 0; k < 8; ++k) { plan->prof_used[k] = 0; plan->prof_calls[k] = 0; }
    return CCSD_OK;
}
extern "C" int ccsd_profile_stride(ccsd_plan_t* plan, int32_t stride) {
    if (!plan || stride < 1) return set_err(CCSD_ERR_INVALID, "bad argument");
    plan->prof_stride = stride;
    for (int k = 0; k < 8; ++k) plan->prof_calls[k] = 0;
    return CCSD_OK;
}
extern "C" int ccsd_profile_launches(ccsd_plan_t* plan, int32_t kernel_id, int64_t* launches) {
    if (!plan || !launches || kernel_id < 0 || kernel_id >= 8) return set_err(CCSD_ERR_INVALID, "bad argument");
    *launches = (int64_t)(plan->prof_calls[kernel_id] >> 1);       // two marks per launch
    return CCSD_OK;
}
extern "C" int ccsd_profile_read(ccsd_plan_t* plan, int32_t kernel_id, int64_t* launches, double* total_ms) {
    if (!plan || !launches || !total_ms || kernel_id < 0 || kernel_id >= 8) return set_err(CCSD_ERR_INVALID, "bad argument");
    *launches = 0; *total_ms = 0.0;
#ifndef CCSD_EMU
    for (size_t i = 0; i + 1 < plan->prof_used[kernel_id]; i += 2) {
        float ms = 0.f;
        RT_CHECK(hipEventSynchronize(plan->prof_ev[kernel_id][i + 1]));
        RT_CHECK(hipEventElapsedTime(&ms, plan->prof_ev[kernel_id][i], plan->prof_ev[kernel_id][i + 1]));
        *total_ms += ms; *launches += 1;
    }
#endif
    plan->prof_used[kernel_id] = 0;
    return CCSD_OK;
}

extern "C" void ccsd_plan_destroy(ccsd_plan_t* plan) {
    if (!plan) return;
#ifndef CCSD_EMU
    for (int k = 0; k < 8; ++k) for (hipEvent_t e : plan->prof_ev[k]) (void)hipEventDestroy(e);
#endif
    if (plan->d) (void)rt_free(plan->d);
    if (plan->w) (void)rt_free(plan->w);
    if (plan->wp) (void)rt_free(plan->wp);
    if (plan->hpairs) (void)rt_free(plan->hpairs);
    if (plan->edges) (void)rt_free(plan->edges);
    if (plan->cells) (void)rt_free(plan->cells);
    if (plan->init_off) (void)rt_free(plan->init_off);
    delete plan;
}

// the weight blob on the device, ScoreNetworkF's zero-padded blocks behind it (PlanD::f_blk)
static int upload_weights(ccsd_plan* pl, const float* weights, size_t n_weights) {
    const size_t wtotal = pl->h.f_blk >= 0 ? (size_t)pl->h.f_blk + CCSD_FBLK_FLOATS : n_weights;
    RT_CHECK(rt_malloc((void**)&pl->w, wtotal * sizeof(float)));
    RT_CHECK(rt_h2d(pl->w, weights, n_weights * sizeof(float)));
    if (pl->h.f_blk >= 0) {
        std::vector<float> blk(CCSD_FBLK_FLOATS);
        ccsd_pack_fnet_blocks(&pl->h, weights, blk.data());
        RT_CHECK(rt_h2d(pl->w + pl->h.f_blk, blk.data(), blk.size() * sizeof(float)));
    }
    return CCSD_OK;
}
// the max-dynamic-LDS attribute of every kernel of the plan's route that may ask for more than 64 KB
static int set_lds_attributes(const ccsd_plan* pl) {
    const Route& r = pl->rt;
    const int E = pl->h.E;
    const size_t xlds = (size_t)pl->h.xa_lds_floats * 4;
    if (xlds > 64 * 1024) {
        RT_CHECK(rt_set_max_dyn_smem((const void*)r.xa->fn, xlds));
        if (r.xa_twin) RT_CHECK(rt_set_max_dyn_smem((const void*)r.xa_twin->fn, xlds));
    }
    if (r.r2 && r.r2_lds > 64 * 1024) RT_CHECK(rt_set_max_dyn_smem((const void*)r.r2->fn, r.r2_lds));
    if (r.lg && lg_nmlp_lds(pl->h) > 64 * 1024) RT_CHECK(rt_set_max_dyn_smem((const void*)k_lg_nmlp, lg_nmlp_lds(pl->h)));
    if (r.lg && pl->h.hb_L > 1) {
        size_t v = 0;
        for (int l = 0; l + 1 < pl->h.hb_L; ++l) if (lg_hb_dense_lds(pl->hbx[l]) > v) v = lg_hb_dense_lds(pl->hbx[l]);
        if (v > 64 * 1024) RT_CHECK(rt_set_max_dyn_smem((const void*)k_lg_hb_dense, v));
    }
    // (k_lg_hd_dense stays below 64 KB: at most 8 channels of 2 x 16 rows of 33 floats + 256 pairs)
    if (r.lg && r.h_general && hodge_value_lds(E) > 64 * 1024)
        RT_CHECK(rt_set_max_dyn_smem(r.h_wide ? (const void*)k_hodge_value_w : (const void*)k_hodge_value, hodge_value_lds(E)));
#ifndef CCSD_EMU
    if (r.hp_full_modes) {      // k_hp_full: 66.6 KB of dynamic LDS
        RT_CHECK(rt_set_max_dyn_smem((const void*)k_hp_full<CCSD_FULL_E, CCSD_FULL_K, 1>, HP_FULL_LDS));
        RT_CHECK(rt_set_max_dyn_smem((const void*)k_hp_full<CCSD_FULL_E, CCSD_FULL_K, 2>, HP_FULL_LDS));
    }
#endif
    return CCSD_OK;
}

// Plans the networks (ccsd_build_plan), uploads the plan, the weights and their packed copies and the enumeration tables (the builders and
// packers of ccsd_plan.h), resolves the route.  Every failure leaves through the one guard.
extern "C" int ccsd_plan_create(const ccsd_config_t* cfg, const float* weights, size_t n_weights,
                                const ccsd_step_coef_t* step_coef, ccsd_plan_t** out) {
    if (!cfg || !weights || !step_coef || !out) return set_err(CCSD_ERR_INVALID, "NULL argument");
    *out = nullptr;
    std::unique_ptr<ccsd_plan, void (*)(ccsd_plan_t*)> guard(new ccsd_plan(), ccsd_plan_destroy);   // every failure leaves through it
    ccsd_plan* pl = guard.get();
    pl->cfg = *cfg;
    const Knobs& k = pl->knobs = read_knobs();
    PlanBuilder pb;
    pb.lg_force = k.lg_force; pb.xa_pass = k.xa_pass; pb.xa_gch = k.xa_gch; pb.no_mlp_wt = k.no_mlp_wt; pb.verbose = k.verbose;
    pl->nweights = ccsd_build_plan(cfg, &pl->h, pb);
    if (pb.status != CCSD_OK) return set_err(pb.status, pb.err);
    static_cast<PlanRouteOut&>(*pl) = pb;
    pl->rt.lg = pb.lg; pl->rt.h_wide = pb.h_wide;
    pl->h.geo_off = k.geo_off;
    if (pl->nweights != n_weights)
        return set_err(CCSD_ERR_WEIGHTS, "weight blob has " + std::to_string(n_weights) + " floats, config needs " +
                                             std::to_string(pl->nweights));
    if (cfg->predictor != CCSD_PRED_EULER && cfg->predictor != CCSD_PRED_REVERSE && cfg->predictor != CCSD_PRED_S4) return set_err(CCSD_ERR_UNSUPPORTED, "unknown predictor");
    if (cfg->corrector != CCSD_CORR_NONE && cfg->corrector != CCSD_CORR_LANGEVIN) return set_err(CCSD_ERR_UNSUPPORTED, "unknown corrector");
    if (cfg->diff_steps < 1 || cfg->n_corr_steps < 0) return set_err(CCSD_ERR_INVALID, "bad step counts");
    ccsd_fold_fnet(&pl->h, weights);
    pl->coef.assign(step_coef, step_coef + (size_t)cfg->diff_steps * 3);
    const int E = pl->h.E;
    const std::vector<unsigned char> edges = ccsd_edge_table(cfg->N, E);
    std::vector<unsigned long long> cells;
    if (!ccsd_cell_table(cfg, pl->h.K, &cells)) return set_err(CCSD_ERR_INVALID, "cell enumeration mismatch");
    RT_CHECK(rt_malloc((void**)&pl->d, sizeof(PlanD)));
    RT_CHECK(rt_h2d(pl->d, &pl->h, sizeof(PlanD)));
    if (int st = upload_weights(pl, weights, n_weights)) return st;
    {
        const std::vector<float> packed = ccsd_pack_weights(pl->h, *pl, pl->rt.lg, weights);
        RT_CHECK(rt_malloc((void**)&pl->wp, packed.size() * sizeof(float)));
        RT_CHECK(rt_h2d(pl->wp, packed.data(), packed.size() * sizeof(float)));
    }
    if (pl->h.h_L > 1 && !pl->rt.lg) {     // (k_xa's pair table; the tiled route walks tiles)
        if (E > 255) return set_err(CCSD_ERR_UNSUPPORTED, "dense hodge layer needs E <= 255");
        const std::vector<unsigned char> hp = ccsd_hodge_pairs(E);
        RT_CHECK(rt_malloc((void**)&pl->hpairs, hp.size()));
        RT_CHECK(rt_h2d(pl->hpairs, hp.data(), hp.size()));
    }
    RT_CHECK(rt_malloc((void**)&pl->edges, edges.size()));
    RT_CHECK(rt_h2d(pl->edges, edges.data(), edges.size()));
    RT_CHECK(rt_malloc((void**)&pl->cells, cells.size() * sizeof(unsigned long long)));
    RT_CHECK(rt_h2d(pl->cells, cells.data(), cells.size() * sizeof(unsigned long long)));
    if (int st = resolve_route(pl)) return st;
    if (int st = set_lds_attributes(pl)) return st;
    if (k.dump_plan) ccsd_dump_plan(pl->h, k.dump_plan, k.dump_plan_name ? k.dump_plan_name : "QM9");
    *out = guard.release();
    return CCSD_OK;
}

#define CCSD_P_SPLITS 8     /* most K slices k_gemm_p is split into when its row tiles cannot fill the chip */

// ---------------- workspace ----------------
struct Workspace {
    unsigned long long* offbits;
    unsigned char *mfr, *mfl;       // flag masks of every complex as byte tables (k_masktab): [B][Kp], [B][Ep]
    int Kp, Ep;
    float *H, *P0, *P1, *U1, *acoef, *net_x, *net_adj, *net_r, *norm2, *part, *sums, *chan, *zpart, *part2;
    float* partb;                   // folded norm sums (Route::fold_sums): the second [B][2] buffer of k_r2's partials -- step parity picks w.part or this
                                    // one; it is part2, which the folding loop does not use otherwise (the workspace does not grow)
    float* psplit; size_t psplit_floats;   // K slices of the layer-1 projection (k_gemm_p with few row tiles)
    float *P0b, *P1b, *U1b;         // second set of hodge projections (merged k_r2 launch: the next norms pass's)
    int ntiles, nchunk;
    float *hgH, *hgR[2], *hgP[CCSD_MAXHL + CCSD_MAXHLX - 1];   // general hodge stack: dumped H^l, R_l (two alternating), P_l of the layers >= 1
    size_t hg_hstride;
    // tiled graph-network route (launch_lg): channel stack [B][a_fdim][N][N]; attention [B][cin][N][N]; D^-1/2 [B][cin][N]; X W and the
    // GCN output [B][cin][N][cp] (Q | K | V side by side); node features (ping-pong) [B][N][max(F, nhid)]; ScoreNetworkX's concatenation
    // [B][N][x_fdim], its X W [B][N][nhid], its masked net [B][N][F]; k_lg_fin's per-tile norm partials [B][lg_tiles][2]
    float *lg_S, *lg_att, *lg_dis, *lg_Y, *lg_QKV, *lg_x[2], *lg_xcat, *lg_xY, *lg_xnet, *lg_part;
    int lg_tiles;
    // ... ScoreNetworkA_Base_CC: hidden rows of a layer's BaselineBlocks [B][cin][E][hid]; the dense output [B][cout][E][E] of a layer
    // but the last (ONE buffer: the next layer's hidden rows are all that reads it, and they are complete before the next dense
    // output is written); per-sample strides in floats
    float *lg_hbg, *lg_hbH;
    size_t lg_hbg_stride, lg_hbH_stride;
    // ... ScoreNetworkA_CC stacks of two or more layers: the Q | K rows of a layer [B][cin][E][2 adim]; D^-1/2 of a dense input
    // [B][cin][E]; the per-edge factors of a raw P_1 [B][2][E]; the dense output [B][cout][E][E] of a layer but the last (ONE buffer, see
    // ccsd_k_lg.h; the general stack's hgH where that is carved); per-sample strides in floats
    float *lg_hdq, *lg_hdd, *lg_hdpc, *lg_hdH;
    size_t lg_hdq_stride, lg_hdH_stride;
    ccsd_state_t third;             // LOOP_LANGEVIN_MULTI with more than one inner iteration: the second corrector iterate of ccsd_sampler_run
    size_t bytes;
    MaskTab masks() const { return MaskTab{mfr, mfl, Kp, Ep}; }
};
// What one pass (a norms pass, a predictor pass, one ccsd_score) hands from launcher to launcher.
struct Pass {
    const float* h_src = nullptr;   // the rank2 block w.H was computed from in this pass (k_hp_full leaves H beside P_0): launch_h skips for it
    int p1_raw = 0;                 // who filled P1 last: k_r2 with the raw factors (1, see k_r2) or k_gemm_p with the finished projections (0)
};
static inline int r2_p1_raw(const PlanD& p) { return p.h_L > 1 && p.hl[0].mval.n == 1; }
static Workspace carve_ws(const ccsd_plan* pl, int B, void* base) {
    const PlanD& p = pl->h;
    Workspace w{};
    size_t o = 0;
    auto take = [&](size_t nbytes) { size_t r = o; o += (nbytes + 255) / 256 * 256; return base ? (char*)base + r : (char*)nullptr; };
    w.offbits = (unsigned long long*)take((size_t)B * 8);
    const size_t E = p.E, K = p.K;
    w.Kp = p.is_cc ? (p.K + 3) & ~3 : 0; w.Ep = p.is_cc ? (p.E + 3) & ~3 : 0;
    w.mfr = (unsigned char*)take((size_t)B * w.Kp);
    w.mfl = (unsigned char*)take((size_t)B * w.Ep);
    w.H = (float*)take(p.is_cc ? (size_t)B * E * h_ld((int)E) * 4 * (p.f_cnum > 2 ? p.f_cnum - 1 : 1) : 0);   // H, H^2, ... (cnum > 2: one slab per power)
    w.P0 = (float*)take(p.h_L > 0 ? (size_t)B * E * p.hl[0].wc * 4 : 0);
    w.P1 = (float*)take(p.h_L > 1 ? (size_t)B * E * p.h_pw * 4 : 0);
    w.U1 = (float*)take(p.h_L > 1 ? (size_t)B * p.h_pw * 4 : 0);
    // K slices of k_gemm_p (always split: batch-invariant summation order; the step-wise score / norms calls of fused-rank-2 plans use k_gemm_p too)
    w.psplit_floats = p.h_L > 1 ? (size_t)CCSD_P_SPLITS * B * E * p.h_pw : 0;
    w.psplit = (float*)take(w.psplit_floats * 4);
    const bool two = pl->rt.r2_family == R2_FUSED;
    w.P0b = (float*)take(two && p.h_L > 0 ? (size_t)B * E * p.hl[0].wc * 4 : 0);
    w.P1b = (float*)take(two && p.h_L > 1 ? (size_t)B * E * p.h_pw * 4 : 0);
    w.U1b = (float*)take(two && p.h_L > 1 ? (size_t)B * p.h_pw * 4 : 0);
    w.acoef = (float*)take(p.h_L > 1 ? (size_t)B * p.a_cinit * E * 4 : 0);
    if (pl->rt.h_general) {
        int cmax = 1;
        for (int l = 0; l + 1 < p.h_L; ++l) cmax = ccsd_hl(p, l).cout > cmax ? ccsd_hl(p, l).cout : cmax;
        w.hg_hstride = (size_t)cmax * E * E;
        w.hgH = (float*)take((size_t)B * w.hg_hstride * 4);
        w.hgR[0] = (float*)take((size_t)B * E * K * 4);
        w.hgR[1] = (float*)take((size_t)B * E * K * 4);
        for (int l = 1; l < p.h_L; ++l) w.hgP[l - 1] = (float*)take((size_t)B * E * ccsd_hl(p, l).wc * 4);
    }
    w.net_x = (float*)take((size_t)B * p.N * p.F * 4);
    w.net_adj = (float*)take((size_t)B * p.N * p.N * 4);
    w.net_r = (float*)take(p.is_cc ? (size_t)B * E * K * 4 : 0);
    w.norm2 = (float*)take((size_t)B * 4 * 4);
    w.ntiles = p.is_cc ? ((p.K + T_BN - 1) / T_BN) * ((p.E + T_BM - 1) / T_BM) : 0;
    w.nchunk = p.is_cc ? (int)((((size_t)p.E * p.K + 3) / 4 + CCSD_NN_CH - 1) / CCSD_NN_CH) : 0;   // k_noise_norm / k_ew1: chunks of flat groups per sample
    { int np = w.ntiles > w.nchunk ? w.ntiles : w.nchunk; if ((int)E > np) np = (int)E;      // (per-row partials of P0Fuse mode 3)
      w.part = (float*)take((size_t)B * (np ? np : 1) * 2 * 4); }
    w.zpart = (float*)take((size_t)B * ((size_t)w.nchunk > E ? (size_t)w.nchunk : E ? E : 1) * 4);   // chunk partials of k_noise_norm, or the row partials of P0Fuse mode 1
    w.part2 = (float*)take((size_t)B * 2 * 4);
    w.partb = w.part2;          // (k_normpart's output: never launched on a pass k_r2 serves, and a folding loop has no other)
    w.sums = (float*)take(64);
    w.chan = (float*)take(p.chan_global ? (size_t)B * p.chan_rows * p.N * p.N * 4 : 0);
    if (pl->rt.lg) {
        const size_t N = p.N, NN = N * N;
        int cin = 1, cp = 1, fx = p.F > p.x_nhid ? p.F : p.x_nhid;
        for (int l = 0; l < p.a_L; ++l) {
            if (p.al[l].cin > cin) cin = p.al[l].cin;
            if (p.al[l].cp > cp) cp = p.al[l].cp;
            if (p.al[l].fout > fx) fx = p.al[l].fout;
        }
        w.lg_tiles = (int)((NN + CCSD_LG_FIN_ROWS - 1) / CCSD_LG_FIN_ROWS);
        w.lg_S = (float*)take((size_t)B * p.a_fdim * NN * 4);
        w.lg_att = (float*)take((size_t)B * cin * NN * 4);
        w.lg_dis = (float*)take((size_t)B * cin * N * 4);
        w.lg_Y = (float*)take((size_t)B * cin * N * cp * 4);
        w.lg_QKV = (float*)take((size_t)B * cin * N * cp * 4);
        w.lg_x[0] = (float*)take((size_t)B * N * fx * 4);
        w.lg_x[1] = (float*)take((size_t)B * N * fx * 4);
        w.lg_xcat = (float*)take((size_t)B * N * p.x_fdim * 4);
        w.lg_xY = (float*)take((size_t)B * N * p.x_nhid * 4);
        w.lg_xnet = (float*)take((size_t)B * N * p.F * 4);
        w.lg_part = (float*)take((size_t)B * w.lg_tiles * 2 * 4);
        if (p.hb_L) {
            size_t g = 0, hd = 0;
            for (int l = 0; l < p.hb_L; ++l) {
                const HodgeBaseD& h = pl->hbx[l];
                if ((size_t)h.cin * E * h.hid > g) g = (size_t)h.cin * E * h.hid;
                if (l + 1 < p.hb_L && (size_t)h.cout * E * E > hd) hd = (size_t)h.cout * E * E;
            }
            w.lg_hbg_stride = g; w.lg_hbH_stride = hd;
            w.lg_hbg = (float*)take((size_t)B * g * 4);
            w.lg_hbH = (float*)take((size_t)B * hd * 4);
        }
        if (p.h_L > 1) {
            size_t q = 0, d = 0, hd = 0;
            for (int l = 0; l < p.h_L; ++l) {
                const HodgeLayerD& h = ccsd_hl(p, l);
                if ((size_t)h.cin * E * 2 * h.adim > q) q = (size_t)h.cin * E * 2 * h.adim;
                if (l > 0 && (size_t)h.cin * E > d) d = (size_t)h.cin * E;
                if (l + 1 < p.h_L && (size_t)h.cout * E * E > hd) hd = (size_t)h.cout * E * E;
            }
            w.lg_hdq_stride = q;
            w.lg_hdq = (float*)take((size_t)B * q * 4);
            w.lg_hdd = (float*)take((size_t)B * d * 4);
            w.lg_hdpc = (float*)take((size_t)B * 2 * E * 4);
            if (pl->rt.h_general) { w.lg_hdH = w.hgH; w.lg_hdH_stride = w.hg_hstride; }
            else { w.lg_hdH_stride = hd; w.lg_hdH = (float*)take((size_t)B * hd * 4); }
        }
    }
    if (pl->rt.loop == LOOP_LANGEVIN_MULTI && pl->cfg.n_corr_steps > 1) {      // (last: no plan with n_steps == 1 moves)
        w.third.x = (float*)take((size_t)B * p.N * p.F * 4);
        w.third.adj = (float*)take((size_t)B * p.N * p.N * 4);
        w.third.rank2 = p.is_cc ? (float*)take((size_t)B * E * K * 4) : nullptr;
    }
    w.bytes = o;
    return w;
}
extern "C" size_t ccsd_workspace_bytes(const ccsd_plan_t* plan, int32_t B) {
    if (!plan || B < 1) return 0;
    return carve_ws(plan, B, nullptr).bytes;
}

static int grid_for(long long n, int block) {
    long long g = (n + block - 1) / block;
    if (g > 2048) g = 2048;   // grid-stride the rest
    if (g < 1) g = 1;
    return (int)g;
}

static int check_common(const ccsd_plan* pl, int B, const void* flags, void* ws, size_t ws_bytes, Workspace& w) {
    if (!pl) return set_err(CCSD_ERR_INVALID, "NULL plan");
    if (B < 1) return set_err(CCSD_ERR_INVALID, "B must be >= 1");
    if (!flags) return set_err(CCSD_ERR_INVALID, "NULL flags");
    if (ws) w = carve_ws(pl, B, ws);       // the one carve of the call
    if (!ws || ws_bytes < w.bytes) return set_err(CCSD_ERR_WORKSPACE, "workspace too small");
    return CCSD_OK;
}
static int check_state(const ccsd_plan* pl, const ccsd_state_t* s, const char* what) {
    if (!s || !s->x || !s->adj || (pl->h.is_cc && !s->rank2)) return set_err(CCSD_ERR_INVALID, std::string("NULL tensor in ") + what);
    return CCSD_OK;
}

static int launch_flagbits(const ccsd_plan* pl, int B, const float* flags, Workspace& w, void* stream) {
    if (pl->rt.lg && !pl->h.is_cc) return CCSD_OK;       // (64-bit node masks feed only the rank-2 tables; graph-only plans of the tiled route go past 64 nodes)
    CCSD_LAUNCH(k_flagbits, dim3(grid_for(B, 256)), dim3(CCSD_NTHREADS), 0, stream, flags, w.offbits, B, pl->h.N);
    LAUNCH_CHECK();
    if (pl->h.is_cc) {      // (consumers: k_ew1, k_langevin_apply, k_noise_norm; the fused rank-2 kernel builds its own masks in LDS)
        CCSD_LAUNCH(k_masktab, dim3(grid_for((long long)B * (w.Kp + w.Ep), 256)), dim3(CCSD_NTHREADS), 0, stream,
                    (const unsigned long long*)w.offbits, (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells, w.mfr, w.mfl,
                    B, pl->h.E, pl->h.K, w.Kp, w.Ep);
        LAUNCH_CHECK();
    }
    return CCSD_OK;
}

// H = F F^T (ScoreNetworkF) from `rank2`
static int launch_h(const ccsd_plan* pl, int B, const float* rank2, Pass& ps, Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    if (!p.is_cc || p.f_cnum < 2) return CCSD_OK;
    if (ps.h_src == rank2) return CCSD_OK;
    const bool full = use_h_full(pl->rt, B);        // (a GPU-only kernel: the emulation launches k_gemm_h)
    const int nth_ = (p.E + T_BM - 1) / T_BM;
    dim3 g(xcd_grid(B, nth_ * (nth_ + 1) / 2));
    prof_mark(pl, KID_GEMM_H, stream);
#ifndef CCSD_EMU
    if (full && pl->knobs.split_bf16 == 3) hipLaunchKernelGGL((k_gemm_h_full<CCSD_FULL_E, CCSD_FULL_K, 2>), dim3(B), dim3(256), 0, (hipStream_t)stream, rank2, w.H, p.f_hmask);
    else if (full) hipLaunchKernelGGL((k_gemm_h_full<CCSD_FULL_E, CCSD_FULL_K>), dim3(B), dim3(256), 0, (hipStream_t)stream, rank2, w.H, p.f_hmask);
    else
#endif
    {
        (void)full;
#define H_GO(EC_, KC_) CCSD_LAUNCH((k_gemm_h<EC_, KC_>), g, dim3(CCSD_NTHREADS), 0, stream, rank2, w.H, p.E, p.K, p.f_hmask, B)
        GEO_EK(pl->rt.geo, H_GO);
#undef H_GO
    }
    prof_mark(pl, KID_GEMM_H, stream);
    LAUNCH_CHECK();
    for (int j = 2; j < p.f_cnum; ++j) {       // H^j = H^(j-1) . H  (pow_tensor_cc, cc_utils.py:972-977)
        const size_t slab = (size_t)B * p.E * h_ld(p.E);
        const int nt = (p.E + 15) / 16, per = CCSD_NTHREADS >= 64 ? CCSD_NTHREADS / 64 : 1;
        CCSD_LAUNCH(k_gemm_pow, dim3((nt * nt + per - 1) / per, 1, B), dim3(CCSD_NTHREADS), 0, stream,
                    (const float*)(w.H + (size_t)(j - 2) * slab), (const float*)w.H, w.H + (size_t)(j - 1) * slab, p.E);
        LAUNCH_CHECK();
    }
    return CCSD_OK;
}
// out = R Wcat of hodge layer `h` for a materialised R: plain k_gemm_p (on wide plans too), whole K, no acoef.  The caller checks the launch
static void launch_gemm_p_whole(const ccsd_plan* pl, int B, const float* R, const HodgeLayerD& h, float* out, const Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    const int rows = B * p.E;
    CCSD_LAUNCH(k_gemm_p, dim3((h.wc + T_BN - 1) / T_BN, (rows + T_BM - 1) / T_BM, 1), dim3(CCSD_NTHREADS), 0, stream, R, (const float*)pl->w, out,
                rows, p.E, p.K, h.wc, h.wcat, 0, h.mval, h.cin, (const float*)nullptr, (const unsigned long long*)w.offbits,
                (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells, p.K);
}
// Rout = fl fr mlp_value_h(cat_c H_c Rin) (k_hodge_value[_w]): H [cin][E][E] per sample, h_stride floats apart; nullptr: layer 0's diagonal form, a_c o Rin with `acoef`
static void launch_hodge_value(const ccsd_plan* pl, int B, const float* Rin, const float* H, size_t h_stride, const float* acoef,
                              const HodgeLayerD& h, float* Rout, const Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    const int cw = hodge_value_cw(p.E);
    CCSD_LAUNCH(pl->rt.h_wide ? k_hodge_value_w : k_hodge_value, dim3((p.K + cw - 1) / cw, B), dim3(CCSD_NTHREADS), hodge_value_lds(p.E), stream, Rin, H,
                (int)h_stride, acoef, (const float*)pl->w, h.mval, h.cin, Rout, p.E, p.K, cw,
                (const unsigned long long*)w.offbits, (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells);
}
// Layer l >= 2 of the general hodge stack, with H^(l-1) (the dense output of layer l - 2) in w.hgH:
// R_l = fl fr mlp_value_(l-1)(cat_c H^(l-1)_c R_(l-1)) into the other of the two R buffers, then P_l = R_l Wcat_l.  launch_p left R_1.
static int hodge_stack_layer(const ccsd_plan* pl, int B, int l, Workspace& w, void* stream) {
    float* Rl = w.hgR[(l - 1) & 1];
    launch_hodge_value(pl, B, w.hgR[(l - 2) & 1], w.hgH, w.hg_hstride, nullptr, ccsd_hl(pl->h, l - 1), Rl, w, stream);
    LAUNCH_CHECK();
    launch_gemm_p_whole(pl, B, Rl, ccsd_hl(pl->h, l), w.hgP[l - 1], w, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}
// The partial buffers of a loop step with folded norm sums (Route::fold_sums; part_in == nullptr: no fold, w.part throughout):
// part_in holds this step's rank-2 partials, part_next takes the next step's.
struct SumFold { const float* part_in = nullptr; float* part_next = nullptr; };
static int launch_r2(const ccsd_plan* pl, int B, const float* rank2, const float* adj, const float* flags, int want_p,
                     RankEpi& ep, NoiseArgs& na, Pass& ps, Workspace& w, void* stream, const CorrFuse* cf, int merge_draw,
                     const SumFold* fold = nullptr);
// hodge projections for ScoreNetworkA_CC from (adj, rank2)
// fuse (tiled path, h_L == 1; Route::tiled_fuse): the Langevin corrector's element-wise work on rank2 rides on the layer-0 projection
// pass -- mode 1: the noise norm of the corrector's draw per row (-> fuse->zrow), mode 2: the corrector apply (corrected rank2 -> fuse->f1,
// which the projection is then taken of).  See P0Fuse (ccsd_k_rank2.h).
static int launch_p(const ccsd_plan* pl, int B, const float* adj, const float* rank2, Pass& ps, Workspace& w, void* stream, const P0Fuse* fuse = nullptr) {
    const PlanD& p = pl->h;
    const Route& rt = pl->rt;
    if (p.h_L < 1) return CCSD_OK;
    if (p.h_L > 2 && !rt.h_general) {
        // more than two hodge layers: k_xa's general layer loop consumes the factors only the fused rank-2 kernel produces
        // (plan creation guarantees it exists); its ScoreNetworkF output lands in the net_r scratch, which every caller
        // of launch_p overwrites afterwards
        RankEpi ep{};
        ep.mode = MODE_SCORE; ep.sscale = 0.f; ep.out = w.net_r;
        NoiseArgs na0{};
        return launch_r2(pl, B, rank2, adj, nullptr, 1, ep, na0, ps, w, stream, nullptr, -1);
    }
    ps.p1_raw = 0;
    const int rows = B * p.E;
    // the corrector's work riding on the pass (modes 1 / 2) on the community_small geometry: ONE kernel streams the block once and leaves
    // P_0, H and the noise norm / the corrected state (k_hp_full; P_0 and H bit-identical to the two-kernel route); the launch_h that
    // follows in the caller, asked for H of the block this pass took it from (mode 2: the corrected state in fuse->f1), finds it done
    const bool hp_full = fuse && use_hp_full(rt, B, fuse->mode);        // (a GPU-only kernel: the emulation takes the two-kernel route)
#ifndef CCSD_EMU
    if (hp_full) {
        const HodgeLayerD& h = p.hl[0];
        const float* WT = (const float*)pl->wp + h.wcatT;
        prof_mark(pl, KID_GEMM_H, stream);
        if (fuse->mode == 1)
            hipLaunchKernelGGL((k_hp_full<CCSD_FULL_E, CCSD_FULL_K, 1>), dim3(B), dim3(512), HP_FULL_LDS, (hipStream_t)stream, rank2, WT, w.H, w.P0, h.wc, p.f_hmask, *fuse);
        else
            hipLaunchKernelGGL((k_hp_full<CCSD_FULL_E, CCSD_FULL_K, 2>), dim3(B), dim3(512), HP_FULL_LDS, (hipStream_t)stream, rank2, WT, w.H, w.P0, h.wc, p.f_hmask, *fuse);
        prof_mark(pl, KID_GEMM_H, stream);
        LAUNCH_CHECK();
        ps.h_src = fuse->mode == 2 ? fuse->f1 : rank2;
        return CCSD_OK;
    }
#endif
    (void)hp_full;
    {
        const HodgeLayerD& h = p.hl[0];
        prof_mark(pl, KID_GEMM_P, stream);
        P0Fuse pf{};
        if (fuse) pf = *fuse;
#ifndef CCSD_EMU
        if (rt.p0 >= 0)      // narrow projections (a GPU-only kernel: the emulation launches the wide one)
            hipLaunchKernelGGL(P0_TABLE[rt.p0].fn[pf.mode], dim3((rows + T_BM - 1) / T_BM), dim3(256), 0, (hipStream_t)stream, rank2,
                               (const float*)pl->wp + h.wcatT, w.P0, rows, p.K, (p.K + 31) & ~31, h.wc, pf);
        else
#endif
        {
            const float* src = rank2;
            if (pf.mode) {      // (host emulation / wide projections: the corrector work as an element-wise pass of its own)
                CCSD_LAUNCH(k_p0_fuse_ew, dim3(grid_for(rows, 256)), dim3(CCSD_NTHREADS), 0, stream, rank2, pf, rows, p.K);
                LAUNCH_CHECK();
                if (pf.mode == 2 || pf.mode == 4) src = pf.f1;
            }
            launch_gemm_p_whole(pl, B, src, h, w.P0, w, stream);
        }
        prof_mark(pl, KID_GEMM_P, stream);
        LAUNCH_CHECK();
    }
    if (p.h_L > 1) {
        CCSD_LAUNCH(k_edgecoef, dim3(B), dim3(CCSD_NTHREADS), (size_t)3 * p.N * p.N * 4, stream, adj, w.acoef, p.N, p.E,
                    p.a_cinit, (const unsigned char*)pl->edges);
        LAUNCH_CHECK();
        const HodgeLayerD& h0 = p.hl[0];
        const HodgeLayerD& h = p.hl[1];
        dim3 g((h.wc + T_BN - 1) / T_BN, (rows + T_BM - 1) / T_BM, 1);
        // K is ALWAYS split into the same slices (up to CCSD_P_SPLITS, one workgroup grid layer each, summed in a fixed order by
        // k_sum_splits): the slicing is a function of (K, T_BK) alone, so the summation order of a row of P_1 -- hence every score
        // downstream -- does not depend on the batch or shard size (a sharded run, a divide_batch chunk and the whole batch agree
        // per sample).  Small batches need the slices anyway to fill the chip (ENZYMES_small_CC at B = 64 has 66 row tiles).
        const int nslab = (p.K + T_BK - 1) / T_BK;
        int S = CCSD_P_SPLITS < nslab ? CCSD_P_SPLITS : nslab;
        if ((size_t)S * rows * h.wc > w.psplit_floats) S = 1;     // (cannot happen: carve_ws sizes the slices for every batch)
        const int kchunk = ((nslab + S - 1) / S) * T_BK;
        S = (p.K + kchunk - 1) / kchunk;
        g.z = S;
        float* P1 = rt.h_general ? w.hgP[0] : w.P1;
        CCSD_LAUNCH(rt.h_wide ? k_gemm_p_w : k_gemm_p, g, dim3(CCSD_NTHREADS), 0, stream, rank2, (const float*)pl->w, S > 1 ? w.psplit : P1, rows, p.E, p.K, h.wc,
                    h.wcat, 1, h0.mval, h0.cin, (const float*)w.acoef, (const unsigned long long*)w.offbits,
                    (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells, kchunk);
        LAUNCH_CHECK();
        if (S > 1) {
            const long long n = (long long)rows * h.wc;
            CCSD_LAUNCH(k_sum_splits, dim3(grid_for(n, 256)), dim3(CCSD_NTHREADS), 0, stream, (const float*)w.psplit, P1, n, S);
            LAUNCH_CHECK();
        }
        if (rt.h_general) {
            // R_1 = fl fr mlp_value_0(a_c o rank2), materialised for the layers behind it (launch_xa / launch_lg go on from here)
            launch_hodge_value(pl, B, rank2, nullptr, 0, w.acoef, h0, w.hgR[0], w, stream);
            LAUNCH_CHECK();
        }
    }
    return CCSD_OK;
}
static int launch_lg(const ccsd_plan* pl, int B, XaArgs& xa, NoiseArgs& na, Workspace& w, void* stream);
static int launch_xa(const ccsd_plan* pl, int B, XaArgs& xa, NoiseArgs& na, const Pass& ps, Workspace& w, void* stream, bool set_b = false) {
    const Route& rt = pl->rt;
    xa.P0 = set_b ? w.P0b : w.P0;
    xa.P1 = set_b ? w.P1b : w.P1; xa.U1 = set_b ? w.U1b : w.U1; xa.p1_raw = ps.p1_raw;
    if (rt.lg) return launch_lg(pl, B, xa, na, w, stream);
    xa.chan_ws = w.chan;
    xa.dbg = pl->dbg ? pl->dbg + 32 : nullptr;
    int xa_threads;
    const XaEntry* inst = xa_launch(rt, B, &xa_threads);
    prof_mark(pl, KID_XA, stream);
    xa.wp = pl->wp; xa.hpairs = pl->hpairs;
    xa.prio_mode = pl->knobs.xa_prio;
    const dim3 xblk(CCSD_NTHREADS == 1 ? 1 : xa_threads);
    const size_t xlds = (size_t)pl->h.xa_lds_floats * 4;
#define XA_LAUNCH(XA_) CCSD_LAUNCH(inst->fn, dim3(B), xblk, xlds, stream, (const PlanD*)pl->d, (const float*)pl->w, (const unsigned char*)pl->edges, XA_, na)
    if (rt.h_general) {
        // general hodge stack: layer l >= 2 projects R_l = fl fr mlp_value_(l-1)(cat_c H^(l-1)_c R_(l-1)).  H^(l-1) is the dense output of
        // layer l - 2 inside k_xa: a launch that stops behind it dumps it, hodge_stack_layer forms R_l and projects it -- then the next
        // layer, and at last the full launch with every P_l delivered.  (launch_p left P_0, P_1 and R_1.)
        const PlanD& p = pl->h;
        if (rt.xa_variant != XA_GEN) return set_err(CCSD_ERR_RUNTIME, "general hodge stack needs k_xa<., XA_GEN>");
        xa.pdirect = 1;
        for (int l = 1; l < p.h_L; ++l) xa.Pd[l - 1] = w.hgP[l - 1];
        for (int l = 2; l < p.h_L; ++l) {
            XaArgs pre = xa;
            pre.hdump_layer = l - 1; pre.hdump = w.hgH; pre.hdump_stride = (int)w.hg_hstride;
            XA_LAUNCH(pre);
            LAUNCH_CHECK();
            if (int st = hodge_stack_layer(pl, B, l, w, stream)) return st;
        }
    }
    XA_LAUNCH(xa);
#undef XA_LAUNCH
    prof_mark(pl, KID_XA, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}
// Tiled graph-network route (ccsd_k_lg.h): ScoreNetworkX on (xX, adjX) and ScoreNetworkA on (xA, adjA) as a sequence of launches over
// the workspace (LgWs fields of Workspace), then the epilogues of k_xa's contract (mode, coefficients, mean pointers, norm2[b][4]).
// Combinatorial-complex plans: ScoreNetworkA_CC (xa.P0 holds the layer-0 hodge projections launch_p / k_r2 left; two layers: xa.P1 the
// second layer's, finished or as k_r2's raw factors with xa.U1; three or more: the general hodge stack, whose layer loop runs here), or
// ScoreNetworkA_Base_CC (its hodge branch reads only the adjacency powers).
// Plans on this route never fuse the corrector apply into this pass (resolve_route), so a CorrFuse here is an error.
static int launch_lg(const ccsd_plan* pl, int B, XaArgs& xa, NoiseArgs& na, Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    if (xa.cf.on) return set_err(CCSD_ERR_RUNTIME, "tiled graph-network route: no fused corrector apply");
    const int N = p.N, F = p.F, NN = N * N, H = p.x_nhid, XF = p.x_fdim;
    const int rt = (N + 15) / 16, gt = (N + CCSD_LG_GT - 1) / CCSD_LG_GT, at = (N + CCSD_LG_AT - 1) / CCSD_LG_AT;
    const dim3 blk(CCSD_NTHREADS);
    auto cdiv = [](int a, int b_) { return (a + b_ - 1) / b_; };
    prof_mark(pl, KID_XA, stream);
    if (xa.do_x) {
        // ScoreNetworkX (ScoreNetwork_X.py:102-132): depth x tanh(DenseGCNConv) on adjX, concatenated behind x, final MLP per node
        CCSD_LAUNCH(k_lg_dis, dim3(grid_for(N, 256), B), blk, 0, stream, xa.adjX, (long long)NN, 0, 1, N, w.lg_dis);
        CCSD_LAUNCH(k_lg_put, dim3(grid_for((long long)B * N * F, 256)), blk, 0, stream, xa.xX, F, w.lg_xcat, XF, B * N);
        for (int l = 0; l < p.x_depth; ++l) {
            const int fin = l ? H : F;
            const float* src = l ? w.lg_xcat + F + (l - 1) * H : xa.xX;
            CCSD_LAUNCH(k_lg_xw, dim3(grid_for((long long)N * H, 256), B), blk, 0, stream, src, (long long)N * (l ? XF : F), l ? XF : F, fin,
                        (const float*)pl->w + p.x_gw[l], 0, H, 1, N, (const float*)w.lg_dis, w.lg_xY);
            CCSD_LAUNCH(k_lg_gcn, dim3(gt * cdiv(H, CCSD_LG_GT), 1, B), blk, 0, stream, xa.adjX, (long long)NN, 0, (const float*)w.lg_xY,
                        (const float*)w.lg_dis, (const float*)pl->w + p.x_gb[l], 0, H, H, 1, N, w.lg_xcat, (long long)N * XF, 0, XF, F + l * H, 1);
        }
        CCSD_LAUNCH(k_lg_nmlp, dim3(rt, B), blk, lg_nmlp_lds_of(p.x_fin), stream, p.x_fin, (const float*)pl->w,
                    (LgGather{w.lg_xcat, (long long)N * XF, 0, XF, 0, XF}), N, xa.flags, 0, w.lg_xnet);
        LAUNCH_CHECK();
    }
    if (xa.do_a) {
        // ScoreNetworkA (ScoreNetwork_A.py:505-541): channel stack [A, A^2, ..] + every AttentionLayer's output channels, final MLP per entry
        const long long ss = (long long)p.a_fdim * NN;
        for (int c = 0; c < p.a_cinit; ++c)
            CCSD_LAUNCH(k_lg_pow, dim3(grid_for(NN, 256), B), blk, 0, stream, xa.adjA, w.lg_S, ss, N, c);
        if (p.h_L == 1) {
            // hodge branch of ScoreNetworkA_CC, one layer: per-edge arithmetic on the powers and P_0, scattered behind the graph channels
            if (!xa.P0) return set_err(CCSD_ERR_RUNTIME, "tiled graph-network route: no hodge projections");
            if (pl->rt.h_wide) {
                CCSD_LAUNCH(k_lg_hodge1_w, dim3(grid_for(p.E, 256), B), blk, 0, stream, p.hl[0], pl->hdm[0], 1.0f / (float)sqrt((double)p.K), (const float*)pl->w,
                            (const float*)pl->wp, (const unsigned char*)pl->edges, xa.P0, w.lg_S, ss, p.a_nch_graph, N, p.E, xa.flags);
            } else {
                CCSD_LAUNCH(k_lg_hodge1, dim3(grid_for(p.E + N, 256), B), blk, 0, stream, p.hl[0], 1.0f / (float)sqrt((double)p.K), (const float*)pl->w,
                            (const unsigned char*)pl->edges, xa.P0, w.lg_S, ss, p.a_nch_graph, N, p.E, xa.flags);
            }
        }
        if (p.h_L > 1) {
            // hodge branch of ScoreNetworkA_CC, two or more layers (k_lg_hd_*): layer 0's Q | K rows per edge; per layer l but the last its
            // dense E x E output H^(l+1) (the diagonal goes to the stack), D^-1/2 of it and the next layer's Q | K rows from it and P_(l+1);
            // the last layer on its diagonal only.  General stack (three or more layers; launch_p left P_0, P_1 and R_1): while H^j is in
            // the buffer, R_(j+1) = fl fr mlp_value_j(cat_c H^j_c R_j) (k_hodge_value) and P_(j+1) = R_(j+1) Wcat_(j+1) (k_gemm_p) for the layer behind
            const Route& rtp = pl->rt;
            if (!xa.P0 || (!rtp.h_general && !xa.P1)) return set_err(CCSD_ERR_RUNTIME, "tiled graph-network route: no hodge projections");
            if (p.h_L > 2 && !rtp.h_general) return set_err(CCSD_ERR_RUNTIME, "tiled graph-network route: more than two hodge layers need the general hodge stack");
            const int E = p.E, et = (E + 15) / 16;
            const unsigned char* edges = (const unsigned char*)pl->edges;
            const float* wts = (const float*)pl->w;
            const float rks = 1.0f / (float)sqrt((double)p.K);
            const long long qs = (long long)w.lg_hdq_stride, hs = (long long)w.lg_hdH_stride;
            int ch = p.a_nch_graph + p.a_cinit;
            CCSD_LAUNCH(k_lg_hd_qk0, dim3(grid_for(E + N, 256), B), blk, 0, stream, p.hl[0], p.a_nch_hodge, wts, edges, xa.P0, w.lg_S, ss, p.a_nch_graph, N, E,
                        w.lg_hdq, qs);
            for (int j = 1; j < p.h_L; ++j) {
                const HodgeLayerD& hp = ccsd_hl(p, j - 1);
                const HodgeLayerD& h = ccsd_hl(p, j);
                CCSD_LAUNCH(k_lg_hd_dense, dim3(et * (et + 1) / 2, B), blk, lg_hd_dense_lds(hp), stream, hp, pl->hdm[j - 1], rks, (const float*)pl->wp, edges,
                            (const float*)w.lg_hdq, qs, w.lg_hdH, hs, w.lg_S, ss, ch, N, E, xa.flags);
                ch += hp.cout;
                LAUNCH_CHECK();
                if (rtp.h_general && j + 1 < p.h_L)
                    if (int st = hodge_stack_layer(pl, B, j + 1, w, stream)) return st;
                const bool raw = j == 1 && !rtp.h_general && xa.p1_raw;
                LgHdRaw rw{};
                if (raw) {
                    if (!xa.U1) return set_err(CCSD_ERR_RUNTIME, "tiled graph-network route: raw hodge projections without their u_1");
                    rw = LgHdRaw{wts, (const float*)w.lg_S, xa.flags, edges, w.lg_hdpc, ss, N, p.hl[0].cin, p.hl[0].mval.w[0], p.hl[0].mval.b[0]};
                }
                const float* Pj = rtp.h_general ? (const float*)w.hgP[j - 1] : xa.P1;
                CCSD_LAUNCH(k_lg_hd_dis, dim3(grid_for((long long)h.cin * E, 256), B), blk, 0, stream, (const float*)w.lg_hdH, hs, h.cin, E, w.lg_hdd, rw);
                CCSD_LAUNCH(k_lg_hd_conv, dim3((et + 3) / 4, h.cin, B), blk, 0, stream, h, wts, (const float*)w.lg_hdH, hs, (const float*)w.lg_hdd, Pj, h.wc,
                            raw ? (const float*)w.lg_hdpc : (const float*)nullptr, raw ? xa.U1 : (const float*)nullptr, E, w.lg_hdq, qs);
                LAUNCH_CHECK();
            }
            if (rtp.h_wide) {
                CCSD_LAUNCH(k_lg_hd_diag_w, dim3(grid_for(E, 256), B), blk, 0, stream, ccsd_hl(p, p.h_L - 1), pl->hdm[p.h_L - 1], rks, (const float*)pl->wp, edges,
                            (const float*)w.lg_hdq, qs, w.lg_S, ss, ch, N, E, xa.flags);
            } else {
                CCSD_LAUNCH(k_lg_hd_diag, dim3(grid_for(E, 256), B), blk, 0, stream, ccsd_hl(p, p.h_L - 1), rks, wts, edges, (const float*)w.lg_hdq, qs, w.lg_S, ss,
                            ch, N, E, xa.flags);
            }
            LAUNCH_CHECK();
        }
        if (p.hb_L) {
            // hodge branch of ScoreNetworkA_Base_CC (k_lg_hb_*): input channels and layer 0's hidden rows; per layer but the last its dense
            // E x E output (the diagonal goes to the stack) and the next layer's hidden rows from it; the last layer on its diagonal only
            const int E = p.E, et = (E + 15) / 16;
            const unsigned char* edges = (const unsigned char*)pl->edges;
            const float* wts = (const float*)pl->w;
            const float* wpk = (const float*)pl->wp;
            int ch = p.a_nch_graph + p.a_cinit;
            CCSD_LAUNCH(k_lg_hb_in, dim3(grid_for(E + N, 256), B), blk, 0, stream, pl->hbx[0], p.a_nch_hodge, wts, edges, w.lg_S, ss, p.a_nch_graph, N, E,
                        w.lg_hbg, (long long)w.lg_hbg_stride);
            for (int l = 0; l + 1 < p.hb_L; ++l) {
                const HodgeBaseD& h = pl->hbx[l];
                const HodgeBaseD& hn = pl->hbx[l + 1];
                float* Hl = w.lg_hbH;
                CCSD_LAUNCH(k_lg_hb_dense, dim3(et * (et + 1) / 2, B), blk, lg_hb_dense_lds(h), stream, h, wts, wpk, edges, (const float*)w.lg_hbg,
                            (long long)w.lg_hbg_stride, Hl, (long long)w.lg_hbH_stride, w.lg_S, ss, ch, N, E, xa.flags);
                CCSD_LAUNCH(k_lg_hb_hid, dim3((et + 3) / 4, hn.cin, B), blk, 0, stream, hn, wts, wpk, (const float*)Hl, (long long)w.lg_hbH_stride, E,
                            w.lg_hbg, (long long)w.lg_hbg_stride);
                ch += h.cout;
            }
            CCSD_LAUNCH(k_lg_hb_diag, dim3(grid_for(E, 256), B), blk, 0, stream, pl->hbx[p.hb_L - 1], wts, edges, (const float*)w.lg_hbg,
                        (long long)w.lg_hbg_stride, w.lg_S, ss, ch, N, E, xa.flags);
            LAUNCH_CHECK();
        }
        for (int l = 0; l < p.a_L; ++l) {
            const AttnLayerD& L = p.al[l];
            const float* xin = l ? w.lg_x[(l - 1) & 1] : xa.xA;
            const float* wq = pl->wp + L.qkvp;                  // per channel [fin][cp] weights + [cp] biases (ccsd_pack_qkv)
            const int wcs = L.fin * L.cp + L.cp;
            CCSD_LAUNCH(k_lg_dis, dim3(grid_for((long long)L.cin * N, 256), B), blk, 0, stream, (const float*)w.lg_S, ss, L.ci0, L.cin, N, w.lg_dis);
            CCSD_LAUNCH(k_lg_xw, dim3(grid_for((long long)L.cin * N * L.cp, 256), B), blk, 0, stream, xin, (long long)N * L.fin, L.fin, L.fin,
                        wq, wcs, L.cp, L.cin, N, (const float*)w.lg_dis, w.lg_Y);
            CCSD_LAUNCH(k_lg_gcn, dim3(gt * cdiv(L.cp, CCSD_LG_GT), L.cin, B), blk, 0, stream, (const float*)w.lg_S, ss, L.ci0, (const float*)w.lg_Y,
                        (const float*)w.lg_dis, wq + L.fin * L.cp, wcs, L.cp, L.cp, L.cin, N, w.lg_QKV, (long long)L.cin * N * L.cp, N * L.cp, L.cp, 0, 0);
            // node update: tanh(mask_x(multi_channel(cat_c V_c)))
            CCSD_LAUNCH(k_lg_nmlp, dim3(rt, B), blk, lg_nmlp_lds_of(L.mc), stream, L.mc, (const float*)pl->w,
                        (LgGather{w.lg_QKV, (long long)L.cin * N * L.cp, N * L.cp, L.cp, 2 * L.adim, L.fout}), N, xa.flags, 1, w.lg_x[l & 1]);
            const float inv_scale = (float)sqrt((double)L.fout);     // attention.py:121: / math.sqrt(out_dim)
            CCSD_LAUNCH(k_lg_att, dim3(at * at, L.cin, B), blk, 0, stream, (const float*)w.lg_QKV, L.cp, L.adim, L.nchunk, L.dsplit, 1.0f / inv_scale,
                        0.5f / (float)L.nchunk, L.cin, N, w.lg_att);
            CCSD_LAUNCH(k_lg_edge, dim3(w.lg_tiles, B), blk, 0, stream, L.mlp, (const float*)pl->wp, (const float*)w.lg_att, w.lg_S, ss, L.ci0, L.co0,
                        L.cin, N);
            CCSD_LAUNCH(k_lg_sym, dim3(grid_for((long long)L.cout * NN, 256), B), blk, 0, stream, w.lg_S, ss, L.co0, L.cout, N, xa.flags);
            LAUNCH_CHECK();
        }
        if (pl->afin_lg.chain) {
            CCSD_LAUNCH(k_lg_fin_w, dim3(w.lg_tiles, B), blk, 0, stream, pl->afin_lg, (const float*)pl->wp, (const float*)w.lg_S, ss, N, xa.flags, xa.adjA,
                        xa, na, w.lg_part);
        } else {
            CCSD_LAUNCH(k_lg_fin, dim3(w.lg_tiles, B), blk, 0, stream, p.a_fin, (const float*)pl->wp, (const float*)w.lg_S, ss, N, xa.flags, xa.adjA,
                        xa, na, w.lg_part);
        }
        LAUNCH_CHECK();
    }
    CCSD_LAUNCH(k_lg_epi, dim3(B), blk, 0, stream, (const float*)w.lg_xnet, xa.xX, xa.flags, xa, na, (const float*)w.lg_part, w.lg_tiles, N, F);
    prof_mark(pl, KID_XA, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}

static int launch_hf(const ccsd_plan* pl, int B, const float* rank2, RankEpi& ep, NoiseArgs& na, Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    dim3 g(xcd_grid(B, ((p.K + T_BN - 1) / T_BN) * ((p.E + T_BM - 1) / T_BM)));
    prof_mark(pl, KID_HF, stream);
#define HF_ARGS (const PlanD*)pl->d, (const float*)pl->w, rank2, (const float*)w.H, (const unsigned long long*)w.offbits, \
                (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells, ep, na, B, w.masks()
    const int fw = fnet_width(p);
#define HF_AFF1(EC_, KC_) CCSD_LAUNCH((k_hf_score<true, 8, 1, EC_, KC_>), g, dim3(CCSD_NTHREADS), 0, stream, HF_ARGS)
#define HF_GEN1(EC_, KC_) CCSD_LAUNCH((k_hf_score<false, 8, 1, EC_, KC_>), g, dim3(CCSD_NTHREADS), 0, stream, HF_ARGS)
#define HF_GO(NP_) \
    do { \
        if (p.f_affine && NP_ == 1) GEO_EK(pl->rt.geo, HF_AFF1); \
        else if (p.f_affine) CCSD_LAUNCH((k_hf_score<true, 8, NP_>), g, dim3(CCSD_NTHREADS), 0, stream, HF_ARGS); \
        else if (fw <= 8 && NP_ == 1) GEO_EK(pl->rt.geo, HF_GEN1); \
        else if (fw <= 8) CCSD_LAUNCH((k_hf_score<false, 8, NP_>), g, dim3(CCSD_NTHREADS), 0, stream, HF_ARGS); \
        else if (fw <= CCSD_FW) CCSD_LAUNCH((k_hf_score<false, CCSD_FW, NP_>), g, dim3(CCSD_NTHREADS), 0, stream, HF_ARGS); \
        else CCSD_LAUNCH((k_hf_score<false, CCSD_FWMAX, NP_>), g, dim3(CCSD_NTHREADS), 0, stream, HF_ARGS); \
    } while (0)
    if (p.f_cnum <= 2) HF_GO(1); else HF_GO(CCSD_MAXCN - 1);
#undef HF_GO
#undef HF_AFF1
#undef HF_GEN1
#undef HF_ARGS
    prof_mark(pl, KID_HF, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// element-wise ScoreNetworkF (k_ew1).  ep: mode / scalars / out / mean / part as for k_hf_score; `net_out` (NORMS, nullable): keep the
// raw score; `cf` (PRED, nullable): fused corrector apply, F1 goes to `f1`
static int launch_ew1(const ccsd_plan* pl, int B, const float* rank2, RankEpi& ep, NoiseArgs& na, Workspace& w, void* stream,
                      float* net_out = nullptr, const CorrFuse* cf = nullptr, float* f1 = nullptr) {
    const PlanD& p = pl->h;
    Ew1Args a{};
    a.r = rank2; a.out = ep.out; a.mean = ep.mean; a.f1 = f1; a.net_out = net_out; a.part = ep.part;
    a.mode = ep.mode; a.apply = (cf && cf->on) ? 1 : 0;
    a.sscale = ep.sscale; a.pa = ep.pa; a.pb = ep.pb; a.pc = ep.pc; a.alpha = p.f_alpha; a.gamma = p.f_gamma;
    if (a.apply) {
        const LangCoef& lc = cf->lc;
        a.sums = lc.sums; a.ss = lc.ss[2]; a.sde_alpha = lc.alpha[2]; a.snr = lc.snr; a.seps = lc.seps; a.draw_corr = cf->draw_r;
    }
    a.E = p.E; a.K = p.K; a.mt = w.masks();
    prof_mark(pl, KID_EW1, stream);
#define EW1_GO(EC_, KC_) CCSD_LAUNCH((k_ew1<EC_, KC_>), dim3(w.nchunk, B), dim3(CCSD_NTHREADS), 0, stream, a, na)
    GEO_EK(pl->rt.geo, EW1_GO);
#undef EW1_GO
    prof_mark(pl, KID_EW1, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}

// merge_draw >= 0: merged launch -- after this (predictor) pass the kernel runs the NEXT corrector's norms pass on the new block
// (draw index merge_draw; raw score -> w.net_r, partials -> w.part or fold->part_next, projections -> the second buffer set)
// fold: the step's partial buffers when the launch reduces the batch norm sums itself (SumFold; launches with the fused apply only)
static int launch_r2(const ccsd_plan* pl, int B, const float* rank2, const float* adj, const float* flags, int want_p,
                     RankEpi& ep, NoiseArgs& na, Pass& ps, Workspace& w, void* stream, const CorrFuse* cf = nullptr, int merge_draw = -1,
                     const SumFold* fold) {
    const Route& rt = pl->rt;
    R2Args ra{};
    if (cf) ra.cf = *cf;
    // launches of the sampler loop that carry the fused corrector apply work on states this library produced: masked (R2Args::masked)
    ra.masked = (cf && cf->on) ? 1 : 0;
    const bool folded = fold && fold->part_in && cf && cf->on;
    if (merge_draw >= 0) {
        ra.merge = 1; ra.draw_r2 = (unsigned)merge_draw;
        ra.P0b = w.P0b; ra.P1b = w.P1b; ra.U1b = w.U1b; ra.net2 = w.net_r; ra.part2 = folded ? fold->part_next : w.part;
    }
    if (folded) { ra.fold = 1; ra.part_in = fold->part_in; ra.norm2 = w.norm2; ra.sums_out = w.sums; }
    ra.rank2 = rank2; ra.adj = adj; ra.flags = flags; ra.offbits = w.offbits; ra.P0 = w.P0; ra.P1 = w.P1; ra.U1 = w.U1; ra.want_p = want_p;
    ra.ldk = rt.r2_ldk; ra.ldh = rt.r2_ldh; ra.dbg = pl->dbg; ra.wp = pl->wp;
    if (want_p && pl->h.h_L > 1) ps.p1_raw = r2_p1_raw(pl->h);
    prof_mark(pl, KID_R2, stream);
    CCSD_LAUNCH(rt.r2->fn, dim3(B), dim3(CCSD_NTHREADS == 1 ? 1 : 512), rt.r2_lds, stream, (const PlanD*)pl->d, (const float*)pl->w,
                (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells, ra, ep, na);
    prof_mark(pl, KID_R2, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}

static inline int draws_per_step(const ccsd_config_t& cfg) { return cfg.predictor == CCSD_PRED_S4 ? 3 : cfg.n_corr_steps + 1; }   // (per target; S4: three)
static unsigned int draw_base(const ccsd_plan* pl, int step, int phase) { return 3u + (unsigned)((step * draws_per_step(pl->cfg) + phase) * 3); }
// work items of an element-wise pass over a state: the elements of x and adj + rank2's Philox groups of four (Route::corrector_flat)
static inline long long state_items(const PlanD& p, int B, int flat_r) {
    const long long r4 = flat_r ? ((long long)p.E * p.K + 3) / 4 : (long long)((p.E + 3) / 4) * p.K;
    return (long long)B * (p.N * p.F + p.N * p.N) + (p.is_cc ? (long long)B * r4 : 0);
}
static NoiseArgs make_noise(const ccsd_noise_t* n, uint64_t seed, int64_t off, unsigned int base, int flat_r = 0) {
    NoiseArgs na{};
    if (n) { na.zx = n->zx; na.zadj = n->zadj; na.zr = n->zrank2; }
    na.seed = seed; na.b_off = off;
    na.draw_x = base; na.draw_adj = base + 1; na.draw_r = base + 2;
    na.flat_r = flat_r;
    return na;
}

// the Langevin scalars of diffusion step `step` over the norm sums `sums` (k_normsum)
static LangCoef lang_coef(const ccsd_plan* pl, int step, const float* sums) {
    LangCoef lc{};
    lc.sums = sums;
    for (int t = 0; t < 3; ++t) {
        const ccsd_step_coef_t& c = pl->coef[(size_t)step * 3 + t];
        lc.ss[t] = c.sscale; lc.alpha[t] = c.alpha;
    }
    lc.snr = pl->h.snr; lc.seps = pl->h.seps;
    return lc;
}
// k_langevin_apply's arguments (k_s4_apply's first part): cur + the raw scores of the norms pass -> out
static LangArgs lang_args(const ccsd_plan* pl, int B, int step, const ccsd_state_t* cur, const float* flags, const float* sums,
                          ccsd_state_t* out, const Workspace& w) {
    const PlanD& p = pl->h;
    LangArgs a{};
    a.x = cur->x; a.adj = cur->adj; a.r = cur->rank2;
    a.nx = w.net_x; a.nadj = w.net_adj; a.nr = w.net_r;
    a.ox = out->x; a.oadj = out->adj; a.orr = out->rank2;
    a.flags = flags; a.lc = lang_coef(pl, step, sums);
    a.B = B; a.N = p.N; a.F = p.F; a.E = p.E; a.K = p.K; a.is_cc = p.is_cc;
    return a;
}
// the fields every P0Fuse mode fills: the corrector's flat-keyed rank2 draw `draw` of the stream `na` and the mask tables
static P0Fuse p0_fuse(const ccsd_plan* pl, int mode, const NoiseArgs& na, unsigned int draw, const Workspace& w) {
    P0Fuse pf{};
    pf.mode = mode; pf.seed = na.seed; pf.b_off = na.b_off; pf.draw = draw;
    pf.mt = w.masks(); pf.E = pl->h.E;
    return pf;
}
// the rank-2 predictor update of diffusion step `step` as an epilogue
static RankEpi pred_epi(const ccsd_plan* pl, int step, ccsd_state_t* out, ccsd_state_t* mean) {
    const ccsd_step_coef_t& c = pl->coef[(size_t)step * 3 + 2];
    RankEpi ep{};
    ep.mode = MODE_PRED; ep.pa = c.pa; ep.pb = c.pb; ep.pc = c.pc;
    ep.out = out->rank2; ep.mean = mean ? mean->rank2 : nullptr;
    return ep;
}
static RankEpi norms_epi(const Workspace& w) {
    RankEpi ep{};
    ep.mode = MODE_NORMS; ep.out = w.net_r; ep.part = w.part;
    return ep;
}
// dst <- src: the first `n` samples of the three tensors of a state, asynchronously on `stream`
static int copy_state(const ccsd_state_t& dst, const ccsd_state_t& src, const PlanD& p, size_t n, void* stream) {
    RT_CHECK(rt_d2d_async(dst.x, src.x, n * p.N * p.F * 4, stream));
    RT_CHECK(rt_d2d_async(dst.adj, src.adj, n * p.N * p.N * 4, stream));
    if (p.is_cc && p.E && p.K) RT_CHECK(rt_d2d_async(dst.rank2, src.rank2, n * p.E * p.K * 4, stream));
    return CCSD_OK;
}

// ---------------- API ----------------
extern "C" int ccsd_score(ccsd_plan_t* pl, int32_t target, int32_t B, const ccsd_state_t* in, const float* flags,
                          float sscale, float* out, void* workspace, size_t ws_bytes, void* stream) {
    Workspace w{};
    int st = check_common(pl, B, flags, workspace, ws_bytes, w);
    if (st) return st;
    if ((st = check_state(pl, in, "in"))) return st;
    if (!out) return set_err(CCSD_ERR_INVALID, "NULL out");
    if ((st = launch_flagbits(pl, B, flags, w, stream))) return st;
    NoiseArgs na{};
    Pass ps;
    if (target == CCSD_TARGET_X || target == CCSD_TARGET_ADJ) {
        XaArgs xa{};
        xa.xX = xa.xA = in->x; xa.adjX = xa.adjA = in->adj; xa.flags = flags;
        xa.do_x = target == CCSD_TARGET_X; xa.do_a = !xa.do_x; xa.mode = MODE_SCORE;
        xa.ss_x = xa.ss_a = sscale; xa.out_x = xa.out_a = out;
        if (xa.do_a && (st = launch_p(pl, B, in->adj, in->rank2, ps, w, stream))) return st;
        return launch_xa(pl, B, xa, na, ps, w, stream);
    }
    if (target == CCSD_TARGET_RANK2) {
        if (!pl->h.is_cc) return set_err(CCSD_ERR_INVALID, "rank2 score requested from a graph-only plan");
        RankEpi ep{};
        ep.mode = MODE_SCORE; ep.sscale = sscale; ep.out = out;
        if (pl->rt.r2_family == R2_FUSED) return launch_r2(pl, B, in->rank2, in->adj, flags, 0, ep, na, ps, w, stream);
        if (pl->rt.r2_family == R2_EW1) return launch_ew1(pl, B, in->rank2, ep, na, w, stream);
        if ((st = launch_h(pl, B, in->rank2, ps, w, stream))) return st;
        return launch_hf(pl, B, in->rank2, ep, na, w, stream);
    }
    return set_err(CCSD_ERR_UNSUPPORTED, "Object not yet supported. Select from [x, adj, rank2].");
}

// masked draws of one draw base into `state` (k_init_state): the prior for base 0, the noise of a half-step otherwise
static int draws_to_state(ccsd_plan* pl, int32_t B, const float* flags, const ccsd_noise_t* raw, uint64_t seed, int64_t sample_offset,
                          unsigned int base, ccsd_state_t* state, void* stream, int flat_r = 0) {
    if (!pl || B < 1 || !flags) return set_err(CCSD_ERR_INVALID, "bad argument");
    int st = check_state(pl, state, "state");
    if (st) return st;
    const PlanD& p = pl->h;
    // this call takes no workspace: the off-bit table lives in a plan-owned buffer that only ever grows, so the call stays
    // asynchronous on `stream`.  A plan is reentrant per handle only and its calls belong on ONE stream (include/ccsd_hip.h):
    // when the buffer has to grow, the whole device is drained first, whatever stream an earlier call used
    if (pl->init_off_cap < (size_t)B) {
        if (pl->init_off) {
#ifndef CCSD_EMU
            (void)hipDeviceSynchronize();
#endif
            (void)rt_free(pl->init_off);
            pl->init_off = nullptr; pl->init_off_cap = 0;
        }
        RT_CHECK(rt_malloc((void**)&pl->init_off, (size_t)B * 8));
        pl->init_off_cap = (size_t)B;
    }
    unsigned long long* offbits = pl->init_off;
    if (!pl->rt.lg || p.is_cc) CCSD_LAUNCH(k_flagbits, dim3(grid_for(B, 256)), dim3(CCSD_NTHREADS), 0, stream, flags, offbits, B, p.N);   // (graph-only plans of the tiled route: no rank-2 draws read it)
    NoiseArgs na = make_noise(raw, seed, sample_offset, base, flat_r);
    CCSD_LAUNCH(k_init_state, dim3(grid_for(state_items(p, B, flat_r), 256)), dim3(CCSD_NTHREADS), 0, stream, state->x, state->adj, state->rank2,
                flags, na, (const unsigned long long*)offbits, (const unsigned char*)pl->edges,
                (const unsigned long long*)pl->cells, B, p.N, p.F, p.E, p.K, p.is_cc);
    LAUNCH_CHECK();
    return CCSD_OK;
}

extern "C" int ccsd_init_state(ccsd_plan_t* pl, int32_t B, const float* flags, const ccsd_noise_t* prior, uint64_t seed,
                               int64_t sample_offset, ccsd_state_t* state, void* stream) {
    return draws_to_state(pl, B, flags, prior, seed, sample_offset, 0, state, stream);
}

extern "C" int ccsd_noise_draws(ccsd_plan_t* pl, int32_t B, const float* flags, uint64_t seed, int64_t sample_offset, int32_t step,
                                int32_t phase, ccsd_state_t* out, void* stream) {
    if (!pl) return set_err(CCSD_ERR_INVALID, "NULL plan");
    if (step < 0 || step >= pl->cfg.diff_steps || phase < 0 || phase >= draws_per_step(pl->cfg)) return set_err(CCSD_ERR_INVALID, "step / phase out of range");
    const bool corr = pl->cfg.predictor != CCSD_PRED_S4 && phase < pl->cfg.n_corr_steps && pl->cfg.corrector == CCSD_CORR_LANGEVIN;
    return draws_to_state(pl, B, flags, nullptr, seed, sample_offset, draw_base(pl, step, phase), out, stream,
                          corr ? pl->rt.corrector_flat : pl->rt.predictor_flat);
}

extern "C" int ccsd_noise_draws_at(ccsd_plan_t* pl, int32_t B, const float* flags, uint64_t seed, int64_t sample_offset, uint32_t draw,
                                   int32_t flat_rank2, ccsd_state_t* out, void* stream) {
    if (!pl) return set_err(CCSD_ERR_INVALID, "NULL plan");
    return draws_to_state(pl, B, flags, nullptr, seed, sample_offset, draw, out, stream, flat_rank2 ? 1 : 0);
}

extern "C" int ccsd_plan_query(const ccsd_plan_t* pl, int32_t what, int64_t* value) {
    if (!pl || !value) return set_err(CCSD_ERR_INVALID, "NULL argument");
    const Route& r = pl->rt;
    const int hint = pl->cfg.batch_hint;        // the batch the batch-dependent answers are given for
    switch (what) {
        case CCSD_QUERY_FUSED_R2: *value = r.r2_family == R2_FUSED; break;
        case CCSD_QUERY_XA_VARIANT: *value = r.xa_variant; break;
        case CCSD_QUERY_R2_LDS_BYTES: *value = (int64_t)r.r2_lds; break;
        case CCSD_QUERY_XA_LDS_BYTES: *value = (int64_t)pl->h.xa_lds_floats * 4; break;
        case CCSD_QUERY_FUSED_LOOP: *value = r.loop == LOOP_LANGEVIN_FUSED; break;
        case CCSD_QUERY_MERGED_R2: *value = r.merged; break;
        case CCSD_QUERY_FOLD_SUMS: *value = r.fold_sums; break;
        case CCSD_QUERY_FOLD_LAST_RUN: *value = pl->last_run_folded; break;
        case CCSD_QUERY_EW1: *value = r.r2_family == R2_EW1; break;
        case CCSD_QUERY_LARGE_GRAPH: *value = r.lg; break;
        case CCSD_QUERY_R2_FAMILY: *value = r.r2_family; break;
        case CCSD_QUERY_R2_INSTANCE: *value = r.r2 ? ((((int64_t)r.r2->mt * 10 + r.r2->rs) * 10 + r.r2->affine) * 10 + r.r2->gen1) * 10 + r.r2->qm9 : -1; break;
        case CCSD_QUERY_LOOP_FORM: *value = r.loop; break;
        case CCSD_QUERY_H_FULL: *value = use_h_full(r, hint); break;
        case CCSD_QUERY_HP_FULL: *value = (use_hp_full(r, hint, 2) ? 1 : 0) | (use_hp_full(r, hint, 1) ? 2 : 0); break;
        case CCSD_QUERY_P0_NARROW: *value = r.p0 >= 0 ? (int64_t)P0_TABLE[r.p0].nt * 100000 + P0_TABLE[r.p0].kc : 0; break;
        case CCSD_QUERY_TILED_FUSE: *value = r.tiled_fuse; break;
        case CCSD_QUERY_EW1_FUSE: *value = r.ew1_fuse; break;
        case CCSD_QUERY_H_GENERAL: *value = r.h_general; break;
        case CCSD_QUERY_GEO_EK: *value = r.geo; break;
        case CCSD_QUERY_H_WIDE: *value = r.h_wide; break;
        case CCSD_QUERY_MLP_FORMS: {
            int64_t edge = 0;
            for (int l = 0; l < pl->h.a_L; ++l) edge |= (int64_t)(pl->h.al[l].mlp.chain != 0) << l;
            const int afin = r.lg && pl->afin_lg.chain ? pl->afin_lg.chain : pl->h.a_fin.chain;
            *value = pl->h.x_fin.chain + 16 * afin + 256 * edge;
            break;
        }
        default: return set_err(CCSD_ERR_INVALID, "unknown query");
    }
    return CCSD_OK;
}

// phase 1 of the Langevin corrector.  `base` = pre-corrector state, `cur` = per-target current
// iterate (== base for the first inner step).
// r2_done: the rank-2 side of this norms pass (raw score, partials, hodge projections in the second buffer set) was already
// produced by the merged k_r2 launch of the previous predictor half-step
static int corrector_norms(ccsd_plan* pl, int B, int step, int it, const ccsd_state_t* base, const ccsd_state_t* cur,
                           const float* flags, const ccsd_noise_t* noise, uint64_t seed, int64_t off, float* sums,
                           Workspace& w, void* stream, bool keep_net = true, bool r2_done = false, const SumFold* fold = nullptr) {
    const PlanD& p = pl->h;
    int st = CCSD_OK;
    NoiseArgs na = make_noise(noise, seed, off, draw_base(pl, step, it), pl->rt.corrector_flat);
    // A-net sees (x_0, adj_cur, rank2_0): hodge projections from the base rank2, edge coefficients from adj_cur.
    // When the rank2 iterate is still the base state the fused kernel serves both the A-net's projections
    // and ScoreNetworkF in one pass over rank2.
    const Route& rt = pl->rt;
    Pass ps;
    // The rank-2 side of THIS pass, named once (same_r2: the rank2 iterate is still the base state; own_draw: the corrector's flat-keyed
    // draw is made in the kernels).  Rests on resolve_route: tiled_fuse only with R2_TILED, ew1_fuse only with R2_EW1, R2_NONE iff !is_cc
    enum { NR_NONE, NR_R2, NR_EW1_RIDE, NR_EW1, NR_TILED };     // NR_TILED: a k_r2 plan too, once its rank2 iterate has left the base state
    const bool same_r2 = cur->rank2 == base->rank2, own_draw = na.flat_r && !na.zr;
    const int form = !p.is_cc ? NR_NONE : rt.r2_family == R2_FUSED && same_r2 ? NR_R2 : rt.r2_family != R2_EW1 ? NR_TILED
                   : rt.ew1_fuse && own_draw && same_r2 ? NR_EW1_RIDE : NR_EW1;
    // ... NR_TILED with one hodge layer: the noise norm of the corrector's draw rides on the projection pass (P0Fuse mode 1), no k_noise_norm
    const bool z_rides = form == NR_TILED && rt.tiled_fuse && own_draw;
    RankEpi ep = norms_epi(w);
    // folded norm sums (the fused loop of k_r2 plans, form NR_R2 always): k_r2's partials go to the step's buffer and the predictor's k_r2
    // launch reduces them, with norm2, itself -- no k_normsum below, `sums` is written by that launch
    const bool folded = fold && fold->part_in;
    if (folded) ep.part = const_cast<float*>(fold->part_in);
    P0Fuse pf{};
    int ntiles = w.ntiles;       // partials per sample in w.part
    switch (form) {
    case NR_R2:             // k_r2, launched here or left by the merged launch of the previous predictor
        if (r2_done) ps.p1_raw = r2_p1_raw(p);          // (as the merged launch left the second buffer set)
        else if ((st = launch_r2(pl, B, cur->rank2, cur->adj, flags, 1, ep, na, ps, w, stream))) return st;
        ntiles = 1;
        break;
    case NR_EW1_RIDE:       // k_ew1 plans, one hodge layer: raw score + both norms per row ride on the projection pass, no k_ew1 launch
        pf = p0_fuse(pl, 3, na, na.draw_r, w);
        pf.zrow = w.part; pf.alpha = p.f_alpha; pf.gamma = p.f_gamma;
        pf.net_out = keep_net ? w.net_r : nullptr;
        ntiles = p.E;                            // (per-row partials written by the projection pass)
        break;
    case NR_TILED:
        if (z_rides) { pf = p0_fuse(pl, 1, na, na.draw_r, w); pf.zrow = w.zpart; }
        break;
    }
    if (form != NR_R2) st = launch_p(pl, B, cur->adj, base->rank2, ps, w, stream, pf.mode ? &pf : nullptr);
    if (st) return st;
    XaArgs xa{};
    xa.xX = cur->x; xa.adjX = base->adj;      // score_x(x_cur, adj_0)      solver.py:761
    xa.xA = base->x; xa.adjA = cur->adj;      // score_adj(x_0, adj_cur)    solver.py:775
    xa.flags = flags; xa.do_x = xa.do_a = 1; xa.mode = MODE_NORMS;
    xa.out_x = w.net_x; xa.out_a = w.net_adj; xa.norm2 = w.norm2;
    if ((st = launch_xa(pl, B, xa, na, ps, w, stream, form == NR_R2 && r2_done))) return st;
    if (form == NR_EW1) {
        // element-wise ScoreNetworkF: one streaming pass gives both norm partials per (sample, chunk); the raw score is kept only
        // for a separate ccsd_corrector_apply (the fused loop recomputes it)
        if ((st = launch_ew1(pl, B, cur->rank2, ep, na, w, stream, keep_net ? w.net_r : nullptr))) return st;
        ntiles = w.nchunk;
    } else if (form == NR_TILED) {
        if ((st = launch_h(pl, B, cur->rank2, ps, w, stream))) return st;
        if ((st = launch_hf(pl, B, cur->rank2, ep, na, w, stream))) return st;
    }
    const float* part = w.part;
    if (form != NR_NONE && form != NR_R2) {
        // tiled path: the noise norm of a flat-keyed Philox draw comes from its own (traffic-free) kernel; the per-tile partials of
        // k_hf_score and its chunk partials are reduced per sample first (one workgroup per sample), then over the batch
        const bool zk = form == NR_TILED && own_draw;
        if (zk && !z_rides) {
#define NN_GO(EC_, KC_) CCSD_LAUNCH((k_noise_norm<EC_, KC_>), dim3(w.nchunk, B), dim3(CCSD_NTHREADS), 0, stream, na, w.masks(), p.E, p.K, w.zpart)
            GEO_EK(pl->rt.geo, NN_GO);
#undef NN_GO
            LAUNCH_CHECK();
        }
        if (zk || ntiles > 8) {
            // (zpart: the chunk partials of k_noise_norm, or the E row partials of the fused projection pass)
            CCSD_LAUNCH(k_normpart, dim3(B), dim3(CCSD_NTHREADS), 0, stream, (const float*)w.part, ntiles, zk ? (const float*)w.zpart : (const float*)nullptr,
                        z_rides ? p.E : w.nchunk, w.part2);
            LAUNCH_CHECK();
            part = w.part2; ntiles = 1;
        }
    }
    if (folded) return form == NR_R2 ? CCSD_OK : set_err(CCSD_ERR_RUNTIME, "folded norm sums on a pass k_r2 does not serve");
    CCSD_LAUNCH(k_normsum, dim3(1), dim3(CCSD_NTHREADS == 1 ? 1 : normsum_threads(B)), 0, stream, (const float*)w.norm2, part, B, ntiles,
                p.is_cc, sums);
    LAUNCH_CHECK();
    return CCSD_OK;
}
static int corrector_apply(ccsd_plan* pl, int B, int step, int it, const ccsd_state_t* cur, const float* flags,
                           const ccsd_noise_t* noise, uint64_t seed, int64_t off, const float* sums, ccsd_state_t* out,
                           Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    NoiseArgs na = make_noise(noise, seed, off, draw_base(pl, step, it), pl->rt.corrector_flat);
    LangArgs a = lang_args(pl, B, step, cur, flags, sums, out, w);
    const long long total = state_items(p, B, 1);
    prof_mark(pl, KID_LANGEVIN, stream);
#define LA_GO(EC_, KC_) CCSD_LAUNCH((k_langevin_apply<EC_, KC_>), dim3(grid_for(total, 256)), dim3(CCSD_NTHREADS), 0, stream, a, na, w.masks())
    GEO_EK(pl->rt.geo, LA_GO);
#undef LA_GO
    prof_mark(pl, KID_LANGEVIN, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}
static int predictor(ccsd_plan* pl, int B, int step, const ccsd_state_t* in, const float* flags, const ccsd_noise_t* noise,
                     uint64_t seed, int64_t off, ccsd_state_t* out, ccsd_state_t* mean, Workspace& w, void* stream,
                     const float* fuse_sums = nullptr, bool merge_next = false, const SumFold* fold = nullptr) {
    const PlanD& p = pl->h;
    int st = CCSD_OK;
    NoiseArgs na = make_noise(noise, seed, off, draw_base(pl, step, pl->cfg.n_corr_steps), pl->rt.predictor_flat);
    const ccsd_step_coef_t* c = &pl->coef[(size_t)step * 3];
    const Route& rt = pl->rt;
    Pass ps;
    // The rank-2 side of THIS pass, named once as in corrector_norms (fuse_sums: the Langevin apply is fused in; na.zr: the host's rank2 draw)
    enum { PR_NONE, PR_R2, PR_EW1_ONEPASS, PR_EW1, PR_TILED_APPLY, PR_TILED };
    const int form = !p.is_cc ? PR_NONE : rt.r2_family == R2_FUSED ? PR_R2
                   : rt.r2_family == R2_EW1 ? (fuse_sums && rt.ew1_fuse && !na.zr ? PR_EW1_ONEPASS : PR_EW1)
                   : fuse_sums && rt.tiled_fuse ? PR_TILED_APPLY : PR_TILED;
    CorrFuse cf{};
    if (fuse_sums) {   // the Langevin corrector's apply pass runs in the prologues of this half-step's kernels
        cf.on = 1; cf.net_x = w.net_x; cf.net_adj = w.net_adj; cf.net_r = w.net_r; cf.lc = lang_coef(pl, step, fuse_sums);
        const unsigned int cb = draw_base(pl, step, 0);
        cf.draw_x = cb; cf.draw_adj = cb + 1; cf.draw_r = cb + 2;
    }
    RankEpi ep = pred_epi(pl, step, out, mean);
    P0Fuse pf{};
    const float* p_in = in->rank2;            // what the hodge projections are taken of
    const float* r2_in = in->rank2;           // what the rank-2 kernels of the tiled path read (the corrected state when the apply is fused)
    // merged launch: the rank-2 side of the NEXT step's norms pass follows in the same launch (its corrector draw: rank2 slot of
    // draw_base(step + 1, 0))
    const int md = merge_next ? (int)draw_base(pl, step + 1, 0) + 2 : -1;
    switch (form) {
    case PR_R2:
        if ((st = launch_r2(pl, B, in->rank2, in->adj, flags, 1, ep, na, ps, w, stream, &cf, md, fold))) return st;
        break;
    case PR_EW1_ONEPASS:    // k_ew1 plans, one hodge layer: corrector apply + projection + predictor update in ONE pass over rank2
        pf = p0_fuse(pl, 4, na, cf.draw_r, w);
        pf.draw_pred = na.draw_r; pf.cf = cf;
        pf.alpha = p.f_alpha; pf.gamma = p.f_gamma; pf.pa = c[2].pa; pf.pb = c[2].pb; pf.pc = c[2].pc;
        pf.out = out->rank2; pf.mean = mean ? mean->rank2 : nullptr;
        pf.f1 = w.net_r;                         // (host emulation only: its projection runs as a pass of its own over the corrected state)
        break;
    case PR_EW1:
        // element-wise ScoreNetworkF first: with the fused apply it produces the corrected rank2 (in the raw-score scratch, which
        // the fused loop does not fill) that the hodge projections of the A-network must see
        if ((st = launch_ew1(pl, B, in->rank2, ep, na, w, stream, nullptr, &cf, w.net_r))) return st;
        if (cf.on) p_in = w.net_r;
        break;
    case PR_TILED_APPLY:
        // tiled path, one hodge layer: the corrector apply rides on the projection pass -- corrected rank2 written in place over the raw
        // scores it consumes (w.net_r), P_0 taken of it; k_gemm_h / k_hf_score below read the corrected state from there
        pf = p0_fuse(pl, 2, na, cf.draw_r, w);
        pf.net = w.net_r; pf.f1 = w.net_r; pf.cf = cf;
        r2_in = w.net_r;
        break;
    }
    if (form != PR_R2) st = launch_p(pl, B, in->adj, p_in, ps, w, stream, pf.mode ? &pf : nullptr);
    if (st) return st;
    XaArgs xa{};
    xa.xX = xa.xA = in->x; xa.adjX = xa.adjA = in->adj; xa.flags = flags;
    xa.do_x = xa.do_a = 1; xa.mode = MODE_PRED;
    xa.pa_x = c[0].pa; xa.pb_x = c[0].pb; xa.pc_x = c[0].pc;
    xa.pa_a = c[1].pa; xa.pb_a = c[1].pb; xa.pc_a = c[1].pc;
    xa.out_x = out->x; xa.out_a = out->adj;
    xa.mean_x = mean ? mean->x : nullptr; xa.mean_a = mean ? mean->adj : nullptr;
    xa.cf = cf;
    if ((st = launch_xa(pl, B, xa, na, ps, w, stream))) return st;
    if (form == PR_TILED_APPLY || form == PR_TILED) {
        if ((st = launch_h(pl, B, r2_in, ps, w, stream))) return st;
        if ((st = launch_hf(pl, B, r2_in, ep, na, w, stream))) return st;
    }
    return CCSD_OK;
}

// update half of one S4 step (k_s4_apply); the norms pass of the step is corrector_norms(step, 0, cur, cur)
static int s4_apply(ccsd_plan* pl, int B, int step, const ccsd_state_t* cur, const float* flags, const ccsd_noise_t* n1,
                    const ccsd_noise_t* n2, const ccsd_noise_t* n3, uint64_t seed, int64_t off, const float* sums,
                    ccsd_state_t* out, ccsd_state_t* mean, Workspace& w, void* stream) {
    const PlanD& p = pl->h;
    S4Args q{};
    q.a = lang_args(pl, B, step, cur, flags, sums, out, w);
    for (int t = 0; t < 3; ++t) {
        const ccsd_step_coef_t& c = pl->coef[(size_t)step * 3 + t];
        q.m1[t] = c.m1; q.s1[t] = c.s1; q.d[t] = c.d; q.m2[t] = c.m2; q.s2[t] = c.s2;
    }
    q.mx = mean ? mean->x : nullptr; q.madj = mean ? mean->adj : nullptr; q.mr = mean ? mean->rank2 : nullptr;
    NoiseArgs na1 = make_noise(n1, seed, off, draw_base(pl, step, 0));
    NoiseArgs na2 = make_noise(n2, seed, off, draw_base(pl, step, 1));
    NoiseArgs na3 = make_noise(n3, seed, off, draw_base(pl, step, 2));
    prof_mark(pl, KID_S4, stream);
    CCSD_LAUNCH(k_s4_apply, dim3(grid_for(state_items(p, B, 0), 256)), dim3(CCSD_NTHREADS), 0, stream, q, na1, na2, na3,
                (const unsigned long long*)w.offbits, (const unsigned char*)pl->edges, (const unsigned long long*)pl->cells);
    prof_mark(pl, KID_S4, stream);
    LAUNCH_CHECK();
    return CCSD_OK;
}

static int check_step(const ccsd_plan* pl, int step) {
    if (step < 0 || step >= pl->cfg.diff_steps) return set_err(CCSD_ERR_INVALID, "step out of range");
    return CCSD_OK;
}

extern "C" int ccsd_corrector_norms(ccsd_plan_t* pl, int32_t B, int32_t step, int32_t corr_iter, const ccsd_state_t* base,
                                    const ccsd_state_t* cur, const float* flags, const ccsd_noise_t* noise, uint64_t seed,
                                    int64_t sample_offset, float* norm_sums, void* workspace, size_t ws_bytes, void* stream) {
    Workspace w{};
    int st = check_common(pl, B, flags, workspace, ws_bytes, w);
    if (st || (st = check_step(pl, step)) || (st = check_state(pl, base, "base")) || (st = check_state(pl, cur, "cur"))) return st;
    if (!norm_sums) return set_err(CCSD_ERR_INVALID, "NULL norm_sums");
    if ((st = launch_flagbits(pl, B, flags, w, stream))) return st;
    return corrector_norms(pl, B, step, corr_iter, base, cur, flags, noise, seed, sample_offset, norm_sums, w, stream);
}
extern "C" int ccsd_corrector_apply(ccsd_plan_t* pl, int32_t B, int32_t step, int32_t corr_iter, const ccsd_state_t* cur,
                                    const float* flags, const ccsd_noise_t* noise, uint64_t seed, int64_t sample_offset,
                                    const float* norm_sums, ccsd_state_t* out, void* workspace, size_t ws_bytes, void* stream) {
    Workspace w{};
    int st = check_common(pl, B, flags, workspace, ws_bytes, w);
    if (st || (st = check_step(pl, step)) || (st = check_state(pl, cur, "cur")) || (st = check_state(pl, out, "out"))) return st;
    if (!norm_sums) return set_err(CCSD_ERR_INVALID, "NULL norm_sums");
    if ((st = launch_flagbits(pl, B, flags, w, stream))) return st;
    return corrector_apply(pl, B, step, corr_iter, cur, flags, noise, seed, sample_offset, norm_sums, out, w, stream);
}
extern "C" int ccsd_predictor(ccsd_plan_t* pl, int32_t B, int32_t step, const ccsd_state_t* in, const float* flags,
                              const ccsd_noise_t* noise, uint64_t seed, int64_t sample_offset, ccsd_state_t* out,
                              ccsd_state_t* mean, void* workspace, size_t ws_bytes, void* stream) {
    Workspace w{};
    int st = check_common(pl, B, flags, workspace, ws_bytes, w);
    if (!st && pl->cfg.predictor == CCSD_PRED_S4) return set_err(CCSD_ERR_INVALID, "S4 plans step with ccsd_corrector_norms + ccsd_s4_apply");
    if (st || (st = check_step(pl, step)) || (st = check_state(pl, in, "in")) || (st = check_state(pl, out, "out"))) return st;
    if (mean && (st = check_state(pl, mean, "mean"))) return st;
    if (in->x == out->x || in->adj == out->adj || (pl->h.is_cc && in->rank2 == out->rank2))
        return set_err(CCSD_ERR_INVALID, "predictor cannot run in place");
    if ((st = launch_flagbits(pl, B, flags, w, stream))) return st;
    return predictor(pl, B, step, in, flags, noise, seed, sample_offset, out, mean, w, stream);
}

extern "C" int ccsd_s4_apply(ccsd_plan_t* pl, int32_t B, int32_t step, const ccsd_state_t* cur, const float* flags,
                             const ccsd_noise_t* noise1, const ccsd_noise_t* noise2, const ccsd_noise_t* noise3, uint64_t seed,
                             int64_t sample_offset, const float* norm_sums, ccsd_state_t* out, ccsd_state_t* mean,
                             void* workspace, size_t ws_bytes, void* stream) {
    Workspace w{};
    int st = check_common(pl, B, flags, workspace, ws_bytes, w);
    if (st || (st = check_step(pl, step)) || (st = check_state(pl, cur, "cur")) || (st = check_state(pl, out, "out"))) return st;
    if (mean && (st = check_state(pl, mean, "mean"))) return st;
    if (pl->cfg.predictor != CCSD_PRED_S4) return set_err(CCSD_ERR_INVALID, "ccsd_s4_apply needs a plan created with CCSD_PRED_S4");
    if (!norm_sums) return set_err(CCSD_ERR_INVALID, "NULL norm_sums");
    if ((st = launch_flagbits(pl, B, flags, w, stream))) return st;
    return s4_apply(pl, B, step, cur, flags, noise1, noise2, noise3, seed, sample_offset, norm_sums, out, mean, w, stream);
}

// The library loop; ccsd_sampler_run is this call without options.  The reduce hook is called once per norms pass, after its k_normsum
// has been enqueued and before any reader of w.sums is: the launches are the same with and without it -- except on plans with folded
// norm sums (Route::fold_sums), which drop the k_normsum launches only when there is no hook.
extern "C" int ccsd_sampler_run_ex(ccsd_plan_t* pl, int32_t B, const float* flags, uint64_t seed, int64_t sample_offset,
                                   int32_t first_step, int32_t last_step, ccsd_state_t* state, ccsd_state_t* scratch,
                                   ccsd_state_t* result, float* traj, void* workspace, size_t ws_bytes, void* stream,
                                   const ccsd_run_options_t* options) {
    Workspace w{};
    int st = check_common(pl, B, flags, workspace, ws_bytes, w);
    if (st || (st = check_state(pl, state, "state")) || (st = check_state(pl, scratch, "scratch")) ||
        (st = check_state(pl, result, "result"))) return st;
    if (first_step < 0 || last_step > pl->cfg.diff_steps || first_step >= last_step) return set_err(CCSD_ERR_INVALID, "bad step range");
    const Route& rt = pl->rt;
    const PlanD& p = pl->h;
    if ((st = launch_flagbits(pl, B, flags, w, stream))) return st;
    const size_t nx = (size_t)p.N * p.F, na = (size_t)p.N * p.N, nr = p.is_cc ? (size_t)p.E * p.K : 0;
    const bool folded = rt.fold_sums && !(options && options->reduce);
    pl->last_run_folded = folded;
    ccsd_state_t a = *state, b = *scratch;   // a = live buffer
    // exact multi-GPU mode: the caller all-reduces the six sums in place, ordered on `stream`
#define REDUCE_SUMS() do { if (options && options->reduce && options->reduce(w.sums, 6, stream, options->user)) \
                               return set_err(CCSD_ERR_CALLBACK, "the reduce hook of ccsd_sampler_run_ex failed"); } while (0)
    for (int step = first_step; step < last_step; ++step) {
        const bool lastone = step == last_step - 1;
        const bool want_mean = pl->cfg.denoise && (lastone || traj);
        if (rt.loop == LOOP_S4) {   // scores + first draw + norm sums at the state, then the element-wise S4 update: a -> b, swap
            if ((st = corrector_norms(pl, B, step, 0, &a, &a, flags, nullptr, seed, sample_offset, w.sums, w, stream))) return st;
            REDUCE_SUMS();
            if ((st = s4_apply(pl, B, step, &a, flags, nullptr, nullptr, nullptr, seed, sample_offset, w.sums, &b,
                               want_mean ? result : nullptr, w, stream))) return st;
            ccsd_state_t t = a; a = b; b = t;
        } else if (rt.loop == LOOP_LANGEVIN_FUSED) {
            // a -> [norms pass] ; [apply fused into the predictor kernels] -> b ; swap roles.  Merged k_r2 launches: the predictor's
            // k_r2 also runs the rank-2 side of the next step's norms pass on the block it has just produced (r2_done below)
            const bool r2_done = rt.merged && step > first_step;
            const bool merge_next = rt.merged && !lastone;
            // folded norm sums: no k_normsum launch -- the predictor's k_r2 reduces this step's partials (one of two buffers, by the
            // parity of the step within the call: its merged pass writes the next step's into the other) and norm2, and leaves w.sums
            // for the k_xa launch behind it.  A reduce hook needs the sums between two launches: today's launches then
            SumFold sf;
            if (folded) { const int par = (step - first_step) & 1; sf.part_in = par ? w.partb : w.part; sf.part_next = par ? w.part : w.partb; }
            if ((st = corrector_norms(pl, B, step, 0, &a, &a, flags, nullptr, seed, sample_offset, w.sums, w, stream, /*keep_net=*/rt.r2_family == R2_FUSED, r2_done, &sf))) return st;
            REDUCE_SUMS();
            // u_1 = fr . Wcat_1 depends on the flags alone: the run's first (general) k_r2 launch has just written it; the masked launches
            // of the loop leave both copies alone (R2Args::masked), so the second buffer set gets its copy once
            if (rt.merged && !r2_done && r2_p1_raw(p))
                RT_CHECK(rt_d2d_async(w.U1b, w.U1, (size_t)B * p.h_pw * 4, stream));
            if ((st = predictor(pl, B, step, &a, flags, nullptr, seed, sample_offset, &b, want_mean ? result : nullptr, w, stream, w.sums, merge_next, &sf))) return st;
            ccsd_state_t t = a; a = b; b = t;
        } else if (rt.loop == LOOP_LANGEVIN || (rt.loop == LOOP_LANGEVIN_MULTI && pl->cfg.n_corr_steps > 0)) {
            // a = base -> (corrector 0) -> b -> (corrector 1) -> third -> (corrector 2) -> b ... -> (predictor) -> a.  Every inner
            // iteration scores against the base state with its own target's tensor taken from the current iterate (corrector_norms).
            const ccsd_state_t* cur = &a;
            for (int it = 0; it < pl->cfg.n_corr_steps; ++it) {
                ccsd_state_t* out = (it & 1) ? &w.third : &b;
                if ((st = corrector_norms(pl, B, step, it, &a, cur, flags, nullptr, seed, sample_offset, w.sums, w, stream))) return st;
                REDUCE_SUMS();
                if ((st = corrector_apply(pl, B, step, it, cur, flags, nullptr, seed, sample_offset, w.sums, out, w, stream))) return st;
                cur = out;
            }
            if ((st = predictor(pl, B, step, cur, flags, nullptr, seed, sample_offset, &a, want_mean ? result : nullptr, w, stream))) return st;
        } else {      // a -> (predictor) -> b, then swap roles
            if ((st = predictor(pl, B, step, &a, flags, nullptr, seed, sample_offset, &b, want_mean ? result : nullptr, w, stream))) return st;
            ccsd_state_t t = a; a = b; b = t;
        }
        if (traj) {
            const ccsd_state_t* src = pl->cfg.denoise ? result : &a;
            float* slot = traj + (size_t)step * (nx + na + nr);      // (a slot holds the first sample's tensors back to back)
            if ((st = copy_state(ccsd_state_t{slot, slot + nx, slot + nx + na}, *src, p, 1, stream))) return st;
        }
    }
#undef REDUCE_SUMS
    if (a.x != state->x) st = copy_state(*state, a, p, B, stream);      // the live buffer ended up in `scratch`: bring the state home
    if (!st && !pl->cfg.denoise) st = copy_state(*result, a, p, B, stream);
    return st;
}
extern "C" int ccsd_sampler_run(ccsd_plan_t* pl, int32_t B, const float* flags, uint64_t seed, int64_t sample_offset,
                                int32_t first_step, int32_t last_step, ccsd_state_t* state, ccsd_state_t* scratch,
                                ccsd_state_t* result, float* traj, void* workspace, size_t ws_bytes, void* stream) {
    return ccsd_sampler_run_ex(pl, B, flags, seed, sample_offset, first_step, last_step, state, scratch, result, traj, workspace, ws_bytes, stream, nullptr);
}

// the plan-free entry points (operations on finished samples): a file of their own, sharing set_err, grid_for and the check macros
#include "ccsd_api_samples.h"
